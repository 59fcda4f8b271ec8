// libsimq: waypoints from dense paths -- skimage.measure.approximate_polygon decided in integers, then the pruning of
//   grid_waypoints_kernel    the back half of GridGraph.shortest_path                                     shortest_paths.pyx:139-154
//
// The rule is stated in include/simq.h and written once in waypoint_rule.h, which action_waypoints.hip shares; that header also says
// what is parallel inside a problem.  What is this kernel's own: the dense path is the caller's, int32 grid pixels in global memory, so
// its length and every point of it are checked first; the lines of the pruning read the grid; the tolerance is the problem's.
#include "batch_abi.h"
#include "waypoint_rule.h"
#include "../../include/simq.h"

#include <vector>

namespace simq {

namespace {

using grid_spfa::kLanes;
constexpr int kMaxPath = SIMQ_GRID_WAYPOINTS_MAX_PATH;
constexpr int kMaxSide = 1 << 15;
static_assert(kMaxPath % 32 == 0 && kMaxPath > SIMQ_GRID_PATH_MAX_BOX_CELLS, "every path simq_grid_paths writes has its flag");

__device__ __forceinline__ bool descriptor_ok(const simq_grid_waypoint_problem& p, int64_t grids_bytes, int64_t path_pairs, int64_t way_pairs) {
    if (p.rows < 1 || p.cols < 1 || p.rows > kMaxSide || p.cols > kMaxSide || (int64_t)p.rows * p.cols >= SIMQ_GRID_MAX_CELLS) return false;
    if (p.grid_offset < 0 || p.grid_offset > grids_bytes - (int64_t)p.rows * p.cols) return false;
    if (p.path_offset < 0 || p.path_offset >= path_pairs) return false;
    if (p.way_capacity < 1 || p.way_offset < 0 || p.way_offset > way_pairs - p.way_capacity) return false;
    return p.tolerance >= 1 && p.tolerance <= 255;
}

__global__ void __launch_bounds__(kLanes) grid_waypoints_kernel(const uint8_t* __restrict__ grids, int64_t grids_bytes,
                                                                const int2* __restrict__ paths, int64_t path_pairs,
                                                                const int32_t* __restrict__ lengths,
                                                                const int32_t* __restrict__ path_status,
                                                                const simq_grid_waypoint_problem* __restrict__ probs,
                                                                int2* __restrict__ ways, int64_t way_pairs,
                                                                int32_t* __restrict__ counts, int32_t* __restrict__ status) {
    __shared__ uint32_t keep[kMaxPath / 32];
    const simq_grid_waypoint_problem p = probs[blockIdx.x];
    const int lane = threadIdx.x;
    if (!descriptor_ok(p, grids_bytes, path_pairs, way_pairs)) {
        if (lane == 0) status[blockIdx.x] = 2;          // (the host validated already: nothing is read or written)
        return;
    }
    const int found = path_status[blockIdx.x];
    if (found == 1 || found == 3) {                     // a clear straight line; a dense path cut short by its capacity
        if (lane == 0) {
            status[blockIdx.x] = 1;
            counts[blockIdx.x] = found == 1 ? 0 : -1;
        }
        return;
    }
    const int n = lengths[blockIdx.x];
    if (found != 0 || n < 1 || n > kMaxPath || (int64_t)n > path_pairs - p.path_offset) {
        if (lane == 0) status[blockIdx.x] = 2;
        return;
    }
    const int R = p.rows, C = p.cols;
    const uint8_t* g = grids + p.grid_offset;
    const int2* path = paths + p.path_offset;

    // ---- every point inside the grid (and so below 2^15: what keeps the products below in range and the lines inside the grid)
    {
        bool outside = false;
        for (int k = lane; k < n; k += kLanes) {
            const int2 q = path[k];
            outside |= (unsigned)q.x >= (unsigned)R || (unsigned)q.y >= (unsigned)C;
        }
        if (__any(outside)) {
            if (lane == 0) status[blockIdx.x] = 2;
            return;
        }
    }

    // ---- simplify, prune, and the kept points last first (waypoint_rule.h)
    int2* way = ways + p.way_offset;
    int total = 0;
    const int st = waypoint_rule::waypoints(
        keep, n, (unsigned long long)(p.tolerance * p.tolerance), p.way_capacity, [&](int k) { return path[k]; },
        [&](int r, int c) { return g[r * C + c] != 1; }, [&](int at, int2 q) { way[at] = q; }, lane, &total);
    if (lane == 0) {
        if (st == 0) counts[blockIdx.x] = total;
        status[blockIdx.x] = st != 0 ? st : (total > p.way_capacity ? 3 : 0);
    }
}

}  // namespace

}  // namespace simq

using namespace simq;

extern "C" int simq_grid_waypoints(const uint8_t* d_grids, int64_t grids_bytes, const int32_t* d_paths, int64_t path_pairs,
                                   const int32_t* d_lengths, const int32_t* d_path_status, const simq_grid_waypoint_problem* problems,
                                   int n, simq_grid_waypoint_problem* d_problems, int32_t* d_ways, int64_t way_pairs, int32_t* d_counts,
                                   int32_t* d_status, void* stream) {
    SIMQ_REQUIRE(d_grids && d_paths && d_lengths && d_path_status && problems && d_problems && d_ways && d_counts && d_status,
                 "grid_waypoints: NULL pointer");
    SIMQ_REQUIRE(n >= 1 && n <= (1 << 24), "grid_waypoints: n = %d (1 .. 2^24 problems)", n);
    SIMQ_REQUIRE(grids_bytes >= 1 && path_pairs >= 1 && way_pairs >= 1 && path_pairs <= ((int64_t)1 << 40) && way_pairs <= ((int64_t)1 << 40),
                 "grid_waypoints: extents of %lld bytes of d_grids, %lld pairs of d_paths, %lld pairs of d_ways (each >= 1, pairs <= 2^40)",
                 (long long)grids_bytes, (long long)path_pairs, (long long)way_pairs);
    std::vector<Span> way_spans;
    way_spans.reserve(n);
    for (int i = 0; i < n; ++i) {
        const simq_grid_waypoint_problem& p = problems[i];
        SIMQ_REQUIRE(p.rows >= 1 && p.cols >= 1 && p.rows <= kMaxSide && p.cols <= kMaxSide && (int64_t)p.rows * p.cols < SIMQ_GRID_MAX_CELLS,
                     "grid_waypoints: problem %d is %d x %d (rows, cols in 1 .. 2^15, rows * cols < 2^22)", i, p.rows, p.cols);
        SIMQ_REQUIRE(p.tolerance >= 1 && p.tolerance <= 255, "grid_waypoints: problem %d: tolerance = %d (1 .. 255)", i, p.tolerance);
        const int64_t cells = (int64_t)p.rows * p.cols;
        SIMQ_REQUIRE(fits(p.grid_offset, cells, grids_bytes),
                     "grid_waypoints: problem %d: grid_offset: bytes [%lld, %lld) outside the %lld of d_grids", i, (long long)p.grid_offset,
                     (long long)(p.grid_offset + cells), (long long)grids_bytes);
        SIMQ_REQUIRE(fits(p.path_offset, 1, path_pairs),
                     "grid_waypoints: problem %d: path_offset: pair %lld outside the %lld of d_paths", i, (long long)p.path_offset,
                     (long long)path_pairs);
        SIMQ_REQUIRE(p.way_capacity >= 1, "grid_waypoints: problem %d: way_capacity = %d (>= 1 pair)", i, p.way_capacity);
        SIMQ_REQUIRE(fits(p.way_offset, p.way_capacity, way_pairs),
                     "grid_waypoints: problem %d: way_offset: pairs [%lld, %lld) outside the %lld of d_ways", i, (long long)p.way_offset,
                     (long long)(p.way_offset + p.way_capacity), (long long)way_pairs);
        way_spans.push_back({(uint64_t)p.way_offset, (uint64_t)(p.way_offset + p.way_capacity), i});
    }
    const size_t o = first_overlap(way_spans);
    SIMQ_REQUIRE(o == 0, "grid_waypoints: problems %d and %d overlap in d_ways at pair %lld", way_spans[o - 1].problem, way_spans[o].problem,
                 (long long)way_spans[o].lo);

    const Buffer bufs[] = {
        {"d_grids", d_grids, grids_bytes, false},
        {"d_paths", d_paths, 8 * path_pairs, false},
        {"d_lengths", d_lengths, 4 * (int64_t)n, false},
        {"d_path_status", d_path_status, 4 * (int64_t)n, false},
        {"d_problems", d_problems, (int64_t)sizeof(simq_grid_waypoint_problem) * n, true},
        {"d_ways", d_ways, 8 * way_pairs, true},
        {"d_counts", d_counts, 4 * (int64_t)n, true},
        {"d_status", d_status, 4 * (int64_t)n, true},
    };
    const int align[] = {1, 8, 4, 4, 8, 8, 4, 4};
    const int nb = (int)(sizeof(bufs) / sizeof(bufs[0]));
    for (int a = 0; a < nb; ++a)
        SIMQ_REQUIRE((uintptr_t)bufs[a].p % align[a] == 0, "grid_waypoints: %s is not %d-byte aligned", bufs[a].name, align[a]);
    int a = 0, b = 0;
    SIMQ_REQUIRE(!first_conflict(bufs, nb, &a, &b), "grid_waypoints: %s and %s overlap", bufs[a].name, bufs[b].name);

    hipStream_t s = static_cast<hipStream_t>(stream);
    const HostBlock block = {problems, sizeof(simq_grid_waypoint_problem) * (size_t)n};
    SIMQ_CHECK_HIP(upload_descriptors(d_problems, &block, 1, nullptr, s));
    grid_waypoints_kernel<<<n, kLanes, 0, s>>>(d_grids, grids_bytes, reinterpret_cast<const int2*>(d_paths), path_pairs, d_lengths,
                                               d_path_status, d_problems, reinterpret_cast<int2*>(d_ways), way_pairs, d_counts, d_status);
    SIMQ_CHECK_LAUNCH();
    note_launch("grid_simplify");
    return 0;
}
