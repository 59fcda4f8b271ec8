// libsimq: from a robot's pixel pair to its waypoint pixels in one launch -- OccupancyMap.shortest_path between the two conversions
//   action_waypoints_kernel  straight-line test, snap, GridGraph._spfa, the walk, approximate_polygon decided in integers, the pruning
//                            envs.py:2483-2490, shortest_paths.pyx:69-154
//
// The search and the stages in front of it are grid_spfa.h's, shared with grid_paths_kernel (grid_waypoints.hip); the simplification,
// the pruning and the reversed output are waypoint_rule.h's, shared with grid_waypoints_kernel (grid_simplify.hip).  The rules are
// those of include/simq.h and the two headers say what is parallel.  What is this kernel's own:
//   * the three maps of a problem come from three bases (configuration space, thin map, closest cells), read where a BatchedMapper
//     keeps them; the window is the caller's, and the pass over the grid that refuses a free cell outside it stays;
//   * the dense path never leaves LDS.  When the queue has drained, the fp32 distances and the ring are dead: the walk writes the path
//     as 16-bit (row, column) pairs of the window (halo included, so a point is also the index of its flag byte) where the distances
//     lay -- a path has at most as many points as the window has free cells, 4 bytes each -- and the kept flags are a bit mask where
//     the ring lay (one bit a point against two bytes a free cell).  The rule compares differences of coordinates only, so
//     window coordinates decide as grid coordinates do; they are below 2^15 by the cap on the window;
//   * the pruning's lines join two points of one path, which lie in the window, so they read the flag bytes: bit 2 is set where the
//     cell of the configuration space is 1 (bit 0, free, is != 0: the search and the line test differ on a cell of 2 .. 255);
//   * an upstream word that is not 0 ends the problem before anything of it is read.
#include "batch_abi.h"
#include "grid_spfa.h"
#include "waypoint_rule.h"
#include "../../include/simq.h"

#include <algorithm>
#include <vector>

namespace simq {

namespace {

using namespace grid_spfa;

static_assert(SIMQ_GRID_WAYPOINTS_MAX_PATH >= SIMQ_GRID_PATH_MAX_BOX_CELLS, "a path has at most as many points as its window has cells");
static_assert(SIMQ_GRID_PATH_MAX_BOX_CELLS / 3 < (1 << 15), "window coordinates fit 16 bits and keep the rule's products in range");

struct Extents {
    int64_t cspace_bytes, thin_bytes, closest_ints, way_pairs;
    int n_upstream;
};

__device__ __forceinline__ bool descriptor_ok(const simq_action_waypoint_problem& p, const uint8_t* thin, const int32_t* closest,
                                              const Extents& x) {
    if (p.rows < 1 || p.cols < 1 || (int64_t)p.rows * p.cols >= SIMQ_GRID_MAX_CELLS) return false;
    const int64_t cells = (int64_t)p.rows * p.cols;
    if (p.src_i < 0 || p.src_i >= p.rows || p.src_j < 0 || p.src_j >= p.cols) return false;
    if (p.tgt_i < 0 || p.tgt_i >= p.rows || p.tgt_j < 0 || p.tgt_j >= p.cols) return false;
    if (p.cspace_offset < 0 || p.cspace_offset > x.cspace_bytes - cells) return false;
    if (p.thin_offset < -1 || (p.thin_offset >= 0 && (!thin || p.thin_offset > x.thin_bytes - cells))) return false;
    if (p.closest_offset < -1 || (p.closest_offset >= 0 && (!closest || p.closest_offset > x.closest_ints - 2 * cells))) return false;
    if (p.way_capacity < 1 || p.way_offset < 0 || p.way_offset > x.way_pairs - p.way_capacity) return false;
    if (p.box_rows < 0 || p.box_cols < 0 || p.box_i0 < 0 || p.box_j0 < 0 || p.box_i0 > p.rows - p.box_rows ||
        p.box_j0 > p.cols - p.box_cols)
        return false;
    if ((int64_t)(p.box_rows + 2) * (p.box_cols + 2) > SIMQ_GRID_PATH_MAX_BOX_CELLS) return false;
    return p.upstream >= -1 && p.upstream < x.n_upstream;
}

__global__ void __launch_bounds__(kLanes) action_waypoints_kernel(const uint8_t* __restrict__ cspace, const uint8_t* __restrict__ thins,
                                                                  const int32_t* __restrict__ closest,
                                                                  const simq_action_waypoint_problem* __restrict__ probs,
                                                                  int2* __restrict__ ways, int32_t* __restrict__ counts,
                                                                  int32_t* __restrict__ endpoints, const int32_t* __restrict__ upstream,
                                                                  int32_t* __restrict__ status, Extents ext, unsigned lds_have) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const simq_action_waypoint_problem p = probs[blockIdx.x];
    const int lane = threadIdx.x;
    if (!descriptor_ok(p, thins, closest, ext) || lds_bytes(p.box_rows, p.box_cols) > (int64_t)lds_have || (p.upstream >= 0 && !upstream)) {
        if (lane == 0) status[blockIdx.x] = 2;          // (the host validated already: nothing is read or written)
        return;
    }
    if (p.upstream >= 0) {
        const int word = upstream[p.upstream];
        if (word != 0) {                                // e.g. a configuration space without a free cell: its closest cells are undefined
            if (lane == 0) {
                status[blockIdx.x] = word;
                counts[blockIdx.x] = 0;
            }
            return;
        }
    }
    const int R = p.rows, C = p.cols, n_cells = R * C;
    const uint8_t* g = cspace + p.cspace_offset;
    int si = p.src_i, sj = p.src_j, ti = p.tgt_i, tj = p.tgt_j;

    // ---- OccupancyMap.shortest_path's straight-line test, on the pixels as given (envs.py:2483-2485)
    if (p.thin_offset >= 0) {
        const uint8_t* thin = thins + p.thin_offset;
        if (!line_hits([&](int r, int c) { return thin[r * C + c] != 1; }, si, sj, ti, tj, lane)) {
            if (lane == 0) {
                status[blockIdx.x] = 1;
                counts[blockIdx.x] = 0;
                int32_t* e = endpoints + 4 * (int64_t)blockIdx.x;
                e[0] = si; e[1] = sj; e[2] = ti; e[3] = tj;
            }
            return;
        }
    }
    // ---- OccupancyMap._closest_valid_cspace_indices (envs.py:2488-2489, 2522-2523)
    if (p.closest_offset >= 0) {
        const int32_t* cl = closest + p.closest_offset;
        if (!snap(cl, R, C, si, sj) || !snap(cl, R, C, ti, tj)) {
            if (lane == 0) status[blockIdx.x] = 2;
            return;
        }
    }

    // ---- every free cell must lie inside the declared window
    const Window box = {p.box_i0, p.box_j0, p.box_rows, p.box_cols};
    if (!free_cells_inside(g, n_cells, C, box, lane)) {
        if (lane == 0) status[blockIdx.x] = 2;
        return;
    }

    // ---- the search over the window + halo, in LDS; the flag bytes keep kOne for the pruning
    const Lds lds(smem, box);
    const float inf = 2.f * (float)n_cells;              // self.inf = 2 * max_num_verts (exact: < 2^24)
    const bool tgt_in = box.holds(ti, tj);
    const int s_l = box.holds(si, sj) ? lds.index(box, si, sj) : -1;
    const int vertices = init_window<true>(lds, g, C, box, s_l, inf, lane);
    const bool searched = s_l >= 0 && (lds.flg[s_l] & kFree) != 0;   // edges leave a free cell only: a blocked source relaxes nothing
    int st = searched ? search<true>(lds, s_l, vertices + 1, lane) : 0;
    if (st != 0) {
        if (lane == 0) status[blockIdx.x] = st;
        return;
    }
    int2* way = ways + p.way_offset;
    int32_t* e = endpoints + 4 * (int64_t)blockIdx.x;

    // ---- a path of the target alone (an unreachable or blocked target, a blocked source, target == source, either outside the window)
    if (!searched || !tgt_in) {
        if (lane == 0) {
            way[0] = make_int2(ti, tj);
            counts[blockIdx.x] = 1;
            e[0] = si; e[1] = sj; e[2] = ti; e[3] = tj;
            status[blockIdx.x] = 0;
        }
        return;
    }

    // ---- the walk from the target (shortest_paths.pyx:126-137): window coordinates where the distances lay
    ushort2* path = reinterpret_cast<ushort2*>(smem);
    uint32_t* keep = reinterpret_cast<uint32_t*>(lds.ring);
    const int W = lds.W, N = lds.N;
    int n = 0;
    if (lane == 0) {
        int i = ti - box.i0 + 1, j = tj - box.j0 + 1;
        int v = i * W + j;
        path[0] = make_ushort2((unsigned short)i, (unsigned short)j);
        n = 1;
        while (v != s_l && n < N) {
            const int pk = lds.par[v];
            if (pk == kNoParent) break;
            i -= dir_di(pk);
            j -= dir_dj(pk);
            v -= dir_di(pk) * W + dir_dj(pk);
            path[n] = make_ushort2((unsigned short)i, (unsigned short)j);
            ++n;
        }
        if (v != s_l && n >= N) n = -1;                 // (a walk longer than the window has cells: the parents hold a cycle)
    }
    n = __shfl(n, 0, kLanes);
    if (n < 0) {
        if (lane == 0) status[blockIdx.x] = 4;
        return;
    }

    // ---- simplify (tolerance 1), prune, and the kept points last first as pixels of the grid (waypoint_rule.h)
    const uint8_t* flg = lds.flg;
    const int oi = box.i0 - 1, oj = box.j0 - 1;
    int total = 0;
    st = waypoint_rule::waypoints(
        keep, n, 1ull, p.way_capacity, [&](int k) { const ushort2 q = path[k]; return make_int2((int)q.x, (int)q.y); },
        [&](int r, int c) { return (flg[r * W + c] & kOne) == 0u; }, [&](int at, int2 q) { way[at] = make_int2(q.x + oi, q.y + oj); },
        lane, &total);
    if (lane == 0) {
        if (st == 0) {
            counts[blockIdx.x] = total;
            e[0] = si; e[1] = sj; e[2] = ti; e[3] = tj;
        }
        status[blockIdx.x] = st != 0 ? st : (total > p.way_capacity ? 3 : 0);
    }
}

}  // namespace

}  // namespace simq

using namespace simq;

extern "C" int simq_action_waypoints(const uint8_t* d_cspace, int64_t cspace_bytes, const uint8_t* d_thin, int64_t thin_bytes,
                                     const int32_t* d_closest, int64_t closest_ints, const simq_action_waypoint_problem* problems, int n,
                                     simq_action_waypoint_problem* d_problems, int32_t* d_ways, int64_t way_pairs, int32_t* d_counts,
                                     int32_t* d_endpoints, const int32_t* d_upstream, int n_upstream, int32_t* d_status, void* stream) {
    SIMQ_REQUIRE(d_cspace && problems && d_problems && d_ways && d_counts && d_endpoints && d_status, "action_waypoints: NULL pointer");
    SIMQ_REQUIRE(n >= 1 && n <= (1 << 24), "action_waypoints: n = %d (1 .. 2^24 problems)", n);
    SIMQ_REQUIRE(cspace_bytes >= 1 && way_pairs >= 1 && way_pairs <= ((int64_t)1 << 40) && thin_bytes >= 0 && closest_ints >= 0,
                 "action_waypoints: extents of %lld bytes of d_cspace, %lld of d_thin, %lld ints of d_closest, %lld pairs of d_ways "
                 "(d_cspace and d_ways >= 1, pairs <= 2^40, none negative)", (long long)cspace_bytes, (long long)thin_bytes,
                 (long long)closest_ints, (long long)way_pairs);
    SIMQ_REQUIRE(n_upstream >= 0 && (n_upstream == 0) == (d_upstream == nullptr),
                 "action_waypoints: d_upstream and n_upstream = %d (NULL with 0, or n_upstream >= 1 words)", n_upstream);
    std::vector<Span> way_spans;
    way_spans.reserve(n);
    int64_t lds = 0;
    for (int i = 0; i < n; ++i) {
        const simq_action_waypoint_problem& p = problems[i];
        SIMQ_REQUIRE(p.rows >= 1 && p.cols >= 1 && (int64_t)p.rows * p.cols < SIMQ_GRID_MAX_CELLS,
                     "action_waypoints: problem %d is %d x %d (rows, cols >= 1, rows * cols < 2^22)", i, p.rows, p.cols);
        SIMQ_REQUIRE(p.src_i >= 0 && p.src_i < p.rows && p.src_j >= 0 && p.src_j < p.cols,
                     "action_waypoints: problem %d: source (%d, %d) outside its %d x %d grid", i, p.src_i, p.src_j, p.rows, p.cols);
        SIMQ_REQUIRE(p.tgt_i >= 0 && p.tgt_i < p.rows && p.tgt_j >= 0 && p.tgt_j < p.cols,
                     "action_waypoints: problem %d: target (%d, %d) outside its %d x %d grid", i, p.tgt_i, p.tgt_j, p.rows, p.cols);
        const int64_t cells = (int64_t)p.rows * p.cols;
        SIMQ_REQUIRE(fits(p.cspace_offset, cells, cspace_bytes),
                     "action_waypoints: problem %d: cspace_offset: bytes [%lld, %lld) outside the %lld of d_cspace", i,
                     (long long)p.cspace_offset, (long long)(p.cspace_offset + cells), (long long)cspace_bytes);
        SIMQ_REQUIRE(p.thin_offset == -1 || (d_thin && fits(p.thin_offset, cells, thin_bytes)),
                     "action_waypoints: problem %d: thin_offset: bytes [%lld, %lld) outside the %lld of d_thin (-1: no straight-line test)", i,
                     (long long)p.thin_offset, (long long)(p.thin_offset + cells), (long long)(d_thin ? thin_bytes : 0));
        SIMQ_REQUIRE(p.closest_offset == -1 || (d_closest && fits(p.closest_offset, 2 * cells, closest_ints)),
                     "action_waypoints: problem %d: closest_offset: ints [%lld, %lld) outside the %lld of d_closest (-1: no snap)", i,
                     (long long)p.closest_offset, (long long)(p.closest_offset + 2 * cells), (long long)(d_closest ? closest_ints : 0));
        SIMQ_REQUIRE(p.box_rows >= 0 && p.box_cols >= 0 && p.box_i0 >= 0 && p.box_j0 >= 0 && p.box_i0 <= p.rows - p.box_rows &&
                         p.box_j0 <= p.cols - p.box_cols,
                     "action_waypoints: problem %d: window rows [%d, %d + %d), columns [%d, %d + %d) outside its %d x %d grid", i, p.box_i0,
                     p.box_i0, p.box_rows, p.box_j0, p.box_j0, p.box_cols, p.rows, p.cols);
        SIMQ_REQUIRE((int64_t)(p.box_rows + 2) * (p.box_cols + 2) <= SIMQ_GRID_PATH_MAX_BOX_CELLS,
                     "action_waypoints: problem %d: window of %d x %d cells plus its halo is %lld cells, over SIMQ_GRID_PATH_MAX_BOX_CELLS = %d "
                     "(the search state lives in LDS)", i, p.box_rows, p.box_cols, (long long)(p.box_rows + 2) * (p.box_cols + 2),
                     SIMQ_GRID_PATH_MAX_BOX_CELLS);
        SIMQ_REQUIRE(p.way_capacity >= 1, "action_waypoints: problem %d: way_capacity = %d (>= 1 pair)", i, p.way_capacity);
        SIMQ_REQUIRE(fits(p.way_offset, p.way_capacity, way_pairs),
                     "action_waypoints: problem %d: way_offset: pairs [%lld, %lld) outside the %lld of d_ways", i, (long long)p.way_offset,
                     (long long)(p.way_offset + p.way_capacity), (long long)way_pairs);
        SIMQ_REQUIRE(p.upstream >= -1 && p.upstream < n_upstream, "action_waypoints: problem %d: upstream = %d (-1, or a word of the %d of d_upstream)",
                     i, p.upstream, n_upstream);
        way_spans.push_back({(uint64_t)p.way_offset, (uint64_t)(p.way_offset + p.way_capacity), i});
        lds = std::max(lds, lds_bytes(p.box_rows, p.box_cols));
    }
    const size_t o = first_overlap(way_spans);
    SIMQ_REQUIRE(o == 0, "action_waypoints: problems %d and %d overlap in d_ways at pair %lld", way_spans[o - 1].problem, way_spans[o].problem,
                 (long long)way_spans[o].lo);

    const Buffer bufs[] = {
        {"d_cspace", d_cspace, cspace_bytes, false},
        {"d_thin", d_thin, d_thin ? thin_bytes : 0, false},
        {"d_closest", d_closest, d_closest ? 4 * closest_ints : 0, false},
        {"d_upstream", d_upstream, 4 * (int64_t)n_upstream, false},
        {"d_problems", d_problems, (int64_t)sizeof(simq_action_waypoint_problem) * n, true},
        {"d_ways", d_ways, 8 * way_pairs, true},
        {"d_counts", d_counts, 4 * (int64_t)n, true},
        {"d_endpoints", d_endpoints, 16 * (int64_t)n, true},
        {"d_status", d_status, 4 * (int64_t)n, true},
    };
    const int align[] = {1, 1, 4, 4, 8, 8, 4, 4, 4};
    const int nb = (int)(sizeof(bufs) / sizeof(bufs[0]));
    for (int a = 0; a < nb; ++a)
        SIMQ_REQUIRE((uintptr_t)bufs[a].p % align[a] == 0, "action_waypoints: %s is not %d-byte aligned", bufs[a].name, align[a]);
    int a = 0, b = 0;
    SIMQ_REQUIRE(!first_conflict(bufs, nb, &a, &b), "action_waypoints: %s and %s overlap", bufs[a].name, bufs[b].name);
    lds = (lds + 15) & ~(int64_t)15;
    SIMQ_REQUIRE(lds <= kLdsBudget, "action_waypoints: %lld bytes of LDS over the %d of a compute unit", (long long)lds, kLdsBudget);

    hipStream_t s = static_cast<hipStream_t>(stream);
    SIMQ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(action_waypoints_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
    const HostBlock block = {problems, sizeof(simq_action_waypoint_problem) * (size_t)n};
    SIMQ_CHECK_HIP(upload_descriptors(d_problems, &block, 1, nullptr, s));
    const Extents ext = {cspace_bytes, d_thin ? thin_bytes : 0, d_closest ? closest_ints : 0, way_pairs, n_upstream};
    action_waypoints_kernel<<<n, kLanes, (size_t)lds, s>>>(d_cspace, d_thin, d_closest, d_problems, reinterpret_cast<int2*>(d_ways), d_counts,
                                                           d_endpoints, d_upstream, d_status, ext, (unsigned)lds);
    SIMQ_CHECK_LAUNCH();
    note_launch("action_waypoints");
    return 0;
}
