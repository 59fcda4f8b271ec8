// libsimq: waypoints from dense paths -- skimage.measure.approximate_polygon decided in integers, then the pruning of
//   grid_waypoints_kernel    the back half of GridGraph.shortest_path                                     shortest_paths.pyx:139-154
//
// The rule is stated in include/simq.h.  One problem per wavefront; what is parallel inside a problem and what is not:
//   * a segment's interior is strided over the lanes.  Every point's squared distance is put over the segment's one denominator
//     L = dr^2 + dc^2 (cross^2 for a perpendicular distance, e^2 * L for an end-point distance; L = 1 when the two ends coincide and
//     no distance is perpendicular), so comparing two of them, or one with t^2 * L, is the cross-multiplication of the rule with no
//     division: all below 2^62.  The products have 32-bit factors (one v_mad_u64_u32 each, no full 64-bit multiply).  Each lane keeps
//     its first maximum, a butterfly of (value, index) gives the wave's: larger value, then smaller index.
//   * the order of segments is sequential but needs no stack: the kept flags are a bit mask in LDS, `s` is a kept point with
//     everything before it resolved, `e` the next kept point.  (s, e) either splits -- a new flag between them, at most n - 2 times --
//     or it does not and s moves to e, at most n - 1 times.  A verdict depends on its end points only, so this is the reference's
//     result.  The next kept point is found 64 mask words (2 048 points) per ballot.
//   * pruning walks the kept points in order, clears the flag of a dropped one, and tests one line at a time with its cells strided
//     over the lanes and one __any.
//   * the output is reversed, so a point's place follows from its rank among the flags: population counts, a scan over the lanes.
#include "batch_abi.h"
#include "../../include/simq.h"

#include <vector>

namespace simq {

namespace {

constexpr int kLanes = 64;
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

// the first flag above `after`, -1 when there is none (wave-uniform; `keep` holds `words` words)
__device__ __forceinline__ int next_kept(const uint32_t* keep, int after, int words, int lane) {
    const int first = after + 1, w0 = first >> 5;
    for (int base = w0; base < words; base += kLanes) {
        const int w = base + lane;
        uint32_t v = w < words ? keep[w] : 0u;
        if (w == w0) v &= ~0u << (first & 31);
        const unsigned long long found = __ballot(v != 0u);
        if (found != 0ull) {
            const int l = __ffsll(found) - 1;
            const uint32_t bits = (uint32_t)__shfl((int)v, l, kLanes);
            return ((base + l) << 5) + __ffs((int)bits) - 1;
        }
    }
    return -1;
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
    const int words = (n + 31) >> 5;

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
    for (int w = lane; w < words; w += kLanes) keep[w] = 0u;
    __syncthreads();
    if (lane == 0) {
        keep[0] |= 1u;
        keep[(n - 1) >> 5] |= 1u << ((n - 1) & 31);
    }
    __syncthreads();

    // ---- simplify: s is kept and everything before it is resolved
    int st = 0;
    const unsigned long long t2 = (unsigned long long)(p.tolerance * p.tolerance);
    int s = 0;
    for (int verdicts = 0; s < n - 1; ++verdicts) {
        const int e = next_kept(keep, s, words, lane);
        if (verdicts > 2 * n || e < 0) { st = 4; break; }
        if (e == s + 1) { s = e; continue; }
        const int2 a = path[s], b = path[e];
        const int dr = b.x - a.x, dc = b.y - a.y;
        const uint32_t L = (uint32_t)(dr * dr + dc * dc);
        const uint32_t Lm = L != 0u ? L : 1u;
        unsigned long long best = 0ull;
        int best_k = n;
        for (int k = s + 1 + lane; k < e; k += kLanes) {
            const int2 q = path[k];
            const int r0 = q.x - a.x, c0 = q.y - a.y, r1 = q.x - b.x, c1 = q.y - b.y;
            const int a0 = r0 * dr + c0 * dc, a1 = -r1 * dr - c1 * dc;
            unsigned long long v;
            if (a0 > 0 && a1 > 0) {
                const int cross = r0 * dc - c0 * dr;
                const uint32_t m = (uint32_t)abs(cross);
                v = (unsigned long long)m * m;
            } else {
                const uint32_t e0 = (uint32_t)(r0 * r0 + c0 * c0), e1 = (uint32_t)(r1 * r1 + c1 * c1);
                v = (unsigned long long)min(e0, e1) * Lm;
            }
            if (best_k == n || v > best) { best = v; best_k = k; }
        }
        for (int o = kLanes / 2; o >= 1; o >>= 1) {
            const unsigned long long ov = __shfl_xor(best, o, kLanes);
            const int ok = __shfl_xor(best_k, o, kLanes);
            if (ok < n && (best_k == n || ov > best || (ov == best && ok < best_k))) { best = ov; best_k = ok; }
        }
        if (best > t2 * Lm) {
            if (lane == 0) keep[best_k >> 5] |= 1u << (best_k & 31);
            __syncthreads();
        } else {
            s = e;
        }
    }

    // ---- prune: `last` is path[-1] of the reference, k the kept point in question, nxt its successor
    if (st == 0) {
        int last = 0;
        int k = next_kept(keep, 0, words, lane);
        for (int lines = 0; k >= 0 && k < n - 1; ++lines) {
            const int nxt = next_kept(keep, k, words, lane);
            if (lines > n || nxt < 0) { st = 4; break; }
            const int2 a = path[last], b = path[nxt];
            const int dr = abs(b.x - a.x), dc = abs(b.y - a.y);
            const int sr = b.x > a.x ? 1 : -1, sc = b.y > a.y ? 1 : -1;
            const int nn = max(dr, dc), mm = min(dr, dc);
            bool hit = false;
            for (int i = lane; i <= nn; i += kLanes) {
                const int minor = nn > 0 ? (int)((2u * (unsigned)mm * (unsigned)i + (unsigned)nn) / (2u * (unsigned)nn)) : 0;
                const int r = dr > dc ? a.x + sr * i : a.x + sr * minor;
                const int c = dr > dc ? a.y + sc * minor : a.y + sc * i;
                hit |= g[r * C + c] != 1;
            }
            if (__any(hit)) {
                last = k;
            } else {
                if (lane == 0) keep[k >> 5] &= ~(1u << (k & 31));
                __syncthreads();
            }
            k = nxt;
        }
    }
    if (st != 0) {
        if (lane == 0) status[blockIdx.x] = st;
        return;
    }

    // ---- the kept points, last first
    int total = 0;
    for (int w = lane; w < words; w += kLanes) total += __popc(keep[w]);
    for (int o = kLanes / 2; o >= 1; o >>= 1) total += __shfl_xor(total, o, kLanes);
    int2* way = ways + p.way_offset;
    int before = 0;                                     // flags in the words below `base`
    for (int base = 0; base < words; base += kLanes) {
        const int w = base + lane;
        uint32_t v = w < words ? keep[w] : 0u;
        const int mine = __popc(v);
        int upto = mine;                                // ... and in this chunk up to and including this lane's word
        for (int o = 1; o < kLanes; o <<= 1) {
            const int below = __shfl_up(upto, o, kLanes);
            if (lane >= o) upto += below;
        }
        int rank = before + upto - mine;
        for (; v != 0u; v &= v - 1u, ++rank) {
            const int at = total - 1 - rank;
            if (at < p.way_capacity) way[at] = path[(w << 5) + __ffs((int)v) - 1];
        }
        before += __shfl(upto, kLanes - 1, kLanes);
    }
    if (lane == 0) {
        counts[blockIdx.x] = total;
        status[blockIdx.x] = total > p.way_capacity ? 3 : 0;
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
