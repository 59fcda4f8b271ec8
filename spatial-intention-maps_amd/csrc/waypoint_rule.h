// From a dense path to its waypoints, which grid_simplify.hip (grid_waypoints_kernel: a path of int32 grid pixels in global memory)
// and action_waypoints.hip (action_waypoints_kernel: a path of 16-bit window pairs in LDS, or in its workspace) share: skimage.measure.approximate_polygon
// decided in integers, then the pruning of the back half of GridGraph.shortest_path (shortest_paths.pyx:139-154).  The rule is stated
// in include/simq.h; this header holds it once, over three functors, and nothing of an entry point:
//   point(k) -> int2             point k of the path, 0 <= k < n, both coordinates in [0, 2^15)
//   not_one(r, c) -> bool        the cell (r, c), in the coordinates of the points, is not 1: a line of the pruning may not cross it
//   emit(at, int2)               waypoint `at` of the output, source first, is this point
//
// One problem per wavefront; what is parallel inside a problem and what is not:
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
//     over the lanes and one __any (grid_spfa::line_hits).
//   * the output is reversed, so a point's place follows from its rank among the flags: population counts, a scan over the lanes.
#pragma once
#include "grid_spfa.h"

namespace simq {

namespace waypoint_rule {

using grid_spfa::kLanes;

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

// the waypoints of the n >= 1 points of a path: simplified at tolerance sqrt(t2), pruned, and the kept points given to `emit` last
// first, those at or past `capacity` left out.  `keep` is (n + 31) / 32 words of LDS, or of global memory the workgroup alone uses
// (action_waypoints_kernel<InHbm>): every store to it is followed by __syncthreads() before a load.  Returns 0, or 4 when a loop
// bound was passed (cannot happen; nothing is emitted then); *total is the number of waypoints, whatever the capacity.  All of it
// wave-uniform.
template <typename Point, typename NotOne, typename Emit>
__device__ __forceinline__ int waypoints(uint32_t* keep, int n, unsigned long long t2, int capacity, Point point, NotOne not_one,
                                         Emit emit, int lane, int* total_out) {
    const int words = (n + 31) >> 5;
    for (int w = lane; w < words; w += kLanes) keep[w] = 0u;
    __syncthreads();
    if (lane == 0) {
        keep[0] |= 1u;
        keep[(n - 1) >> 5] |= 1u << ((n - 1) & 31);
    }
    __syncthreads();

    // ---- simplify: s is kept and everything before it is resolved
    int s = 0;
    for (int verdicts = 0; s < n - 1; ++verdicts) {
        const int e = next_kept(keep, s, words, lane);
        if (verdicts > 2 * n || e < 0) return 4;
        if (e == s + 1) { s = e; continue; }
        const int2 a = point(s), b = point(e);
        const int dr = b.x - a.x, dc = b.y - a.y;
        const uint32_t L = (uint32_t)(dr * dr + dc * dc);
        const uint32_t Lm = L != 0u ? L : 1u;
        unsigned long long best = 0ull;
        int best_k = n;
        for (int k = s + 1 + lane; k < e; k += kLanes) {
            const int2 q = point(k);
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
    {
        int last = 0;
        int k = next_kept(keep, 0, words, lane);
        for (int lines = 0; k >= 0 && k < n - 1; ++lines) {
            const int nxt = next_kept(keep, k, words, lane);
            if (lines > n || nxt < 0) return 4;
            const int2 a = point(last), b = point(nxt);
            if (grid_spfa::line_hits(not_one, a.x, a.y, b.x, b.y, lane)) {
                last = k;
            } else {
                if (lane == 0) keep[k >> 5] &= ~(1u << (k & 31));
                __syncthreads();
            }
            k = nxt;
        }
    }

    // ---- the kept points, last first
    int total = 0;
    for (int w = lane; w < words; w += kLanes) total += __popc(keep[w]);
    for (int o = kLanes / 2; o >= 1; o >>= 1) total += __shfl_xor(total, o, kLanes);
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
            if (at < capacity) emit(at, point((w << 5) + __ffs((int)v) - 1));
        }
        before += __shfl(upto, kLanes - 1, kLanes);
    }
    *total_out = total;
    return 0;
}

}  // namespace waypoint_rule

}  // namespace simq
