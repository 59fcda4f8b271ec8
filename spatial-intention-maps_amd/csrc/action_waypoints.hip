// libsimq: from a robot's pixel pair to its waypoint pixels in one launch -- OccupancyMap.shortest_path between the two conversions
//   action_waypoints_kernel  straight-line test, snap, GridGraph._spfa, the walk, approximate_polygon decided in integers, the pruning
//                            envs.py:2483-2490, shortest_paths.pyx:69-154
//
// The search is grid_paths_kernel's (grid_waypoints.hip) and the simplification grid_waypoints_kernel's (grid_simplify.hip), restated
// here so that the two stay as they are: the rules are those of include/simq.h and the comments there say what is parallel.  What is
// this kernel's own:
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
#include "../../include/simq.h"

#include <algorithm>
#include <vector>

namespace simq {

namespace {

constexpr int kLanes = 64;
constexpr float kSqrt2 = 1.41421353816986083984375f;   // float32(np.sqrt(2)), shortest_paths.pyx:31
constexpr int kNoParent = 0xFF;
constexpr int kLdsBudget = 160 * 1024;
constexpr unsigned kFree = 1u, kQueued = 2u, kOne = 4u;
static_assert(SIMQ_GRID_WAYPOINTS_MAX_PATH >= SIMQ_GRID_PATH_MAX_BOX_CELLS, "a path has at most as many points as its window has cells");
static_assert(SIMQ_GRID_PATH_MAX_BOX_CELLS / 3 < (1 << 15), "window coordinates fit 16 bits and keep the rule's products in range");

// direction k of shortest_paths.pyx:30
__device__ __forceinline__ int dir_di(int k) { return k < 2 ? 0 : (k < 5 ? -1 : 1); }
__device__ __forceinline__ int dir_dj(int k) { return k < 2 ? 2 * k - 1 : (k - 2) % 3 - 1; }
__device__ __forceinline__ float dir_w(int k) { return (0xB4 >> k) & 1 ? kSqrt2 : 1.f; }   // diagonals: 2, 4, 5, 7

// distances | ring | parents | flags, as grid_paths_kernel lays them out; the path and the kept mask reuse the first two
__host__ __device__ inline int64_t lds_bytes(int box_rows, int box_cols) {
    const int64_t n = (int64_t)(box_rows + 2) * (box_cols + 2);
    const int64_t q = (int64_t)box_rows * box_cols + 1;
    return 4 * n + 2 * ((q + 1) & ~(int64_t)1) + 2 * n;
}

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
        const int dr = abs(ti - si), dc = abs(tj - sj);
        const int sr = ti > si ? 1 : -1, sc = tj > sj ? 1 : -1;
        const int nn = max(dr, dc), mm = min(dr, dc);
        bool hit = false;
        for (int i = lane; i <= nn; i += kLanes) {
            const int minor = nn > 0 ? (2 * mm * i + nn) / (2 * nn) : 0;
            const int r = dr > dc ? si + sr * i : si + sr * minor;
            const int c = dr > dc ? sj + sc * minor : sj + sc * i;
            hit |= thin[r * C + c] != 1;
        }
        if (!__any(hit)) {
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
        const int a = cl[si * C + sj], b = cl[n_cells + si * C + sj], c = cl[ti * C + tj], d = cl[n_cells + ti * C + tj];
        if (a < 0 || a >= R || b < 0 || b >= C || c < 0 || c >= R || d < 0 || d >= C) {
            if (lane == 0) status[blockIdx.x] = 2;
            return;
        }
        si = a; sj = b; ti = c; tj = d;
    }

    // ---- every free cell must lie inside the declared window: one pass over the grid, 16 bytes at a time where aligned
    const int bi0 = p.box_i0, bj0 = p.box_j0, bh = p.box_rows, bw = p.box_cols;
    {
        bool outside = false;
        const int lead = min(n_cells, (int)((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15));
        const int chunks = (n_cells - lead) / 16;
        auto check = [&](int idx, int count) {
            int r = idx / C, c = idx - r * C;
            for (int t = 0; t < count; ++t) {
                if (g[idx + t] != 0 && (r < bi0 || r >= bi0 + bh || c < bj0 || c >= bj0 + bw)) outside = true;
                if (++c == C) { c = 0; ++r; }
            }
        };
        if (lane == 0 && lead > 0) check(0, lead);
        if (lane == 1 && lead + 16 * chunks < n_cells) check(lead + 16 * chunks, n_cells - lead - 16 * chunks);
        const uint4* g16 = reinterpret_cast<const uint4*>(g + lead);
        for (int q = lane; q < chunks; q += kLanes) {
            const uint4 w = g16[q];
            if ((w.x | w.y | w.z | w.w) != 0u) check(lead + 16 * q, 16);
        }
        if (__any(outside)) {
            if (lane == 0) status[blockIdx.x] = 2;
            return;
        }
    }

    // ---- LDS state over the window + halo
    const int W = bw + 2, N = (bh + 2) * W;
    float* dist = reinterpret_cast<float*>(smem);
    uint16_t* ring = reinterpret_cast<uint16_t*>(smem + 4 * (int64_t)N);
    uint8_t* par = reinterpret_cast<uint8_t*>(smem + 4 * (int64_t)N + 2 * ((bh * bw + 2) & ~1));
    uint8_t* flg = par + N;
    const float inf = 2.f * (float)n_cells;              // self.inf = 2 * max_num_verts (exact: < 2^24)
    int vertices = 0;
    for (int l = lane; l < N; l += kLanes) {
        const int li = l / W, lj = l - li * W;
        const bool inner = li >= 1 && li <= bh && lj >= 1 && lj <= bw;
        const unsigned cell = inner ? g[(bi0 + li - 1) * C + (bj0 + lj - 1)] : 0u;
        dist[l] = inf;
        par[l] = kNoParent;
        flg[l] = (uint8_t)((cell != 0u ? kFree : 0u) | (cell == 1u ? kOne : 0u));
        vertices += cell != 0u ? 1 : 0;
    }
    for (int o = kLanes / 2; o >= 1; o >>= 1) vertices += __shfl_xor(vertices, o, kLanes);
    const int Q = vertices + 1;                          // ring slots: at most every vertex is queued at once
    __syncthreads();
    const bool src_in = si >= bi0 && si < bi0 + bh && sj >= bj0 && sj < bj0 + bw;
    const bool tgt_in = ti >= bi0 && ti < bi0 + bh && tj >= bj0 && tj < bj0 + bw;
    const int s_l = src_in ? (si - bi0 + 1) * W + (sj - bj0 + 1) : -1;
    const bool search = src_in && (flg[s_l] & kFree) != 0;   // edges leave a free cell only: a blocked source relaxes nothing
    int st = 0;

    if (search) {
        const int k = lane & 7;
        const int my_off = dir_di(k) * W + dir_dj(k);
        const float my_w = dir_w(k);
        int head = 0, tail = 1;
        int hp = 1 % Q, tp = 1 % Q;                      // ring positions of slot head + 1 (the front) and of slot tail
        int f = s_l;                                     // the front vertex (slot head + 1), -1 when nothing is queued
        float df = 0.f;                                  // ... and its distance as it stands
        if (lane == 0) { dist[s_l] = 0.f; ring[hp] = (uint16_t)s_l; flg[s_l] |= kQueued; }
        const int64_t pop_cap = 64 * (int64_t)(Q - 1) + 64;
        int64_t pops = 0;
        __syncthreads();
        while (head < tail) {
            if (++pops > pop_cap) { st = 4; break; }
            ++head;
            const int u = f;
            const float du = df;
            const unsigned fu = flg[u];
            hp = hp + 1 == Q ? 0 : hp + 1;
            int nf = -1;
            float ndf = 0.f;
            if (head < tail) { nf = ring[hp]; ndf = dist[nf]; }
            const int v = u + my_off;
            const float dv = dist[v];
            const unsigned fv = flg[v];
            const float nw = du + my_w;
            const bool acc = (fv & kFree) && nw < dv;
            const unsigned accepted = (unsigned)__ballot(acc) & 0xFFu;
            const unsigned pushing = (unsigned)__ballot(acc && !(fv & kQueued)) & 0xFFu;
            if (lane < 8 && acc) {
                dist[v] = nw;
                par[v] = (uint8_t)k;
                if (!(fv & kQueued)) flg[v] = (uint8_t)(fv | kQueued);
            }
            if (lane == 0) flg[u] = (uint8_t)(fu & ~kQueued);     // in_queue[u] = 0
            f = nf;
            df = ndf;
            for (unsigned m = accepted; m != 0u; m &= m - 1u) {
                const int kk = __ffs(m) - 1;
                const int vk = u + dir_di(kk) * W + dir_dj(kk);
                const float nk = du + dir_w(kk);
                if (vk == f) df = nk;                    // the front is a neighbour of u: later pushes of this pop see it lowered
                if ((pushing >> kk) & 1u) {
                    ++tail;
                    tp = tp + 1 == Q ? 0 : tp + 1;
                    if (head + 1 == tail) {              // the only one queued: both sides of the comparison are this slot
                        if (lane == 0) ring[tp] = (uint16_t)vk;
                        f = vk;
                        df = nk;
                    } else if (nk < df) {
                        if (lane == 0) { ring[tp] = (uint16_t)f; ring[hp] = (uint16_t)vk; }
                        f = vk;
                        df = nk;
                    } else if (lane == 0) {
                        ring[tp] = (uint16_t)vk;
                    }
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (st != 0) {
        if (lane == 0) status[blockIdx.x] = st;
        return;
    }
    int2* way = ways + p.way_offset;
    int32_t* e = endpoints + 4 * (int64_t)blockIdx.x;

    // ---- a path of the target alone (an unreachable or blocked target, a blocked source, target == source, either outside the window)
    if (!search || !tgt_in) {
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
    uint32_t* keep = reinterpret_cast<uint32_t*>(smem + 4 * (int64_t)N);
    int n = 0;
    if (lane == 0) {
        int i = ti - bi0 + 1, j = tj - bj0 + 1;
        int v = i * W + j;
        path[0] = make_ushort2((unsigned short)i, (unsigned short)j);
        n = 1;
        while (v != s_l && n < N) {
            const int pk = par[v];
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
    const int words = (n + 31) >> 5;
    for (int w = lane; w < words; w += kLanes) keep[w] = 0u;
    __syncthreads();
    if (lane == 0) {
        keep[0] |= 1u;
        keep[(n - 1) >> 5] |= 1u << ((n - 1) & 31);
    }
    __syncthreads();

    // ---- simplify (tolerance 1): s is kept and everything before it is resolved
    int s = 0;
    for (int verdicts = 0; s < n - 1; ++verdicts) {
        const int en = next_kept(keep, s, words, lane);
        if (verdicts > 2 * n || en < 0) { st = 4; break; }
        if (en == s + 1) { s = en; continue; }
        const ushort2 a = path[s], b = path[en];
        const int dr = (int)b.x - (int)a.x, dc = (int)b.y - (int)a.y;
        const uint32_t L = (uint32_t)(dr * dr + dc * dc);
        const uint32_t Lm = L != 0u ? L : 1u;
        unsigned long long best = 0ull;
        int best_k = n;
        for (int k = s + 1 + lane; k < en; k += kLanes) {
            const ushort2 q = path[k];
            const int r0 = (int)q.x - (int)a.x, c0 = (int)q.y - (int)a.y, r1 = (int)q.x - (int)b.x, c1 = (int)q.y - (int)b.y;
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
        if (best > (unsigned long long)Lm) {
            if (lane == 0) keep[best_k >> 5] |= 1u << (best_k & 31);
            __syncthreads();
        } else {
            s = en;
        }
    }

    // ---- prune: `last` is path[-1] of the reference, k the kept point in question, nxt its successor
    if (st == 0) {
        int last = 0;
        int k = next_kept(keep, 0, words, lane);
        for (int lines = 0; k >= 0 && k < n - 1; ++lines) {
            const int nxt = next_kept(keep, k, words, lane);
            if (lines > n || nxt < 0) { st = 4; break; }
            const ushort2 a = path[last], b = path[nxt];
            const int ar = a.x, ac = a.y, br = b.x, bc = b.y;
            const int dr = abs(br - ar), dc = abs(bc - ac);
            const int sr = br > ar ? 1 : -1, sc = bc > ac ? 1 : -1;
            const int nn = max(dr, dc), mm = min(dr, dc);
            bool hit = false;
            for (int i = lane; i <= nn; i += kLanes) {
                const int minor = nn > 0 ? (int)((2u * (unsigned)mm * (unsigned)i + (unsigned)nn) / (2u * (unsigned)nn)) : 0;
                const int r = dr > dc ? ar + sr * i : ar + sr * minor;
                const int c = dr > dc ? ac + sc * minor : ac + sc * i;
                hit |= (flg[r * W + c] & kOne) == 0u;
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

    // ---- the kept points, last first, as pixels of the grid
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
            if (at < p.way_capacity) {
                const ushort2 q = path[(w << 5) + __ffs((int)v) - 1];
                way[at] = make_int2((int)q.x - 1 + bi0, (int)q.y - 1 + bj0);
            }
        }
        before += __shfl(upto, kLanes - 1, kLanes);
    }
    if (lane == 0) {
        counts[blockIdx.x] = total;
        e[0] = si; e[1] = sj; e[2] = ti; e[3] = tj;
        status[blockIdx.x] = total > p.way_capacity ? 3 : 0;
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
