// libsimq: batched shortest-path waypoints on 8-connected grids -- SPFA's parents and the dense path, bit for bit
//   grid_paths_kernel        GridGraph._spfa + the walk of GridGraph.shortest_path               shortest_paths.pyx:69-114, 126-137
//                            (+ the front half of OccupancyMap.shortest_path: straight-line test, closest free cells   envs.py:2477-2490)
//
// Exactness.  SPFA's distances are a fixed point that any update order reaches (grid_paths.hip); its parents are not: where two paths
// tie, the parent is the vertex whose relaxation was accepted last, and that follows the order of the queue, including the exchange
// of the newest entry with the front.  So the search itself is emulated, one problem per wavefront, with the problems as the
// parallel axis.  The rules are stated in include/simq.h; what is parallel inside one pop and what is not:
//   * the eight relaxations of a pop read d[u] (fixed during the pop: u is not its own neighbour) and eight distinct cells, so lanes
//     0 .. 7 take one edge each: load the neighbour, form fl32(d[u] + w), compare, store distance and parent.  Two ballots give the
//     accepted edges and those that push.
//   * the queue is sequential.  A uniform loop walks the accepted edges in the reference's order; it keeps the front vertex and the
//     front's distance in registers, lowers that distance at the edge that relaxes the front, and decides each push's exchange against
//     the value as it stands at that edge -- an exchange decided against the front's distance before or after the whole pop is
//     sometimes the other way round.
// State per cell of the caller's window plus a blocked one-cell halo (so no edge needs a bounds test), in LDS: fp32 distance, a
// 16-bit ring entry, the parent as a direction byte, a flag byte (bit 0 free, bit 1 queued).  The ring is laid out for window cells + 1
// entries and uses free cells + 1 of them: at most every vertex is queued at once, and slot numbers only ever grow, so positions wrap
// (a cluttered grid pushes 1 - 7 % more often than it has vertices).
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

// direction k of shortest_paths.pyx:30
__device__ __forceinline__ int dir_di(int k) { return k < 2 ? 0 : (k < 5 ? -1 : 1); }
__device__ __forceinline__ int dir_dj(int k) { return k < 2 ? 2 * k - 1 : (k - 2) % 3 - 1; }
__device__ __forceinline__ float dir_w(int k) { return (0xB4 >> k) & 1 ? kSqrt2 : 1.f; }   // diagonals: 2, 4, 5, 7

__host__ __device__ inline int64_t lds_bytes(int box_rows, int box_cols) {
    const int64_t n = (int64_t)(box_rows + 2) * (box_cols + 2);
    const int64_t q = (int64_t)box_rows * box_cols + 1;
    return 4 * n + 2 * ((q + 1) & ~(int64_t)1) + 2 * n;
}

__device__ __forceinline__ bool descriptor_ok(const simq_grid_path_problem& p, const int32_t* closest, const int32_t* parents,
                                              const float* dist) {
    if (p.rows < 1 || p.cols < 1 || (int64_t)p.rows * p.cols >= SIMQ_GRID_MAX_CELLS) return false;
    if (p.src_i < 0 || p.src_i >= p.rows || p.src_j < 0 || p.src_j >= p.cols) return false;
    if (p.tgt_i < 0 || p.tgt_i >= p.rows || p.tgt_j < 0 || p.tgt_j >= p.cols) return false;
    if (p.grid_offset < 0 || p.path_offset < 0 || p.path_capacity < 1) return false;
    if (p.box_rows < 0 || p.box_cols < 0 || p.box_i0 < 0 || p.box_j0 < 0 || p.box_i0 > p.rows - p.box_rows ||
        p.box_j0 > p.cols - p.box_cols)
        return false;
    if ((int64_t)(p.box_rows + 2) * (p.box_cols + 2) > SIMQ_GRID_PATH_MAX_BOX_CELLS) return false;
    if ((p.closest_offset >= 0 && !closest) || (p.parents_offset >= 0 && !parents) || (p.dist_offset >= 0 && !dist)) return false;
    return true;
}

__global__ void __launch_bounds__(kLanes) grid_paths_kernel(const uint8_t* __restrict__ grids, const int32_t* __restrict__ closest,
                                                            const simq_grid_path_problem* __restrict__ probs, int32_t* __restrict__ paths,
                                                            int32_t* __restrict__ lengths, int32_t* __restrict__ endpoints,
                                                            int32_t* __restrict__ parents_out, float* __restrict__ dist_out,
                                                            int32_t* __restrict__ status, unsigned lds_have) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const simq_grid_path_problem p = probs[blockIdx.x];
    const int lane = threadIdx.x;
    if (!descriptor_ok(p, closest, parents_out, dist_out) || lds_bytes(p.box_rows, p.box_cols) > (int64_t)lds_have) {
        if (lane == 0) status[blockIdx.x] = 2;          // (the host validated already: nothing is read or written)
        return;
    }
    const int R = p.rows, C = p.cols, n = R * C;
    const uint8_t* g = grids + p.grid_offset;
    int si = p.src_i, sj = p.src_j, ti = p.tgt_i, tj = p.tgt_j;

    // ---- OccupancyMap.shortest_path's straight-line test, on the pixels as given (envs.py:2483-2485)
    if (p.thin_offset >= 0) {
        const uint8_t* thin = grids + p.thin_offset;
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
                lengths[blockIdx.x] = 0;
                int32_t* e = endpoints + 4 * (int64_t)blockIdx.x;
                e[0] = si; e[1] = sj; e[2] = ti; e[3] = tj;
            }
            return;
        }
    }
    // ---- OccupancyMap._closest_valid_cspace_indices (envs.py:2488-2489, 2522-2523)
    if (p.closest_offset >= 0) {
        const int32_t* cl = closest + p.closest_offset;
        const int a = cl[si * C + sj], b = cl[n + si * C + sj], c = cl[ti * C + tj], d = cl[n + ti * C + tj];
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
        const int lead = min(n, (int)((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15));
        const int chunks = (n - lead) / 16;
        auto check = [&](int idx, int count) {
            int r = idx / C, c = idx - r * C;
            for (int t = 0; t < count; ++t) {
                if (g[idx + t] != 0 && (r < bi0 || r >= bi0 + bh || c < bj0 || c >= bj0 + bw)) outside = true;
                if (++c == C) { c = 0; ++r; }
            }
        };
        if (lane == 0 && lead > 0) check(0, lead);
        if (lane == 1 && lead + 16 * chunks < n) check(lead + 16 * chunks, n - lead - 16 * chunks);
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
    const float inf = 2.f * (float)n;                    // self.inf = 2 * max_num_verts (exact: < 2^24)
    int vertices = 0;
    for (int l = lane; l < N; l += kLanes) {
        const int li = l / W, lj = l - li * W;
        const bool inner = li >= 1 && li <= bh && lj >= 1 && lj <= bw;
        const bool is_free = inner && g[(bi0 + li - 1) * C + (bj0 + lj - 1)] != 0;
        dist[l] = inf;
        par[l] = kNoParent;
        flg[l] = is_free ? 1 : 0;
        vertices += is_free ? 1 : 0;
    }
    for (int o = kLanes / 2; o >= 1; o >>= 1) vertices += __shfl_xor(vertices, o, kLanes);
    const int Q = vertices + 1;                          // ring slots: at most every vertex is queued at once
    __syncthreads();
    const bool src_in = si >= bi0 && si < bi0 + bh && sj >= bj0 && sj < bj0 + bw;
    const bool tgt_in = ti >= bi0 && ti < bi0 + bh && tj >= bj0 && tj < bj0 + bw;
    const int s_l = src_in ? (si - bi0 + 1) * W + (sj - bj0 + 1) : -1;
    const bool search = src_in && flg[s_l] != 0;         // edges leave a free cell only: a blocked source relaxes nothing
    int st = 0;
    if (src_in && lane == 0) dist[s_l] = 0.f;

    if (search) {
        const int k = lane & 7;
        const int my_off = dir_di(k) * W + dir_dj(k);
        const float my_w = dir_w(k);
        int head = 0, tail = 1;
        int hp = 1 % Q, tp = 1 % Q;                      // ring positions of slot head + 1 (the front) and of slot tail
        int f = s_l;                                     // the front vertex (slot head + 1), -1 when nothing is queued
        float df = 0.f;                                  // ... and its distance as it stands
        if (lane == 0) { ring[hp] = (uint16_t)s_l; flg[s_l] = 3; }
        const int64_t pop_cap = 64 * (int64_t)(Q - 1) + 64;
        int64_t pops = 0;
        __syncthreads();
        while (head < tail) {
            if (++pops > pop_cap) { st = 4; break; }
            ++head;
            const int u = f;
            const float du = df;
            hp = hp + 1 == Q ? 0 : hp + 1;
            int nf = -1;
            float ndf = 0.f;
            if (head < tail) { nf = ring[hp]; ndf = dist[nf]; }
            const int v = u + my_off;
            const float dv = dist[v];
            const unsigned fv = flg[v];
            const float nw = du + my_w;
            const bool acc = (fv & 1u) && nw < dv;
            const unsigned accepted = (unsigned)__ballot(acc) & 0xFFu;
            const unsigned pushing = (unsigned)__ballot(acc && !(fv & 2u)) & 0xFFu;
            if (lane < 8 && acc) {
                dist[v] = nw;
                par[v] = (uint8_t)k;
                if (!(fv & 2u)) flg[v] = 3;
            }
            if (lane == 0) flg[u] = 1;                   // in_queue[u] = 0
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

    // ---- the walk from the target (shortest_paths.pyx:126-137)
    if (lane == 0) {
        int32_t* path = paths + 2 * p.path_offset;
        int len = 1;
        path[0] = ti;
        path[1] = tj;
        if (search && tgt_in) {
            int i = ti, j = tj;
            int v = (ti - bi0 + 1) * W + (tj - bj0 + 1);
            while (v != s_l && len <= N) {
                const int pk = par[v];
                if (pk == kNoParent) break;
                i -= dir_di(pk);
                j -= dir_dj(pk);
                v -= dir_di(pk) * W + dir_dj(pk);
                if (len < p.path_capacity) { path[2 * len] = i; path[2 * len + 1] = j; }
                ++len;
            }
        }
        lengths[blockIdx.x] = len;
        int32_t* e = endpoints + 4 * (int64_t)blockIdx.x;
        e[0] = si; e[1] = sj; e[2] = ti; e[3] = tj;
        if (st == 0 && len > p.path_capacity) st = 3;
        status[blockIdx.x] = st;
    }

    // ---- the optional images over the full grid, from LDS
    if (p.parents_offset >= 0 || p.dist_offset >= 0) {
        int32_t* po = p.parents_offset >= 0 ? parents_out + p.parents_offset : nullptr;
        float* dout = p.dist_offset >= 0 ? dist_out + p.dist_offset : nullptr;
        for (int r = 0; r < R; ++r) {
            const bool row_in = r >= bi0 && r < bi0 + bh;
            for (int c = lane; c < C; c += kLanes) {
                int32_t pv = -1;
                float x = r == si && c == sj ? 0.f : -1.f;
                if (row_in && c >= bj0 && c < bj0 + bw) {
                    const int l = (r - bi0 + 1) * W + (c - bj0 + 1);
                    const int pk = par[l];
                    if (pk != kNoParent) pv = (r - dir_di(pk)) * C + (c - dir_dj(pk));
                    const float d = dist[l];
                    x = d == inf ? -1.f : d;
                }
                if (po) po[r * C + c] = pv;
                if (dout) dout[r * C + c] = x;
            }
        }
    }
}

int disjoint(std::vector<Span>& spans, const char* what) {
    const size_t i = first_overlap(spans);
    SIMQ_REQUIRE(i == 0, "grid_paths: problems %d and %d overlap in %s at element %lld", spans[i - 1].problem, spans[i].problem, what,
                 (long long)spans[i].lo);
    return 0;
}

}  // namespace

}  // namespace simq

using namespace simq;

extern "C" int simq_grid_paths(const uint8_t* d_grids, int64_t grids_bytes, const int32_t* d_closest, int64_t closest_ints,
                               const simq_grid_path_problem* problems, int n, simq_grid_path_problem* d_problems, int32_t* d_paths,
                               int64_t path_pairs, int32_t* d_lengths, int32_t* d_endpoints, int32_t* d_parents, int64_t parents_ints,
                               float* d_dist, int64_t dist_floats, int32_t* d_status, void* stream) {
    SIMQ_REQUIRE(d_grids && problems && d_problems && d_paths && d_lengths && d_endpoints && d_status, "grid_paths: NULL pointer");
    SIMQ_REQUIRE(n >= 1 && n <= (1 << 24), "grid_paths: n = %d (1 .. 2^24 problems)", n);
    std::vector<Span> path_spans, parent_spans, dist_spans;
    path_spans.reserve(n);
    int64_t lds = 0;
    for (int i = 0; i < n; ++i) {
        const simq_grid_path_problem& p = problems[i];
        SIMQ_REQUIRE(p.rows >= 1 && p.cols >= 1 && (int64_t)p.rows * p.cols < SIMQ_GRID_MAX_CELLS,
                     "grid_paths: problem %d is %d x %d (rows, cols >= 1, rows * cols < 2^22)", i, p.rows, p.cols);
        SIMQ_REQUIRE(p.src_i >= 0 && p.src_i < p.rows && p.src_j >= 0 && p.src_j < p.cols,
                     "grid_paths: problem %d: source (%d, %d) outside its %d x %d grid", i, p.src_i, p.src_j, p.rows, p.cols);
        SIMQ_REQUIRE(p.tgt_i >= 0 && p.tgt_i < p.rows && p.tgt_j >= 0 && p.tgt_j < p.cols,
                     "grid_paths: problem %d: target (%d, %d) outside its %d x %d grid", i, p.tgt_i, p.tgt_j, p.rows, p.cols);
        const int64_t cells = (int64_t)p.rows * p.cols;
        SIMQ_REQUIRE(fits(p.grid_offset, cells, grids_bytes),
                     "grid_paths: problem %d: grid_offset: bytes [%lld, %lld) outside the %lld of d_grids", i, (long long)p.grid_offset,
                     (long long)(p.grid_offset + cells), (long long)grids_bytes);
        SIMQ_REQUIRE(p.thin_offset == -1 || fits(p.thin_offset, cells, grids_bytes),
                     "grid_paths: problem %d: thin_offset: bytes [%lld, %lld) outside the %lld of d_grids (-1: no straight-line test)", i,
                     (long long)p.thin_offset, (long long)(p.thin_offset + cells), (long long)grids_bytes);
        SIMQ_REQUIRE(p.closest_offset == -1 || (d_closest && fits(p.closest_offset, 2 * cells, closest_ints)),
                     "grid_paths: problem %d: closest_offset: ints [%lld, %lld) outside the %lld of d_closest (-1: no snap)", i,
                     (long long)p.closest_offset, (long long)(p.closest_offset + 2 * cells), (long long)(d_closest ? closest_ints : 0));
        SIMQ_REQUIRE(p.box_rows >= 0 && p.box_cols >= 0 && p.box_i0 >= 0 && p.box_j0 >= 0 && p.box_i0 <= p.rows - p.box_rows &&
                         p.box_j0 <= p.cols - p.box_cols,
                     "grid_paths: problem %d: box rows [%d, %d + %d), columns [%d, %d + %d) outside its %d x %d grid", i, p.box_i0, p.box_i0,
                     p.box_rows, p.box_j0, p.box_j0, p.box_cols, p.rows, p.cols);
        SIMQ_REQUIRE((int64_t)(p.box_rows + 2) * (p.box_cols + 2) <= SIMQ_GRID_PATH_MAX_BOX_CELLS,
                     "grid_paths: problem %d: box of %d x %d cells plus its halo is %lld cells, over SIMQ_GRID_PATH_MAX_BOX_CELLS = %d "
                     "(the search state lives in LDS)", i, p.box_rows, p.box_cols, (long long)(p.box_rows + 2) * (p.box_cols + 2),
                     SIMQ_GRID_PATH_MAX_BOX_CELLS);
        SIMQ_REQUIRE(p.path_capacity >= 1, "grid_paths: problem %d: path_capacity = %d (>= 1 pair)", i, p.path_capacity);
        SIMQ_REQUIRE(fits(p.path_offset, p.path_capacity, path_pairs),
                     "grid_paths: problem %d: path_offset: pairs [%lld, %lld) outside the %lld of d_paths", i, (long long)p.path_offset,
                     (long long)(p.path_offset + p.path_capacity), (long long)path_pairs);
        path_spans.push_back({(uint64_t)p.path_offset, (uint64_t)(p.path_offset + p.path_capacity), i});
        SIMQ_REQUIRE(p.parents_offset == -1 || (d_parents && fits(p.parents_offset, cells, parents_ints)),
                     "grid_paths: problem %d: parents_offset: ints [%lld, %lld) outside the %lld of d_parents (-1: no parent image)", i,
                     (long long)p.parents_offset, (long long)(p.parents_offset + cells), (long long)(d_parents ? parents_ints : 0));
        if (p.parents_offset >= 0) parent_spans.push_back({(uint64_t)p.parents_offset, (uint64_t)(p.parents_offset + cells), i});
        SIMQ_REQUIRE(p.dist_offset == -1 || (d_dist && fits(p.dist_offset, cells, dist_floats)),
                     "grid_paths: problem %d: dist_offset: floats [%lld, %lld) outside the %lld of d_dist (-1: no distance image)", i,
                     (long long)p.dist_offset, (long long)(p.dist_offset + cells), (long long)(d_dist ? dist_floats : 0));
        if (p.dist_offset >= 0) dist_spans.push_back({(uint64_t)p.dist_offset, (uint64_t)(p.dist_offset + cells), i});
        lds = std::max(lds, lds_bytes(p.box_rows, p.box_cols));
    }
    if (disjoint(path_spans, "d_paths") || disjoint(parent_spans, "d_parents") || disjoint(dist_spans, "d_dist")) return -1;

    // alignment, and the buffers against each other: an output may share no byte with another buffer of the call.  This walk is
    // not batch_abi.h's first_conflict: it names the written buffer first, meets a buffer's alignment before its pairs and skips an
    // empty buffer, and which refusal comes first when several rules are broken is part of this entry point's behaviour.
    const Buffer bufs[] = {
        {"d_grids", d_grids, grids_bytes, false},
        {"d_closest", d_closest, d_closest ? 4 * closest_ints : 0, false},
        {"d_problems", d_problems, (int64_t)sizeof(simq_grid_path_problem) * n, true},
        {"d_paths", d_paths, 8 * path_pairs, true},
        {"d_lengths", d_lengths, 4 * (int64_t)n, true},
        {"d_endpoints", d_endpoints, 16 * (int64_t)n, true},
        {"d_parents", d_parents, d_parents ? 4 * parents_ints : 0, true},
        {"d_dist", d_dist, d_dist ? 4 * dist_floats : 0, true},
        {"d_status", d_status, 4 * (int64_t)n, true},
    };
    const int align[] = {1, 4, 8, 4, 4, 4, 4, 4, 4};
    const int nb = (int)(sizeof(bufs) / sizeof(bufs[0]));
    for (int a = 0; a < nb; ++a) {
        SIMQ_REQUIRE((uintptr_t)bufs[a].p % align[a] == 0, "grid_paths: %s is not %d-byte aligned", bufs[a].name, align[a]);
        for (int b = 0; b < nb; ++b) {
            if (a == b || !bufs[a].written || bufs[a].bytes <= 0 || bufs[b].bytes <= 0 || (bufs[b].written && b < a)) continue;
            SIMQ_REQUIRE(!overlaps(bufs[a].p, bufs[a].bytes, bufs[b].p, bufs[b].bytes), "grid_paths: %s and %s overlap", bufs[a].name,
                         bufs[b].name);
        }
    }
    lds = (lds + 15) & ~(int64_t)15;
    SIMQ_REQUIRE(lds <= kLdsBudget, "grid_paths: %lld bytes of LDS over the %d of a compute unit", (long long)lds, kLdsBudget);

    hipStream_t s = static_cast<hipStream_t>(stream);
    SIMQ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(grid_paths_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
    const HostBlock block = {problems, sizeof(simq_grid_path_problem) * (size_t)n};
    SIMQ_CHECK_HIP(upload_descriptors(d_problems, &block, 1, nullptr, s));
    grid_paths_kernel<<<n, kLanes, (size_t)lds, s>>>(d_grids, d_closest, d_problems, d_paths, d_lengths, d_endpoints, d_parents, d_dist,
                                                     d_status, (unsigned)lds);
    SIMQ_CHECK_LAUNCH();
    note_launch("grid_waypoints");
    return 0;
}
