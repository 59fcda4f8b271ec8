// The emulated SPFA over a window in LDS and the stages in front of it, which grid_waypoints.hip (grid_paths_kernel: the dense path
// and the optional images) and action_waypoints.hip (action_waypoints_kernel: pixels to waypoints in one launch) share:
// GridGraph._spfa (shortest_paths.pyx:69-114) and the front half of OccupancyMap.shortest_path (envs.py:2477-2490).  The rules are
// stated in include/simq.h; this header holds the search and nothing of an entry point.
//
// Exactness.  SPFA's distances are a fixed point that any update order reaches (grid_paths.hip); its parents are not: where two paths
// tie, the parent is the vertex whose relaxation was accepted last, and that follows the order of the queue, including the exchange
// of the newest entry with the front.  So the search itself is emulated, one problem per wavefront, with the problems as the
// parallel axis.  What is parallel inside one pop and what is not:
//   * the eight relaxations of a pop read d[u] (fixed during the pop: u is not its own neighbour) and eight distinct cells, so lanes
//     0 .. 7 take one edge each: load the neighbour, form fl32(d[u] + w), compare, store distance and parent.  Two ballots give the
//     accepted edges and those that push.
//   * the queue is sequential.  A uniform loop walks the accepted edges in the reference's order; it keeps the front vertex and the
//     front's distance in registers, lowers that distance at the edge that relaxes the front, and decides each push's exchange against
//     the value as it stands at that edge -- an exchange decided against the front's distance before or after the whole pop is
//     sometimes the other way round.
// State per cell of the caller's window plus a blocked one-cell halo (so no edge needs a bounds test), in LDS: fp32 distance, a
// 16-bit ring entry, the parent as a direction byte, a flag byte (kFree, kQueued and, for the kernel that asks for it, kOne).  The
// ring is laid out for window cells + 1 entries and uses free cells + 1 of them: at most every vertex is queued at once, and slot
// numbers only ever grow, so positions wrap (a cluttered grid pushes 1 - 7 % more often than it has vertices).
//
// The state's home.  init_window and search take the state as a type: the four arrays, the ring's entry type, W, N and index.  Lds is
// the carve-up above.  Hbm is the same carve-up over a caller's workspace in global memory with a 32-bit ring entry -- a window of a
// grid of SIMQ_GRID_MAX_CELLS cells plus its halo needs 23 bits -- for windows no LDS holds (grid_paths_kernel<InHbm>).  The rules do not
// know which one they run on; between the lanes of the one wavefront the barrier at the end of each pop orders the stores of that pop
// before the loads of the next in either memory.
//
// kKeepOne.  action_waypoints_kernel's pruning reads "the cell is 1" from the flag byte, so its search must carry that bit through
// every flag store: it reads the popped vertex's flags and writes them back without kQueued.  grid_paths_kernel has no such reader;
// with kKeepOne = false every flag store is a constant and the pop loop, the serial chain of that kernel, has no LDS access for it.
#pragma once
#include "common.h"

namespace simq {

namespace grid_spfa {

constexpr int kLanes = 64;
constexpr float kSqrt2 = 1.41421353816986083984375f;   // float32(np.sqrt(2)), shortest_paths.pyx:31
constexpr int kNoParent = 0xFF;
constexpr int kLdsBudget = 160 * 1024;
// the flag byte: the cell is != 0 (a vertex), it is in the queue, it is 1 (what a line of the pruning may cross; kKeepOne only)
constexpr unsigned kFree = 1u, kQueued = 2u, kOne = 4u;

// direction k of shortest_paths.pyx:30
__device__ __forceinline__ int dir_di(int k) { return k < 2 ? 0 : (k < 5 ? -1 : 1); }
__device__ __forceinline__ int dir_dj(int k) { return k < 2 ? 2 * k - 1 : (k - 2) % 3 - 1; }
__device__ __forceinline__ float dir_w(int k) { return (0xB4 >> k) & 1 ? kSqrt2 : 1.f; }   // diagonals: 2, 4, 5, 7

// distances | ring | parents | flags
__host__ __device__ inline int64_t lds_bytes(int box_rows, int box_cols) {
    const int64_t n = (int64_t)(box_rows + 2) * (box_cols + 2);
    const int64_t q = (int64_t)box_rows * box_cols + 1;
    return 4 * n + 2 * ((q + 1) & ~(int64_t)1) + 2 * n;
}

// the caller's window: rows [i0, i0 + rows), columns [j0, j0 + cols) of the grid
struct Window {
    int i0, j0, rows, cols;
    __device__ __forceinline__ bool holds(int i, int j) const { return i >= i0 && i < i0 + rows && j >= j0 && j < j0 + cols; }
};

// the carve-up of lds_bytes over the window + halo: W cells a row, N cells in all, the grid's cell (i, j) at index(b, i, j)
struct Lds {
    using Entry = uint16_t;
    float* dist;
    Entry* ring;
    uint8_t* par;
    uint8_t* flg;
    int W, N;
    __device__ __forceinline__ Lds(char* smem, const Window& b) : W(b.cols + 2), N((b.rows + 2) * (b.cols + 2)) {
        dist = reinterpret_cast<float*>(smem);
        ring = reinterpret_cast<Entry*>(smem + 4 * (int64_t)N);
        par = reinterpret_cast<uint8_t*>(smem + 4 * (int64_t)N + 2 * ((b.rows * b.cols + 2) & ~1));
        flg = par + N;
    }
    __device__ __forceinline__ int index(const Window& b, int i, int j) const { return (i - b.i0 + 1) * W + (j - b.j0 + 1); }
};

// distances | ring | parents | flags over a workspace in global memory: 10 bytes a cell, rounded up to 16
__host__ __device__ inline int64_t work_bytes(int box_rows, int box_cols) {
    const int64_t n = (int64_t)(box_rows + 2) * (box_cols + 2);
    const int64_t q = (int64_t)box_rows * box_cols + 1;
    return (4 * n + 4 * q + 2 * n + 15) & ~(int64_t)15;
}

// the carve-up of work_bytes at `work` (16-byte aligned): Lds's members and index, a 32-bit ring entry
struct Hbm {
    using Entry = uint32_t;
    float* dist;
    Entry* ring;
    uint8_t* par;
    uint8_t* flg;
    int W, N;
    __device__ __forceinline__ Hbm(char* work, const Window& b) : W(b.cols + 2), N((b.rows + 2) * (b.cols + 2)) {
        dist = reinterpret_cast<float*>(work);
        ring = reinterpret_cast<Entry*>(work + 4 * (int64_t)N);
        par = reinterpret_cast<uint8_t*>(work + 4 * (int64_t)N + 4 * ((int64_t)b.rows * b.cols + 1));
        flg = par + N;
    }
    __device__ __forceinline__ int index(const Window& b, int i, int j) const { return (i - b.i0 + 1) * W + (j - b.j0 + 1); }
};

// skimage.draw.line from (r0, c0) to (r1, c1) in closed form, its cells strided over the lanes: whether cell_is_not_one(r, c) holds
// for any of them (wave-uniform, one __any).  Step i of the longer side nn has moved round_half_up(mm * i / nn) along the shorter
// side mm.  The numerator is formed unsigned: the straight-line test has dr * dc < 2^22 cells, so 2 * mm * i + nn < 2^24; a line of
// the pruning has both sides <= 2^15, so it is < 2^32.  Neither reaches the sign bit, where the signed and the unsigned quotient would
// part, so this one spelling gives the cells of both.
template <typename NotOne>
__device__ __forceinline__ bool line_hits(NotOne cell_is_not_one, int r0, int c0, int r1, int c1, int lane) {
    const int dr = abs(r1 - r0), dc = abs(c1 - c0);
    const int sr = r1 > r0 ? 1 : -1, sc = c1 > c0 ? 1 : -1;
    const int nn = max(dr, dc), mm = min(dr, dc);
    bool hit = false;
    for (int i = lane; i <= nn; i += kLanes) {
        const int minor = nn > 0 ? (int)((2u * (unsigned)mm * (unsigned)i + (unsigned)nn) / (2u * (unsigned)nn)) : 0;
        const int r = dr > dc ? r0 + sr * i : r0 + sr * minor;
        const int c = dr > dc ? c0 + sc * minor : c0 + sc * i;
        hit |= cell_is_not_one(r, c);
    }
    return __any(hit);
}

// closest[:, i, j] of an int32 [2][R][C] block (OccupancyMap._closest_valid_cspace_indices, envs.py:2522-2523); false when it names
// no cell of the grid
__device__ __forceinline__ bool snap(const int32_t* __restrict__ cl, int R, int C, int& i, int& j) {
    const int a = cl[i * C + j], b = cl[R * C + i * C + j];
    if (a < 0 || a >= R || b < 0 || b >= C) return false;
    i = a;
    j = b;
    return true;
}

// every free cell of the n_cells of g lies inside the window (wave-uniform): one pass over the grid, 16 bytes at a time where aligned
__device__ __forceinline__ bool free_cells_inside(const uint8_t* __restrict__ g, int n_cells, int C, const Window& b, int lane) {
    bool outside = false;
    const int lead = min(n_cells, (int)((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15));
    const int chunks = (n_cells - lead) / 16;
    auto check = [&](int idx, int count) {
        int r = idx / C, c = idx - r * C;
        for (int t = 0; t < count; ++t) {
            if (g[idx + t] != 0 && !b.holds(r, c)) outside = true;
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
    return !__any(outside);
}

// the state before the search: every distance inf but the source's (s_l, -1 when it lies outside the window: 0 there even when the
// cell is blocked, which the distance image of simq_grid_paths documents), no parents, the flags from the grid, the halo blocked.
// Returns the number of vertices (wave-uniform); the state is visible to every lane on return.
template <bool kKeepOne, typename State>
__device__ __forceinline__ int init_window(const State& lds, const uint8_t* __restrict__ g, int C, const Window& b, int s_l, float inf,
                                           int lane) {
    int vertices = 0;
    for (int l = lane; l < lds.N; l += kLanes) {
        const int li = l / lds.W, lj = l - li * lds.W;
        const bool inner = li >= 1 && li <= b.rows && lj >= 1 && lj <= b.cols;
        const unsigned cell = inner ? g[(b.i0 + li - 1) * C + (b.j0 + lj - 1)] : 0u;
        lds.dist[l] = l == s_l ? 0.f : inf;
        lds.par[l] = kNoParent;
        lds.flg[l] = (uint8_t)((cell != 0u ? kFree : 0u) | (kKeepOne && cell == 1u ? kOne : 0u));
        vertices += cell != 0u ? 1 : 0;
    }
    for (int o = kLanes / 2; o >= 1; o >>= 1) vertices += __shfl_xor(vertices, o, kLanes);
    __syncthreads();
    return vertices;
}

// the search from the free window cell s_l over a ring of Q = vertices + 1 slots: distances and parents as the reference leaves them.
// Returns 0, or 4 when the pop cap was passed (cannot happen); the state is visible to every lane on return.
template <bool kKeepOne, typename State>
__device__ __forceinline__ int search(const State lds, int s_l, int Q, int lane) {
    using Entry = typename State::Entry;
    float* const dist = lds.dist;
    Entry* const ring = lds.ring;
    uint8_t* const par = lds.par;
    uint8_t* const flg = lds.flg;
    const int W = lds.W;
    const int k = lane & 7;
    const int my_off = dir_di(k) * W + dir_dj(k);
    const float my_w = dir_w(k);
    int st = 0;
    int head = 0, tail = 1;
    int hp = 1 % Q, tp = 1 % Q;                      // ring positions of slot head + 1 (the front) and of slot tail
    int f = s_l;                                     // the front vertex (slot head + 1), -1 when nothing is queued
    float df = 0.f;                                  // ... and its distance as it stands
    if (lane == 0) {
        ring[hp] = (Entry)s_l;
        if (kKeepOne) flg[s_l] |= kQueued;
        else flg[s_l] = kFree | kQueued;
    }
    const int64_t pop_cap = 64 * (int64_t)(Q - 1) + 64;
    int64_t pops = 0;
    __syncthreads();
    while (head < tail) {
        if (++pops > pop_cap) { st = 4; break; }
        ++head;
        const int u = f;
        const float du = df;
        unsigned fu = kFree | kQueued;
        if (kKeepOne) fu = flg[u];
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
            if (!(fv & kQueued)) flg[v] = kKeepOne ? (uint8_t)(fv | kQueued) : (uint8_t)(kFree | kQueued);
        }
        if (lane == 0) flg[u] = (uint8_t)(fu & ~kQueued);   // in_queue[u] = 0
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
                    if (lane == 0) ring[tp] = (Entry)vk;
                    f = vk;
                    df = nk;
                } else if (nk < df) {
                    if (lane == 0) { ring[tp] = (Entry)f; ring[hp] = (Entry)vk; }
                    f = vk;
                    df = nk;
                } else if (lane == 0) {
                    ring[tp] = (Entry)vk;
                }
            }
        }
        __syncthreads();
    }
    __syncthreads();
    return st;
}

}  // namespace grid_spfa

}  // namespace simq
