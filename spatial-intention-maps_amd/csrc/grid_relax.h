// The label-correcting relaxation that grid_paths.hip (distance images) and grid_queries.hip (point queries) share: one wavefront,
// one problem, the fp32 image in global memory as the working buffer.  The rules and why any order of such updates ends at SPFA's
// distances are stated at the top of grid_paths.hip; this header holds the row walk and nothing of an entry point.
//
// The wave covers 256 columns at a time (4 adjacent cells per lane) and walks the rows, alternately top -> bottom and bottom -> top
// (Gauss-Seidel sweeps of the fast-sweeping kind).  At row r it relaxes r's cells from row r - dir (final for this pass, held in
// registers) and from row r + dir (the previous pass's values), then solves the row's horizontal edges to their fixed point: in-lane
// forward + backward sweeps, cross-lane halos by shuffles, repeated until no lane's end cell moved.  Only the bounding box of the free
// cells is walked (nothing outside it can change); a box wider than 256 columns takes several column blocks per pass, whose edge lanes
// read the neighbouring block's cells from memory.
#pragma once
#include "common.h"

namespace simq {

namespace grid_relax {

constexpr int kLanes = 64;
constexpr int kCells = 4;                         // adjacent cells per lane
constexpr int kBlockCols = kLanes * kCells;       // columns per block walk
// float32(sqrt 2) of `cdef float sqrt_2 = np.sqrt(2)` (shortest_paths.pyx:31): 0x3FB504F3
constexpr float kSqrt2 = 1.41421353816986083984375f;

// the walked window: rows [rlo, rhi), columns [clo, chi) of a grid with row stride C
struct Box {
    int rlo, rhi, clo, chi, C;
};

struct Row {
    float v[kCells];   // the lane's cells (inf outside the box)
    unsigned f;        // bit k: cell k is free (never for cells outside the box)
    float el, er;      // block-edge lanes only: the cell left of the block / right of it
    unsigned ef;       // bit 0: el's cell free, bit 1: er's cell free
};

__device__ __forceinline__ void load_row(Row& row, const uint8_t* __restrict__ g, const float* d, const Box& box, int r, int c0, int b0,
                                         int lane, float inf) {
    row.f = 0u;
    row.ef = 0u;
    row.el = inf;
    row.er = inf;
#pragma unroll
    for (int k = 0; k < kCells; ++k) row.v[k] = inf;
    if (r < box.rlo || r >= box.rhi) return;
    const int64_t base = (int64_t)r * box.C;
#pragma unroll
    for (int k = 0; k < kCells; ++k) {
        const int c = c0 + k;
        if (c < box.chi) {
            row.v[k] = d[base + c];
            row.f |= (g[base + c] != 0 ? 1u : 0u) << k;
        }
    }
    if (lane == 0 && b0 > box.clo) {
        row.el = d[base + b0 - 1];
        row.ef |= g[base + b0 - 1] != 0 ? 1u : 0u;
    }
    if (lane == kLanes - 1 && b0 + kBlockCols < box.chi) {
        row.er = d[base + b0 + kBlockCols];
        row.ef |= g[base + b0 + kBlockCols] != 0 ? 2u : 0u;
    }
}

// the cells of `row` at columns c0 - 1 .. c0 + kCells (ev[0], ev[kCells + 1]: the neighbouring lanes' / the neighbouring block's)
__device__ __forceinline__ void extend(const Row& row, int lane, float* ev, unsigned* ef) {
    float lv = __shfl_up(row.v[kCells - 1], 1, kLanes);
    unsigned lf = __shfl_up((row.f >> (kCells - 1)) & 1u, 1, kLanes);
    float rv = __shfl_down(row.v[0], 1, kLanes);
    unsigned rf = __shfl_down(row.f & 1u, 1, kLanes);
    if (lane == 0) { lv = row.el; lf = row.ef & 1u; }
    if (lane == kLanes - 1) { rv = row.er; rf = (row.ef >> 1) & 1u; }
    ev[0] = lv;
#pragma unroll
    for (int k = 0; k < kCells; ++k) ev[k + 1] = row.v[k];
    ev[kCells + 1] = rv;
    *ef = lf | (row.f << 1) | (rf << (kCells + 1));
}

// relax the free cells of `cur` from an adjacent row (its extended form): straight 1, diagonal sqrt 2
__device__ __forceinline__ bool relax_from(Row& cur, const float* ev, unsigned ef) {
    bool chg = false;
#pragma unroll
    for (int k = 0; k < kCells; ++k) {
        if (!((cur.f >> k) & 1u)) continue;
#pragma unroll
        for (int dj = -1; dj <= 1; ++dj) {
            if (!((ef >> (k + 1 + dj)) & 1u)) continue;
            const float t = ev[k + 1 + dj] + (dj == 0 ? 1.f : kSqrt2);
            if (t < cur.v[k]) { cur.v[k] = t; chg = true; }
        }
    }
    return chg;
}

// the row's horizontal edges (weight 1) to their fixed point; returns whether a cell of this lane changed
__device__ __forceinline__ bool relax_row(Row& cur, int lane) {
    bool chg = false;
    for (;;) {
        float ev[kCells + 2];
        unsigned ef;
        extend(cur, lane, ev, &ef);
        const float first = cur.v[0], last = cur.v[kCells - 1];
        float nb = ev[0];
        bool nbf = ef & 1u;
#pragma unroll
        for (int k = 0; k < kCells; ++k) {                       // left -> right
            const bool fk = (cur.f >> k) & 1u;
            if (fk && nbf) {
                const float t = nb + 1.f;
                if (t < cur.v[k]) { cur.v[k] = t; chg = true; }
            }
            nb = cur.v[k];
            nbf = fk;
        }
        nb = ev[kCells + 1];
        nbf = (ef >> (kCells + 1)) & 1u;
#pragma unroll
        for (int k = kCells - 1; k >= 0; --k) {                  // right -> left
            const bool fk = (cur.f >> k) & 1u;
            if (fk && nbf) {
                const float t = nb + 1.f;
                if (t < cur.v[k]) { cur.v[k] = t; chg = true; }
            }
            nb = cur.v[k];
            nbf = fk;
        }
        // with its halos fixed, one forward + backward sweep is a lane's 1-D fixed point: only a moved end cell changes a neighbour's halo
        const bool ends_moved = cur.v[0] != first || cur.v[kCells - 1] != last;
        if (!__any(ends_moved)) break;
    }
    return chg;
}

// d = inf everywhere, 0 at the ravelled cell `src`, over the R * C cells of the grid; returns the bounding box of the free cells
// (empty when no cell is free).  Nothing outside that box ever changes (a blocked cell has no edge), so the passes walk only the box
// (a Mapper's configuration space is free inside the room only: ~44 x 92 cells of a 184 x 232 grid).  The wave's stores are fenced:
// the passes read them back through other lanes.
__device__ __forceinline__ Box init_labels(const uint8_t* __restrict__ g, float* d, int R, int C, int src, float inf, int lane) {
    const int n = R * C;
    int rlo = R, rhi = -1, clo = C, chi = -1;
    for (int i = lane; i < n; i += kLanes) {
        d[i] = i == src ? 0.f : inf;
        if (g[i] != 0) {
            const int r = i / C, c = i - r * C;
            rlo = min(rlo, r); rhi = max(rhi, r); clo = min(clo, c); chi = max(chi, c);
        }
    }
    for (int o = kLanes / 2; o >= 1; o >>= 1) {
        rlo = min(rlo, __shfl_xor(rlo, o, kLanes)); rhi = max(rhi, __shfl_xor(rhi, o, kLanes));
        clo = min(clo, __shfl_xor(clo, o, kLanes)); chi = max(chi, __shfl_xor(chi, o, kLanes));
    }
    const Box box = {rlo, rhi + 1, clo, chi + 1, C};
    __threadfence_block();
    return box;
}

// Passes over the box until one changes nothing (every edge then satisfies d[v] <= fl32(d[u] + w) with the final values), capped at
// n + 1 passes: a pass relaxes every edge with values at least as new as one Jacobi sweep would, and n - 1 Jacobi sweeps reach the
// fixed point.  Returns whether the cap ended the loop (the image is then not the fixed point); *dmax: each lane's largest finite
// distance of the last pass (the final one when it changed nothing).  Every column block ends in a fence: the next block's edge lanes,
// the next pass and whatever the caller reads afterwards see the rows this wave stored.
__device__ __forceinline__ bool relax_passes(const uint8_t* __restrict__ g, float* d, const Box& box, int n, float inf, int lane,
                                             float* dmax_out) {
    const int C = box.C;
    const int cap = n + 1;
    const int nrows = max(box.rhi - box.rlo, 0);
    const int nblocks = box.chi > box.clo ? (box.chi - box.clo + kBlockCols - 1) / kBlockCols : 0;
    bool changed = true;
    float dmax = 0.f;
    for (int pass = 0; pass < cap && changed; ++pass) {
        changed = false;
        dmax = 0.f;
        const bool down = (pass & 1) == 0;
        const int dir = down ? 1 : -1;
        const int r0 = down ? box.rlo : box.rhi - 1;
        for (int bi = 0; bi < nblocks; ++bi) {
            const int b0 = box.clo + (down ? bi : nblocks - 1 - bi) * kBlockCols;
            const int c0 = b0 + lane * kCells;
            Row prev, cur, nxt, nn;
            load_row(prev, g, d, box, r0 - dir, c0, b0, lane, inf);
            load_row(cur, g, d, box, r0, c0, b0, lane, inf);
            load_row(nxt, g, d, box, r0 + dir, c0, b0, lane, inf);
            load_row(nn, g, d, box, r0 + 2 * dir, c0, b0, lane, inf);
            for (int s = 0; s < nrows; ++s) {
                const int r = r0 + s * dir;
                float ev[kCells + 2];
                unsigned ef;
                bool chg = false;
                extend(prev, lane, ev, &ef);
                chg |= relax_from(cur, ev, ef);
                extend(nxt, lane, ev, &ef);
                chg |= relax_from(cur, ev, ef);
                chg |= relax_row(cur, lane);
                if (chg) {
                    const int64_t base = (int64_t)r * C;
#pragma unroll
                    for (int k = 0; k < kCells; ++k)
                        if (c0 + k < box.chi) d[base + c0 + k] = cur.v[k];
                    changed = true;
                }
#pragma unroll
                for (int k = 0; k < kCells; ++k)
                    if (cur.v[k] < inf) dmax = fmaxf(dmax, cur.v[k]);
                prev = cur;
                cur = nxt;
                nxt = nn;
                load_row(nn, g, d, box, r + 3 * dir, c0, b0, lane, inf);
            }
            __threadfence_block();                       // the next block's edge lanes (and the next pass) read these rows
        }
        changed = __any(changed);
    }
    *dmax_out = dmax;
    return changed;
}

}  // namespace grid_relax

}  // namespace simq
