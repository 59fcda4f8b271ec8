// libsimq: batched single-source shortest-path distance images on 8-connected grids
//   grid_distance_kernel     GridGraph(grid) + GridGraph._spfa distances + the -1 fill   shortest_paths.pyx:26-67, 69-114
//                            (+ optional Mapper epilogue: / pixels_per_meter, <0 -> max, * scale   envs.py:2287-2300, 2513-2516)
//
// Exactness.  The reference relaxes edge (u, v) with new = fl32(d[u] + w), w in {1, fl32(sqrt 2)}, and accepts it only when strictly
// smaller.  Any label-correcting scheme that makes only such updates and stops when no edge improves any label ends at the same values:
// per vertex the minimum over paths of the left-to-right fp32 sum of the weights.  So the order of the updates below is free; what
// is not free is the arithmetic (one fp32 add per update, nothing to contract it with) and the stopping rule (a whole pass over every
// edge with no improvement).
//
// Algorithm: one wavefront per problem; the image itself (d_out) is the working buffer.  The wave covers 256 columns at a time (4
// adjacent cells per lane) and walks the rows, alternately top -> bottom and bottom -> top (Gauss-Seidel sweeps of the fast-sweeping
// kind).  At row r it relaxes r's cells from row r - dir (final for this pass, held in registers) and from row r + dir (the previous
// pass's values), then solves the row's horizontal edges to their fixed point: in-lane forward + backward sweeps, cross-lane halos by
// shuffles, repeated until no lane's end cell moved.  A path that snakes through the rows in the direction of a pass is resolved in that
// one pass.  Only the bounding box of the free cells is walked (nothing outside it can change); a box wider than 256 columns takes
// several column blocks per pass, whose edge lanes read the neighbouring block's cells from memory.  Passes repeat until one changes
// nothing (every edge then satisfies d[v] <= fl32(d[u] + w) with the final values), capped at rows * cols + 1 passes: a pass relaxes
// every edge with values at least as new as one Jacobi sweep would, and rows * cols - 1 Jacobi sweeps reach the fixed point.  Hitting
// the cap writes status 1 and stops.
#include "batch_abi.h"
#include "../../include/simq.h"

#include <vector>

namespace simq {

namespace {

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

__global__ void __launch_bounds__(kLanes) grid_distance_kernel(const uint8_t* __restrict__ grids, const simq_grid_problem* __restrict__ probs,
                                                               float* out, float ppm, int unreachable_to_max, float scale,
                                                               int32_t* __restrict__ status) {
    const simq_grid_problem p = probs[blockIdx.x];
    const int lane = threadIdx.x;
    const int R = p.rows, C = p.cols;
    if (R < 1 || C < 1 || (int64_t)R * C >= SIMQ_GRID_MAX_CELLS || p.src_i < 0 || p.src_i >= R || p.src_j < 0 || p.src_j >= C ||
        p.grid_offset < 0 || p.out_offset < 0) {
        if (lane == 0) status[blockIdx.x] = 2;          // (the host validated already: nothing is read or written)
        return;
    }
    const int n = R * C;
    const uint8_t* g = grids + p.grid_offset;
    float* d = out + p.out_offset;
    const float inf = 2.f * (float)n;                    // self.inf = 2 * max_num_verts (exact: < 2^24)
    const int src = p.src_i * C + p.src_j;

    // bounding box of the free cells: nothing outside it ever changes (a blocked cell has no edge), so the passes walk only the box
    // (a Mapper's configuration space is free inside the room only: ~44 x 92 cells of a 184 x 232 grid)
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
    const Box box = {rlo, rhi + 1, clo, chi + 1, C};     // empty when no cell is free
    __threadfence_block();

    const int cap = n + 1;
    const int nrows = max(box.rhi - box.rlo, 0);
    const int nblocks = box.chi > box.clo ? (box.chi - box.clo + kBlockCols - 1) / kBlockCols : 0;
    bool changed = true;
    float dmax = 0.f;                                    // max finite distance the last pass saw (the final one when it changed nothing)
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
    for (int o = kLanes / 2; o >= 1; o >>= 1) dmax = fmaxf(dmax, __shfl_xor(dmax, o, kLanes));

    // the reference's order: img = dists / ppm (the -1 fill included); img[img < 0] = img.max(); img *= scale.  Correctly rounded
    // division is monotone, so the image max is fl32(dmax / ppm) (dmax >= 0: the source holds 0).
    const float fill = unreachable_to_max ? dmax / ppm : -1.f / ppm;
    for (int i = lane; i < n; i += kLanes) {
        const float x = d[i];
        const float q = x == inf ? fill : x / ppm;
        d[i] = q * scale;
    }
    if (lane == 0) status[blockIdx.x] = changed ? 1 : 0;
}

}  // namespace

}  // namespace simq

using namespace simq;

extern "C" int simq_grid_distance_images(const uint8_t* d_grids, int64_t grids_bytes, const simq_grid_problem* problems, int n,
                                         simq_grid_problem* d_problems, float* d_out, int64_t out_floats, float pixels_per_meter,
                                         int unreachable_to_max, float scale, int32_t* d_status, void* stream) {
    SIMQ_REQUIRE(d_grids && problems && d_problems && d_out && d_status, "grid_distance_images: NULL pointer");
    SIMQ_REQUIRE(n >= 1 && n <= (1 << 24), "grid_distance_images: n = %d (1 .. 2^24 problems)", n);
    SIMQ_REQUIRE(pixels_per_meter > 0.f && pixels_per_meter <= 3.4e38f, "grid_distance_images: pixels_per_meter = %g (> 0, finite; 1 = none)",
                 (double)pixels_per_meter);
    SIMQ_REQUIRE(scale >= -3.4e38f && scale <= 3.4e38f, "grid_distance_images: scale = %g (finite; 1 = none)", (double)scale);
    std::vector<Span> spans;
    spans.reserve(n);
    for (int i = 0; i < n; ++i) {
        const simq_grid_problem& p = problems[i];
        SIMQ_REQUIRE(p.rows >= 1 && p.cols >= 1 && (int64_t)p.rows * p.cols < SIMQ_GRID_MAX_CELLS,
                     "grid_distance_images: problem %d is %d x %d (rows, cols >= 1, rows * cols < 2^22)", i, p.rows, p.cols);
        SIMQ_REQUIRE(p.src_i >= 0 && p.src_i < p.rows && p.src_j >= 0 && p.src_j < p.cols,
                     "grid_distance_images: problem %d: source (%d, %d) outside its %d x %d grid", i, p.src_i, p.src_j, p.rows, p.cols);
        const int64_t cells = (int64_t)p.rows * p.cols;
        SIMQ_REQUIRE(fits(p.grid_offset, cells, grids_bytes),
                     "grid_distance_images: problem %d: grid bytes [%lld, %lld) outside the %lld of d_grids", i, (long long)p.grid_offset,
                     (long long)(p.grid_offset + cells), (long long)grids_bytes);
        SIMQ_REQUIRE(fits(p.out_offset, cells, out_floats),
                     "grid_distance_images: problem %d: image floats [%lld, %lld) outside the %lld of d_out", i, (long long)p.out_offset,
                     (long long)(p.out_offset + cells), (long long)out_floats);
        spans.push_back({(uint64_t)p.out_offset, (uint64_t)(p.out_offset + cells), i});
    }
    const size_t clash = first_overlap(spans);
    SIMQ_REQUIRE(clash == 0, "grid_distance_images: two images overlap in d_out at float %lld", (long long)spans[clash].lo);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const HostBlock block = {problems, sizeof(simq_grid_problem) * (size_t)n};
    SIMQ_CHECK_HIP(upload_descriptors(d_problems, &block, 1, nullptr, s));
    grid_distance_kernel<<<n, kLanes, 0, s>>>(d_grids, d_problems, d_out, pixels_per_meter, unreachable_to_max, scale, d_status);
    SIMQ_CHECK_LAUNCH();
    note_launch("grid_distance");
    return 0;
}
