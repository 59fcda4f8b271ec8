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
// Algorithm: one wavefront per problem; the image itself (d_out) is the working buffer.  The row walk -- Gauss-Seidel passes over
// the bounding box of the free cells, alternately down and up, until one changes nothing, capped at rows * cols + 1 passes -- is
// grid_relax.h, shared with grid_queries.hip.  Hitting the cap writes status 1 and stops.
//
//   grid_distance_snapped_kernel   the same image with OccupancyMap._closest_valid_cspace_indices in front (envs.py:2513-2516,
//                            2522-2523): the source goes through closest[:, i, j] on the device, and a problem whose upstream
//                            status word is nonzero is not searched at all.  Every branch that leaves early is taken by the whole
//                            wave (the descriptor, the upstream word and the closest pair are one address for all 64 lanes), so the
//                            shuffles and votes of the relaxation always run with every lane.
#include "batch_abi.h"
#include "grid_relax.h"
#include "../../include/simq.h"

#include <vector>

namespace simq {

namespace {

using namespace grid_relax;

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

    const Box box = init_labels(g, d, R, C, src, inf, lane);
    float dmax;                                          // max finite distance the last pass saw (the final one when it changed nothing)
    const bool changed = relax_passes(g, d, box, n, inf, lane, &dmax);
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

// every cell of a problem that is not searched: SIMQ_GRID_SNAPPED_FILL
__device__ __forceinline__ void fill_image(float* d, int n, int lane) {
    for (int i = lane; i < n; i += kLanes) d[i] = SIMQ_GRID_SNAPPED_FILL;
}

__global__ void __launch_bounds__(kLanes) grid_distance_snapped_kernel(const uint8_t* __restrict__ grids, const int32_t* __restrict__ closest,
                                                                       const simq_grid_snapped_problem* __restrict__ probs, float* out,
                                                                       float ppm, int unreachable_to_max, float scale,
                                                                       const int32_t* __restrict__ upstream, int32_t* __restrict__ status,
                                                                       int64_t grids_bytes, int64_t closest_ints, int64_t out_floats,
                                                                       int n_upstream) {
    const simq_grid_snapped_problem p = probs[blockIdx.x];
    const int lane = threadIdx.x;
    const int R = p.rows, C = p.cols;
    if (R < 1 || C < 1 || (int64_t)R * C >= SIMQ_GRID_MAX_CELLS || p.src_i < 0 || p.src_i >= R || p.src_j < 0 || p.src_j >= C ||
        p.grid_offset < 0 || p.grid_offset > grids_bytes - (int64_t)R * C || p.out_offset < 0 ||
        p.out_offset > out_floats - (int64_t)R * C || p.closest_offset < 0 || p.closest_offset > closest_ints - 2 * (int64_t)R * C ||
        p.upstream < -1 || p.upstream >= n_upstream) {
        if (lane == 0) status[blockIdx.x] = 2;          // (the host validated already: nothing is read or written)
        return;
    }
    const int n = R * C;
    const uint8_t* g = grids + p.grid_offset;
    const int32_t* cl = closest + p.closest_offset;
    float* d = out + p.out_offset;

    // ---- a problem whose producer failed (its closest cells are undefined) is not searched: its code is passed on
    const int up = p.upstream >= 0 ? upstream[p.upstream] : 0;
    if (up != 0) {
        fill_image(d, n, lane);
        if (lane == 0) status[blockIdx.x] = up;
        return;
    }

    // ---- OccupancyMap._closest_valid_cspace_indices on the source (envs.py:2515, 2522-2523): a pair that names no free cell of
    // the grid is a status, never an address
    const int si = cl[p.src_i * C + p.src_j], sj = cl[n + p.src_i * C + p.src_j];
    if (si < 0 || si >= R || sj < 0 || sj >= C || g[si * C + sj] == 0) {
        fill_image(d, n, lane);
        if (lane == 0) status[blockIdx.x] = 3;
        return;
    }

    // ---- GridGraph._spfa's distances and the Mapper epilogue, as grid_distance_kernel
    const float inf = 2.f * (float)n;                    // self.inf = 2 * max_num_verts (exact: < 2^24)
    const Box box = init_labels(g, d, R, C, si * C + sj, inf, lane);
    float dmax;
    const bool changed = relax_passes(g, d, box, n, inf, lane, &dmax);
    for (int o = kLanes / 2; o >= 1; o >>= 1) dmax = fmaxf(dmax, __shfl_xor(dmax, o, kLanes));
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

extern "C" int simq_grid_distance_images_snapped(const uint8_t* d_grids, int64_t grids_bytes, const int32_t* d_closest, int64_t closest_ints,
                                                 const simq_grid_snapped_problem* problems, int n, simq_grid_snapped_problem* d_problems,
                                                 float* d_out, int64_t out_floats, float pixels_per_meter, int unreachable_to_max,
                                                 float scale, const int32_t* d_upstream, int n_upstream, int32_t* d_status, void* stream) {
    SIMQ_REQUIRE(d_grids && d_closest && problems && d_problems && d_out && d_status, "grid_distance_images_snapped: NULL pointer");
    SIMQ_REQUIRE(n >= 1 && n <= (1 << 24), "grid_distance_images_snapped: n = %d (1 .. 2^24 problems)", n);
    SIMQ_REQUIRE(pixels_per_meter > 0.f && pixels_per_meter <= 3.4e38f,
                 "grid_distance_images_snapped: pixels_per_meter = %g (> 0, finite; 1 = none)", (double)pixels_per_meter);
    SIMQ_REQUIRE(scale >= -3.4e38f && scale <= 3.4e38f, "grid_distance_images_snapped: scale = %g (finite; 1 = none)", (double)scale);
    SIMQ_REQUIRE(grids_bytes >= 0 && closest_ints >= 0 && out_floats >= 0 && grids_bytes < (1LL << 40) && closest_ints < (1LL << 40) &&
                     out_floats < (1LL << 40),
                 "grid_distance_images_snapped: buffer sizes %lld, %lld, %lld (each in [0, 2^40))", (long long)grids_bytes,
                 (long long)closest_ints, (long long)out_floats);
    SIMQ_REQUIRE(n_upstream >= 0 && n_upstream <= (1 << 24) && (n_upstream == 0 || d_upstream),
                 "grid_distance_images_snapped: n_upstream = %d (0 .. 2^24 status words; 0: d_upstream is not read)", n_upstream);
    SIMQ_REQUIRE(((uintptr_t)d_problems & 7) == 0 && ((uintptr_t)d_closest & 3) == 0 && ((uintptr_t)d_out & 3) == 0 &&
                     ((uintptr_t)d_upstream & 3) == 0 && ((uintptr_t)d_status & 3) == 0,
                 "grid_distance_images_snapped: d_problems must be 8-byte, d_closest, d_out, d_upstream and d_status 4-byte aligned");
    std::vector<Span> spans;
    spans.reserve(n);
    for (int i = 0; i < n; ++i) {
        const simq_grid_snapped_problem& p = problems[i];
        SIMQ_REQUIRE(p.rows >= 1 && p.cols >= 1 && (int64_t)p.rows * p.cols < SIMQ_GRID_MAX_CELLS,
                     "grid_distance_images_snapped: problem %d is %d x %d (rows, cols >= 1, rows * cols < 2^22)", i, p.rows, p.cols);
        SIMQ_REQUIRE(p.src_i >= 0 && p.src_i < p.rows && p.src_j >= 0 && p.src_j < p.cols,
                     "grid_distance_images_snapped: problem %d: source (%d, %d) outside its %d x %d grid", i, p.src_i, p.src_j, p.rows,
                     p.cols);
        const int64_t cells = (int64_t)p.rows * p.cols;
        SIMQ_REQUIRE(fits(p.grid_offset, cells, grids_bytes),
                     "grid_distance_images_snapped: problem %d: grid bytes [%lld, %lld) outside the %lld of d_grids", i,
                     (long long)p.grid_offset, (long long)(p.grid_offset + cells), (long long)grids_bytes);
        SIMQ_REQUIRE(fits(p.closest_offset, 2 * cells, closest_ints),
                     "grid_distance_images_snapped: problem %d: closest ints [%lld, %lld) outside the %lld of d_closest", i,
                     (long long)p.closest_offset, (long long)(p.closest_offset + 2 * cells), (long long)closest_ints);
        SIMQ_REQUIRE(fits(p.out_offset, cells, out_floats),
                     "grid_distance_images_snapped: problem %d: image floats [%lld, %lld) outside the %lld of d_out", i,
                     (long long)p.out_offset, (long long)(p.out_offset + cells), (long long)out_floats);
        SIMQ_REQUIRE(p.upstream >= -1 && p.upstream < n_upstream,
                     "grid_distance_images_snapped: problem %d: upstream = %d (-1: none, or one of the %d words of d_upstream)", i,
                     p.upstream, n_upstream);
        spans.push_back({(uint64_t)p.out_offset, (uint64_t)(p.out_offset + cells), i});
    }
    const size_t clash = first_overlap(spans);
    SIMQ_REQUIRE(clash == 0, "grid_distance_images_snapped: problems %d and %d share image floats from %lld on", spans[clash - 1].problem,
                 spans[clash].problem, (long long)spans[clash].lo);

    // every buffer the launch writes against every other buffer of the call (an absent or empty buffer takes no part)
    const int64_t prob_bytes = (int64_t)sizeof(simq_grid_snapped_problem) * n;
    const Buffer all[] = {{"d_out", d_out, 4 * out_floats, true},
                          {"d_status", d_status, 4LL * n, true},
                          {"d_problems", d_problems, prob_bytes, true},
                          {"d_grids", d_grids, grids_bytes, false},
                          {"d_closest", d_closest, 4 * closest_ints, false},
                          {"d_upstream", d_upstream, 4LL * n_upstream, false}};
    Buffer bufs[6];
    int nb = 0;
    for (const Buffer& b : all)
        if (b.p && b.bytes > 0) bufs[nb++] = b;
    int a = 0, b = 0;
    SIMQ_REQUIRE(!first_conflict(bufs, nb, &a, &b), "grid_distance_images_snapped: %s overlaps %s", bufs[a].name, bufs[b].name);

    hipStream_t s = static_cast<hipStream_t>(stream);
    const HostBlock block = {problems, (size_t)prob_bytes};
    SIMQ_CHECK_HIP(upload_descriptors(d_problems, &block, 1, nullptr, s));
    grid_distance_snapped_kernel<<<n, kLanes, 0, s>>>(d_grids, d_closest, d_problems, d_out, pixels_per_meter, unreachable_to_max, scale,
                                                      d_upstream, d_status, grids_bytes, closest_ints, out_floats, n_upstream);
    SIMQ_CHECK_LAUNCH();
    note_launch("grid_distance_snapped");
    return 0;
}
