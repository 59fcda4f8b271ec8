// libsimq: batched observation maps -- a camera frame into the persistent overhead and occupancy maps
//   observation_maps_kernel  depth, point cloud and segmentation of Camera.capture_image               envs.py:1926-1954
//                            the height-ordered scatter of Mapper.update into the overhead map        envs.py:2053-2061
//                            the obstacle scatter of OccupancyMap.update into the occupancy map       envs.py:2444-2449
//   observation_sequences_kernel  several frames per pair of maps, applied in the order given (at the end of this file)
//
// Exactness.  Everything the reference computes here is float32, one numpy operation per product, sum and quotient.  The projection is
// compiled with contraction off (the ISA holds v_mul_f32 / v_add_f32 / v_sub_f32 and no fused form) and the division is the compiler's
// correctly rounded one.  The reference assigns seg values in ascending order of the point's z, so a pixel ends with the seg of its
// highest point; among equal heights this project fixes the order a stable sort gives: the largest frame index wins.  Both are one
// maximum over the 64-bit key (order-preserving bits of z) << 32 | frame index, taken in LDS (ds_max_u64): the order in which lanes
// arrive does not matter.  Finite floats order as their bit patterns with the sign bit flipped (positive) or all bits flipped
// (negative); -0 is folded into +0 first.  No finite point has key 0, which marks a pixel nothing landed on.
//
// Shape.  One workgroup of 1024 lanes per 32 x 256 tile of one problem's maps: 64 KB of keys and 8 KB of occupancy bytes in LDS.  Every
// workgroup streams all height * width points of its problem, one lane per point (a dozen fp32 operations and two coalesced loads), and
// keeps those that land in its tile.  Every workgroup of a problem therefore sees a non-finite point itself and none of them writes:
// no flag crosses workgroups, and there are no global atomics, no workspace and no second launch.  The second pass walks the tile with
// consecutive lanes on consecutive pixels of a row: a pixel with a key reads its winner's id again and stores the seg, an occupancy byte
// that was set stores 1 (plain vector stores; every writer of a byte stores the same value); everything else is left untouched.
#include "batch_abi.h"
#include "../../include/simq.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace simq {

namespace {

constexpr int kTileRows = 32;
constexpr int kTileCols = 256;
constexpr int kTilePixels = kTileRows * kTileCols;
constexpr int kThreads = 1024;
constexpr int kMaxPoints = SIMQ_OBSERVATION_MAX_POINTS;
constexpr int64_t kMaxCells = 1 << 28;
constexpr int kMaxSide = 1 << 24;                                                     // rows, cols, rows - 1 and rows / 2 exact in fp32

// Camera.capture_image's seg value of body id `raw`: a sum of eighths, exact in any order
__device__ __forceinline__ float seg_value(const simq_observation_problem& p, int raw) {
    float s = raw == 0 ? 0.125f : 0.f;
    s += (raw >= p.min_obstacle && raw <= p.max_obstacle) ? 0.25f : 0.f;
    s += (p.has_receptacle && raw == p.receptacle) ? 0.375f : 0.f;
    s += (raw >= p.min_cube && raw <= p.max_cube) ? 0.5f : 0.f;
    return s;
}

// the frame pixel (h, w) with depth-buffer value `buffer` as a world point; hipcc contracts a * b + c into v_fma_f32 by default, numpy
// rounds the product and the sum separately
__device__ __forceinline__ void project(const simq_observation_problem& p, float buffer, float px, float py, float& x, float& y, float& z) {
#pragma clang fp contract(off)
    const float scaled = p.far_minus_near * buffer;
    const float denom = p.far - scaled;
    const float depth = p.far_near / denom;
    const float rx = px * p.right[0], ry = px * p.right[1], rz = px * p.right[2];
    const float ux = py * p.up[0], uy = py * p.up[1], uz = py * p.up[2];
    const float dx = (p.principal[0] + rx) + ux, dy = (p.principal[1] + ry) + uy, dz = (p.principal[2] + rz) + uz;
    const float sx = depth * dx, sy = depth * dy, sz = depth * dz;
    x = p.cam[0] + sx;
    y = p.cam[1] + sy;
    z = p.cam[2] + sz;
}

// Mapper.position_to_pixel_indices of one coordinate: clip(floor(half + sign * v * 96), 0, size - 1), the product and the sum rounded apart
__device__ __forceinline__ int pixel_index(float half, float v, bool minus, int size) {
#pragma clang fp contract(off)
    const float scaled = v * 96.f;
    const float t = minus ? half - scaled : half + scaled;
    float f = floorf(t);
    f = f > 0.f ? f : 0.f;
    const float top = (float)(size - 1);
    f = f < top ? f : top;
    return (int)f;
}

__device__ __forceinline__ bool descriptor_ok(const simq_observation_problem& p, int64_t frame_words, int64_t overhead_floats,
                                              int64_t occupancy_bytes) {
    if (p.height < 1 || p.width < 1 || (int64_t)p.height * p.width > kMaxPoints) return false;
    if (p.rows < 1 || p.cols < 1 || p.rows >= kMaxSide || p.cols >= kMaxSide || (int64_t)p.rows * p.cols >= kMaxCells) return false;
    const int64_t points = (int64_t)p.height * p.width, cells = (int64_t)p.rows * p.cols;
    return p.depth_offset >= 0 && p.depth_offset <= frame_words - points && p.ids_offset >= 0 && p.ids_offset <= frame_words - points &&
           p.px_offset >= 0 && p.px_offset <= frame_words - p.width && p.py_offset >= 0 && p.py_offset <= frame_words - p.height &&
           p.overhead_offset >= 0 && p.overhead_offset <= overhead_floats - cells && p.occupancy_offset >= 0 &&
           p.occupancy_offset <= occupancy_bytes - cells;
}

__global__ void __launch_bounds__(kThreads) observation_maps_kernel(const uint32_t* __restrict__ frames, int64_t frame_words,
                                                                    const simq_observation_problem* __restrict__ probs, int max_tiles,
                                                                    float* overhead, int64_t overhead_floats, uint8_t* occupancy,
                                                                    int64_t occupancy_bytes, int32_t* __restrict__ status) {
    __shared__ unsigned long long keys[kTilePixels];
    __shared__ uint8_t occupied[kTilePixels];
    __shared__ int not_finite;
    const int tid = threadIdx.x;
    const int p = blockIdx.x / max_tiles, t = blockIdx.x - p * max_tiles;
    const simq_observation_problem pr = probs[p];                                     // (uniform over the workgroup)
    if (tid == 0) not_finite = 0;
    for (int k = tid; k < kTilePixels; k += kThreads) {
        keys[k] = 0ull;
        occupied[k] = 0;
    }
    __syncthreads();
    if (!descriptor_ok(pr, frame_words, overhead_floats, occupancy_bytes)) {          // (the host validated already: nothing is read or written)
        if (t == 0 && tid == 0) status[p] = 2;
        return;
    }
    const int tiles_j = (pr.cols + kTileCols - 1) / kTileCols, tiles_i = (pr.rows + kTileRows - 1) / kTileRows;
    if (t >= tiles_i * tiles_j) return;                                               // (the grid is sized by the launch's largest map)
    const int ti = t / tiles_j, tj = t - ti * tiles_j;
    const int i0 = ti * kTileRows, j0 = tj * kTileCols;

    const float* depth = reinterpret_cast<const float*>(frames + pr.depth_offset);
    const int32_t* ids = reinterpret_cast<const int32_t*>(frames + pr.ids_offset);
    const float* px = reinterpret_cast<const float*>(frames + pr.px_offset);
    const float* py = reinterpret_cast<const float*>(frames + pr.py_offset);
    const int points = pr.height * pr.width;
    const float half_rows = (float)pr.rows * 0.5f, half_cols = (float)pr.cols * 0.5f;  // (exact: descriptor_ok holds rows, cols < 2^24)
    bool bad = false;
    for (int k = tid; k < points; k += kThreads) {
        const int h = k / pr.width, w = k - h * pr.width;
        float x, y, z;
        project(pr, depth[k], px[w], py[h], x, y, z);
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) {
            bad = true;
            continue;
        }
        const int li = pixel_index(half_rows, y, true, pr.rows) - i0, lj = pixel_index(half_cols, x, false, pr.cols) - j0;
        if (li < 0 || li >= kTileRows || lj < 0 || lj >= kTileCols) continue;
        const int raw = ids[k];
        uint32_t zb = z == 0.f ? 0u : __float_as_uint(z);                             // -0 and +0 are one height
        zb = (zb & 0x80000000u) ? ~zb : (zb | 0x80000000u);
        atomicMax(&keys[li * kTileCols + lj], ((unsigned long long)zb << 32) | (unsigned)k);
        if (seg_value(pr, raw) == 0.25f) occupied[li * kTileCols + lj] = 1;       // (2/8: the obstacle term and no other)
    }
    if (bad) not_finite = 1;
    __syncthreads();
    const bool skip = not_finite != 0;
    if (t == 0 && tid == 0) status[p] = skip ? 1 : 0;
    if (skip) return;

    float* o_map = overhead + pr.overhead_offset;
    uint8_t* o_occ = occupancy + pr.occupancy_offset;
    for (int k = tid; k < kTilePixels; k += kThreads) {
        const int li = k / kTileCols, lj = k - li * kTileCols;
        const int gi = i0 + li, gj = j0 + lj;
        if (gi >= pr.rows || gj >= pr.cols) continue;
        const unsigned long long key = keys[k];
        const int64_t cell = (int64_t)gi * pr.cols + gj;
        if (key != 0ull) o_map[cell] = seg_value(pr, ids[(uint32_t)key]);
        if (occupied[k]) o_occ[cell] = 1;
    }
}

}  // namespace

}  // namespace simq

using namespace simq;

extern "C" int simq_observation_update(const void* d_frames, int64_t frame_words, const simq_observation_problem* problems, int n,
                                       simq_observation_problem* d_problems, float* d_overhead, int64_t overhead_floats,
                                       uint8_t* d_occupancy, int64_t occupancy_bytes, int32_t* d_status, void* stream) {
    SIMQ_REQUIRE(d_frames && problems && d_problems && d_overhead && d_occupancy && d_status, "observation_update: NULL pointer");
    SIMQ_REQUIRE(n >= 1 && n <= (1 << 20), "observation_update: n = %d (1 .. 2^20 problems)", n);
    SIMQ_REQUIRE(frame_words >= 0 && overhead_floats >= 0 && occupancy_bytes >= 0 && frame_words < (1LL << 40) &&
                     overhead_floats < (1LL << 40) && occupancy_bytes < (1LL << 40),
                 "observation_update: buffer sizes %lld, %lld, %lld (each in [0, 2^40))", (long long)frame_words, (long long)overhead_floats,
                 (long long)occupancy_bytes);
    SIMQ_REQUIRE(((uintptr_t)d_frames & 3) == 0 && ((uintptr_t)d_overhead & 3) == 0 && ((uintptr_t)d_problems & 7) == 0 &&
                     ((uintptr_t)d_status & 3) == 0,
                 "observation_update: d_problems must be 8-byte, d_frames, d_overhead and d_status 4-byte aligned");
    const int64_t prob_bytes = (int64_t)sizeof(simq_observation_problem) * n, status_bytes = 4LL * n;
    std::vector<Span> spans;                                                          // the bytes this launch may write, as addresses
    spans.reserve(2 * (size_t)n);
    int max_tiles = 1;
    for (int i = 0; i < n; ++i) {
        const simq_observation_problem& p = problems[i];
        SIMQ_REQUIRE(p.height >= 1 && p.width >= 1 && (int64_t)p.height * p.width <= kMaxPoints,
                     "observation_update: problem %d: a frame of %d x %d (height, width >= 1, at most %d points)", i, p.height, p.width,
                     kMaxPoints);
        SIMQ_REQUIRE(p.rows >= 1 && p.cols >= 1 && p.rows < kMaxSide && p.cols < kMaxSide && (int64_t)p.rows * p.cols < kMaxCells,
                     "observation_update: problem %d: maps of %d x %d (rows, cols in [1, 2^24), rows * cols < 2^28)", i, p.rows, p.cols);
        const int64_t points = (int64_t)p.height * p.width, cells = (int64_t)p.rows * p.cols;
        SIMQ_REQUIRE(fits(p.depth_offset, points, frame_words),
                     "observation_update: problem %d: depth words [%lld, %lld) outside the %lld of d_frames", i, (long long)p.depth_offset,
                     (long long)(p.depth_offset + points), (long long)frame_words);
        SIMQ_REQUIRE(fits(p.ids_offset, points, frame_words),
                     "observation_update: problem %d: id words [%lld, %lld) outside the %lld of d_frames", i, (long long)p.ids_offset,
                     (long long)(p.ids_offset + points), (long long)frame_words);
        SIMQ_REQUIRE(fits(p.px_offset, p.width, frame_words) && fits(p.py_offset, p.height, frame_words),
                     "observation_update: problem %d: px words [%lld, +%d) or py words [%lld, +%d) outside the %lld of d_frames", i,
                     (long long)p.px_offset, p.width, (long long)p.py_offset, p.height, (long long)frame_words);
        SIMQ_REQUIRE(fits(p.overhead_offset, cells, overhead_floats),
                     "observation_update: problem %d: overhead floats [%lld, %lld) outside the %lld of d_overhead", i,
                     (long long)p.overhead_offset, (long long)(p.overhead_offset + cells), (long long)overhead_floats);
        SIMQ_REQUIRE(fits(p.occupancy_offset, cells, occupancy_bytes),
                     "observation_update: problem %d: occupancy bytes [%lld, %lld) outside the %lld of d_occupancy", i,
                     (long long)p.occupancy_offset, (long long)(p.occupancy_offset + cells), (long long)occupancy_bytes);
        bool finite = std::isfinite(p.far_near) && std::isfinite(p.far) && std::isfinite(p.far_minus_near);
        for (int c = 0; c < 3; ++c)
            finite = finite && std::isfinite(p.cam[c]) && std::isfinite(p.principal[c]) && std::isfinite(p.right[c]) && std::isfinite(p.up[c]);
        SIMQ_REQUIRE(finite, "observation_update: problem %d: a camera vector or depth constant is not finite", i);
        SIMQ_REQUIRE(p.has_receptacle == 0 || p.has_receptacle == 1, "observation_update: problem %d: has_receptacle = %d (0 or 1)", i,
                     p.has_receptacle);
        const uintptr_t a = (uintptr_t)(d_overhead + p.overhead_offset), b = (uintptr_t)(d_occupancy + p.occupancy_offset);
        spans.push_back({a, a + 4 * (uintptr_t)cells, i});
        spans.push_back({b, b + (uintptr_t)cells, i});
        const int64_t tiles = (int64_t)((p.rows + kTileRows - 1) / kTileRows) * ((p.cols + kTileCols - 1) / kTileCols);
        max_tiles = std::max(max_tiles, (int)tiles);
    }
    const size_t clash = first_overlap(spans);
    SIMQ_REQUIRE(clash == 0,
                 "observation_update: two maps of one launch share memory at address %p (every problem needs an overhead map and an "
                 "occupancy map of its own: the order of two updates of one map matters)", (void*)spans[clash].lo);
    const Buffer others[] = {
        {"d_frames", d_frames, frame_words * 4, false}, {"d_problems", d_problems, prob_bytes, true}, {"d_status", d_status, status_bytes, true}};
    for (const Span& s : spans)
        for (const Buffer& o : others)
            SIMQ_REQUIRE(!overlaps((const void*)s.lo, (int64_t)(s.hi - s.lo), o.p, o.bytes), "observation_update: a map overlaps %s", o.name);
    int a = 0, b = 0;
    SIMQ_REQUIRE(!first_conflict(others, 3, &a, &b), "observation_update: %s overlaps %s", others[a].name, others[b].name);
    const int64_t blocks = (int64_t)n * max_tiles;
    SIMQ_REQUIRE(blocks <= 0x7fffffffLL, "observation_update: %d problems of up to %d tiles take %lld workgroups (at most 2^31 - 1)", n,
                 max_tiles, (long long)blocks);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const HostBlock block = {problems, (size_t)prob_bytes};
    SIMQ_CHECK_HIP(upload_descriptors(d_problems, &block, 1, nullptr, s));
    observation_maps_kernel<<<(unsigned)blocks, kThreads, 0, s>>>(static_cast<const uint32_t*>(d_frames), frame_words, d_problems, max_tiles,
                                                                  d_overhead, overhead_floats, d_occupancy, occupancy_bytes, d_status);
    SIMQ_CHECK_LAUNCH();
    note_launch("observation_maps");
    return 0;
}

// ---- ordered frame sequences: several frames per pair of maps in one launch -----------------------------------------------------------
// What K successive launches of the kernel above leave in one pair of maps, computed in one: an overhead pixel holds the seg the last
// frame that reached it gives it by that frame's own rule, an occupancy byte is the OR over the frames.  The key gains the frame's
// position in its sequence above the height, [position + 1 : 10][order-preserving z : 32][frame index : 22]: one maximum still decides,
// a later frame beats any height of an earlier one, and inside a frame nothing changes.  SIMQ_OBSERVATION_MAX_POINTS is 2^22, so the
// index needs 22 bits and 10 are left: position + 1 in 1 .. 1023 (key 0 stays the untouched pixel), the cap of a sequence.
//
// One workgroup per 32 x 256 tile of a SEQUENCE's maps streams the points of all its frames, so it sees every non-finite point of the
// sequence itself.  A frame with such a point must count for nothing, but its earlier points may have scattered already: the frame is
// flagged in LDS and, in that rare case, the tile is cleared and the scatter repeated without the flagged frames.  The second attempt
// cannot raise a flag -- every point of every other frame was seen finite in the first -- so there are at most two.
namespace simq {

namespace {

constexpr int kMaxSequence = SIMQ_OBSERVATION_MAX_SEQUENCE;
constexpr int kIndexBits = 22, kPositionShift = 32 + kIndexBits;
static_assert(kMaxPoints == (1 << kIndexBits), "the frame index of a key has 22 bits");
static_assert(kMaxSequence + 1 == (1 << (64 - kPositionShift)), "position + 1 of a key has what is left of 64 bits");

__host__ __device__ __forceinline__ bool same_maps(const simq_observation_problem& a, const simq_observation_problem& b) {
    return a.overhead_offset == b.overhead_offset && a.occupancy_offset == b.occupancy_offset && a.rows == b.rows && a.cols == b.cols;
}

__global__ void __launch_bounds__(kThreads) observation_sequences_kernel(const uint32_t* __restrict__ frames, int64_t frame_words,
                                                                         const simq_observation_problem* __restrict__ probs, int n_frames,
                                                                         const int32_t* __restrict__ begin, int max_tiles, float* overhead,
                                                                         int64_t overhead_floats, uint8_t* occupancy, int64_t occupancy_bytes,
                                                                         int32_t* __restrict__ status) {
    __shared__ unsigned long long keys[kTilePixels];
    __shared__ uint8_t occupied[kTilePixels];
    __shared__ uint8_t frame_bad[kMaxSequence + 1];
    __shared__ int bad_descriptor, raised;
    const int tid = threadIdx.x;
    const int s = blockIdx.x / max_tiles, t = blockIdx.x - s * max_tiles;
    const int f0 = begin[s], f1 = begin[s + 1];                                       // (uniform over the workgroup)
    if (f0 < 0 || f1 <= f0 || f1 > n_frames) return;                                  // (the host validated already: the table names no frame of the launch)
    const int count = f1 - f0;
    if (tid == 0) bad_descriptor = raised = 0;
    for (int k = tid; k < kTilePixels; k += kThreads) {
        keys[k] = 0ull;
        occupied[k] = 0;
    }
    frame_bad[tid] = 0;
    __syncthreads();
    const simq_observation_problem first = probs[f0];
    bool ok = count <= kMaxSequence;
    for (int f = tid; f < count && ok; f += kThreads)
        ok = descriptor_ok(probs[f0 + f], frame_words, overhead_floats, occupancy_bytes) && same_maps(probs[f0 + f], first);
    if (!ok) bad_descriptor = 1;
    __syncthreads();
    if (bad_descriptor != 0) {                                                        // (nothing of the sequence is read or written)
        if (t == 0)
            for (int f = tid; f < count; f += kThreads) status[f0 + f] = 2;
        return;
    }
    const int tiles_j = (first.cols + kTileCols - 1) / kTileCols, tiles_i = (first.rows + kTileRows - 1) / kTileRows;
    if (t >= tiles_i * tiles_j) return;                                               // (the grid is sized by the launch's largest map)
    const int ti = t / tiles_j, tj = t - ti * tiles_j;
    const int i0 = ti * kTileRows, j0 = tj * kTileCols;
    const float half_rows = (float)first.rows * 0.5f, half_cols = (float)first.cols * 0.5f;

    for (int attempt = 0; attempt < 2; ++attempt) {
        for (int f = 0; f < count; ++f) {
            if (attempt != 0 && frame_bad[f] != 0) continue;
            const simq_observation_problem pr = probs[f0 + f];                        // (uniform over the workgroup)
            const float* depth = reinterpret_cast<const float*>(frames + pr.depth_offset);
            const int32_t* ids = reinterpret_cast<const int32_t*>(frames + pr.ids_offset);
            const float* px = reinterpret_cast<const float*>(frames + pr.px_offset);
            const float* py = reinterpret_cast<const float*>(frames + pr.py_offset);
            const int points = pr.height * pr.width;
            const unsigned long long above = (unsigned long long)(f + 1) << kPositionShift;
            bool bad = false;
            for (int k = tid; k < points; k += kThreads) {
                const int h = k / pr.width, w = k - h * pr.width;
                float x, y, z;
                project(pr, depth[k], px[w], py[h], x, y, z);
                if (!(isfinite(x) && isfinite(y) && isfinite(z))) {
                    bad = true;
                    continue;
                }
                const int li = pixel_index(half_rows, y, true, pr.rows) - i0, lj = pixel_index(half_cols, x, false, pr.cols) - j0;
                if (li < 0 || li >= kTileRows || lj < 0 || lj >= kTileCols) continue;
                const int raw = ids[k];
                uint32_t zb = z == 0.f ? 0u : __float_as_uint(z);                     // -0 and +0 are one height
                zb = (zb & 0x80000000u) ? ~zb : (zb | 0x80000000u);
                atomicMax(&keys[li * kTileCols + lj], above | ((unsigned long long)zb << kIndexBits) | (unsigned)k);
                if (seg_value(pr, raw) == 0.25f) occupied[li * kTileCols + lj] = 1;   // (2/8: the obstacle term and no other)
            }
            if (bad) {
                frame_bad[f] = 1;
                raised = 1;
            }
        }
        __syncthreads();
        if (raised == 0) break;                                                       // (uniform: read between two barriers)
        __syncthreads();
        if (attempt != 0) break;                                                      // (cannot happen: see above)
        if (tid == 0) raised = 0;
        for (int k = tid; k < kTilePixels; k += kThreads) {
            keys[k] = 0ull;
            occupied[k] = 0;
        }
        __syncthreads();
    }
    if (t == 0)
        for (int f = tid; f < count; f += kThreads) status[f0 + f] = frame_bad[f] != 0 ? 1 : 0;

    float* o_map = overhead + first.overhead_offset;
    uint8_t* o_occ = occupancy + first.occupancy_offset;
    for (int k = tid; k < kTilePixels; k += kThreads) {
        const int li = k / kTileCols, lj = k - li * kTileCols;
        const int gi = i0 + li, gj = j0 + lj;
        if (gi >= first.rows || gj >= first.cols) continue;
        const unsigned long long key = keys[k];
        const int64_t cell = (int64_t)gi * first.cols + gj;
        if (key != 0ull) {
            const simq_observation_problem& won = probs[f0 + (int)(key >> kPositionShift) - 1];
            const int32_t* ids = reinterpret_cast<const int32_t*>(frames + won.ids_offset);
            o_map[cell] = seg_value(won, ids[(uint32_t)key & ((1u << kIndexBits) - 1)]);
        }
        if (occupied[k]) o_occ[cell] = 1;
    }
}

// what simq_observation_update checks of one descriptor, for frame i of a sequences call
int check_frame(const simq_observation_problem& p, int i, int64_t frame_words, int64_t overhead_floats, int64_t occupancy_bytes) {
    SIMQ_REQUIRE(p.height >= 1 && p.width >= 1 && (int64_t)p.height * p.width <= kMaxPoints,
                 "observation_update_sequences: frame %d: a frame of %d x %d (height, width >= 1, at most %d points)", i, p.height, p.width,
                 kMaxPoints);
    SIMQ_REQUIRE(p.rows >= 1 && p.cols >= 1 && p.rows < kMaxSide && p.cols < kMaxSide && (int64_t)p.rows * p.cols < kMaxCells,
                 "observation_update_sequences: frame %d: maps of %d x %d (rows, cols in [1, 2^24), rows * cols < 2^28)", i, p.rows, p.cols);
    const int64_t points = (int64_t)p.height * p.width, cells = (int64_t)p.rows * p.cols;
    SIMQ_REQUIRE(fits(p.depth_offset, points, frame_words),
                 "observation_update_sequences: frame %d: depth words [%lld, %lld) outside the %lld of d_frames", i, (long long)p.depth_offset,
                 (long long)(p.depth_offset + points), (long long)frame_words);
    SIMQ_REQUIRE(fits(p.ids_offset, points, frame_words),
                 "observation_update_sequences: frame %d: id words [%lld, %lld) outside the %lld of d_frames", i, (long long)p.ids_offset,
                 (long long)(p.ids_offset + points), (long long)frame_words);
    SIMQ_REQUIRE(fits(p.px_offset, p.width, frame_words) && fits(p.py_offset, p.height, frame_words),
                 "observation_update_sequences: frame %d: px words [%lld, +%d) or py words [%lld, +%d) outside the %lld of d_frames", i,
                 (long long)p.px_offset, p.width, (long long)p.py_offset, p.height, (long long)frame_words);
    SIMQ_REQUIRE(fits(p.overhead_offset, cells, overhead_floats),
                 "observation_update_sequences: frame %d: overhead floats [%lld, %lld) outside the %lld of d_overhead", i,
                 (long long)p.overhead_offset, (long long)(p.overhead_offset + cells), (long long)overhead_floats);
    SIMQ_REQUIRE(fits(p.occupancy_offset, cells, occupancy_bytes),
                 "observation_update_sequences: frame %d: occupancy bytes [%lld, %lld) outside the %lld of d_occupancy", i,
                 (long long)p.occupancy_offset, (long long)(p.occupancy_offset + cells), (long long)occupancy_bytes);
    bool finite = std::isfinite(p.far_near) && std::isfinite(p.far) && std::isfinite(p.far_minus_near);
    for (int c = 0; c < 3; ++c)
        finite = finite && std::isfinite(p.cam[c]) && std::isfinite(p.principal[c]) && std::isfinite(p.right[c]) && std::isfinite(p.up[c]);
    SIMQ_REQUIRE(finite, "observation_update_sequences: frame %d: a camera vector or depth constant is not finite", i);
    SIMQ_REQUIRE(p.has_receptacle == 0 || p.has_receptacle == 1, "observation_update_sequences: frame %d: has_receptacle = %d (0 or 1)", i,
                 p.has_receptacle);
    return 0;
}

}  // namespace

}  // namespace simq

extern "C" int simq_observation_update_sequences(const void* d_frames, int64_t frame_words, const simq_observation_problem* frames,
                                                 int n_frames, const int32_t* begin, int n_sequences, simq_observation_problem* d_problems,
                                                 int32_t* d_begin, float* d_overhead, int64_t overhead_floats, uint8_t* d_occupancy,
                                                 int64_t occupancy_bytes, int32_t* d_status, void* stream) {
    SIMQ_REQUIRE(d_frames && frames && begin && d_problems && d_begin && d_overhead && d_occupancy && d_status,
                 "observation_update_sequences: NULL pointer");
    SIMQ_REQUIRE(n_frames >= 1 && n_frames <= (1 << 20), "observation_update_sequences: n_frames = %d (1 .. 2^20 frames)", n_frames);
    SIMQ_REQUIRE(n_sequences >= 1 && n_sequences <= n_frames, "observation_update_sequences: n_sequences = %d (1 .. n_frames = %d: no sequence is empty)",
                 n_sequences, n_frames);
    SIMQ_REQUIRE(frame_words >= 0 && overhead_floats >= 0 && occupancy_bytes >= 0 && frame_words < (1LL << 40) &&
                     overhead_floats < (1LL << 40) && occupancy_bytes < (1LL << 40),
                 "observation_update_sequences: buffer sizes %lld, %lld, %lld (each in [0, 2^40))", (long long)frame_words,
                 (long long)overhead_floats, (long long)occupancy_bytes);
    SIMQ_REQUIRE(((uintptr_t)d_frames & 3) == 0 && ((uintptr_t)d_overhead & 3) == 0 && ((uintptr_t)d_problems & 7) == 0 &&
                     ((uintptr_t)d_begin & 3) == 0 && ((uintptr_t)d_status & 3) == 0,
                 "observation_update_sequences: d_problems must be 8-byte, d_frames, d_begin, d_overhead and d_status 4-byte aligned");
    SIMQ_REQUIRE(begin[0] == 0 && begin[n_sequences] == n_frames,
                 "observation_update_sequences: begin[0] = %d and begin[%d] = %d (begin rises from 0 to n_frames = %d)", begin[0], n_sequences,
                 begin[n_sequences], n_frames);
    for (int s = 0; s < n_sequences; ++s) {
        const int64_t count = (int64_t)begin[s + 1] - begin[s];
        SIMQ_REQUIRE(count >= 1, "observation_update_sequences: sequence %d: begin goes from %d to %d (begin rises: every sequence has a frame)", s,
                     begin[s], begin[s + 1]);
        SIMQ_REQUIRE(count <= kMaxSequence && begin[s + 1] <= n_frames,
                     "observation_update_sequences: sequence %d: frames %d .. %d (at most %d frames per sequence, of n_frames = %d)", s, begin[s],
                     begin[s + 1] - 1, kMaxSequence, n_frames);
    }
    for (int i = 0; i < n_frames; ++i)
        if (check_frame(frames[i], i, frame_words, overhead_floats, occupancy_bytes) != 0) return -1;
    const int64_t prob_bytes = (int64_t)sizeof(simq_observation_problem) * n_frames, begin_bytes = 4LL * (n_sequences + 1), status_bytes = 4LL * n_frames;
    std::vector<Span> spans;                                                          // the bytes this launch may write, as addresses
    spans.reserve(2 * (size_t)n_sequences);
    int max_tiles = 1;
    for (int s = 0; s < n_sequences; ++s) {
        const simq_observation_problem& p = frames[begin[s]];
        for (int i = begin[s] + 1; i < begin[s + 1]; ++i) {
            const simq_observation_problem& q = frames[i];
            SIMQ_REQUIRE(q.overhead_offset == p.overhead_offset,
                         "observation_update_sequences: sequence %d: frame %d names overhead_offset %lld, frame %d names %lld (the frames of a sequence update one pair of maps)",
                         s, i, (long long)q.overhead_offset, begin[s], (long long)p.overhead_offset);
            SIMQ_REQUIRE(q.occupancy_offset == p.occupancy_offset,
                         "observation_update_sequences: sequence %d: frame %d names occupancy_offset %lld, frame %d names %lld (the frames of a sequence update one pair of maps)",
                         s, i, (long long)q.occupancy_offset, begin[s], (long long)p.occupancy_offset);
            SIMQ_REQUIRE(q.rows == p.rows, "observation_update_sequences: sequence %d: frame %d names rows %d, frame %d names %d (the frames of a sequence update one pair of maps)",
                         s, i, q.rows, begin[s], p.rows);
            SIMQ_REQUIRE(q.cols == p.cols, "observation_update_sequences: sequence %d: frame %d names cols %d, frame %d names %d (the frames of a sequence update one pair of maps)",
                         s, i, q.cols, begin[s], p.cols);
        }
        const int64_t cells = (int64_t)p.rows * p.cols;
        const uintptr_t a = (uintptr_t)(d_overhead + p.overhead_offset), b = (uintptr_t)(d_occupancy + p.occupancy_offset);
        spans.push_back({a, a + 4 * (uintptr_t)cells, s});
        spans.push_back({b, b + (uintptr_t)cells, s});
        const int64_t tiles = (int64_t)((p.rows + kTileRows - 1) / kTileRows) * ((p.cols + kTileCols - 1) / kTileCols);
        max_tiles = std::max(max_tiles, (int)tiles);
    }
    const size_t clash = first_overlap(spans);
    SIMQ_REQUIRE(clash == 0,
                 "observation_update_sequences: two maps of one launch share memory at address %p (every sequence needs an overhead map and an "
                 "occupancy map of its own: the frames of one map go into one sequence, in order)", (void*)spans[clash].lo);
    const Buffer others[] = {{"d_frames", d_frames, frame_words * 4, false},
                             {"d_problems", d_problems, prob_bytes, true},
                             {"d_begin", d_begin, begin_bytes, true},
                             {"d_status", d_status, status_bytes, true}};
    for (const Span& sp : spans)
        for (const Buffer& o : others)
            SIMQ_REQUIRE(!overlaps((const void*)sp.lo, (int64_t)(sp.hi - sp.lo), o.p, o.bytes), "observation_update_sequences: a map overlaps %s",
                         o.name);
    int a = 0, b = 0;
    SIMQ_REQUIRE(!first_conflict(others, 4, &a, &b), "observation_update_sequences: %s overlaps %s", others[a].name, others[b].name);
    const int64_t blocks = (int64_t)n_sequences * max_tiles;
    SIMQ_REQUIRE(blocks <= 0x7fffffffLL, "observation_update_sequences: %d sequences of up to %d tiles take %lld workgroups (at most 2^31 - 1)",
                 n_sequences, max_tiles, (long long)blocks);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const HostBlock desc = {frames, (size_t)prob_bytes}, table = {begin, (size_t)begin_bytes};
    SIMQ_CHECK_HIP(upload_descriptors(d_problems, &desc, 1, nullptr, st));
    SIMQ_CHECK_HIP(upload_descriptors(d_begin, &table, 1, nullptr, st));
    observation_sequences_kernel<<<(unsigned)blocks, kThreads, 0, st>>>(static_cast<const uint32_t*>(d_frames), frame_words, d_problems, n_frames,
                                                                        d_begin, max_tiles, d_overhead, overhead_floats, d_occupancy,
                                                                        occupancy_bytes, d_status);
    SIMQ_CHECK_LAUNCH();
    note_launch("observation_sequences");
    return 0;
}
