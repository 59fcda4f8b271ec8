// libsimq: batched global intention / history maps -- the line-drawing stage of Mapper.get_state
//   intention_maps_kernel    _create_global_intention_or_history_map (all five encodings)          envs.py:2301-2346
//                            the per-robot spatial maps of _get_intention_channels                 envs.py:2360-2366
//
// Exactness.  Every write of the reference is a store of one non-negative constant or a maximum with a value clipped to [0, 1], and a
// skimage.draw.line segment visits no pixel twice: the map is the maximum, per pixel, over every point of every segment, whatever the
// order.  Non-negative floats order as their bit patterns, so the maximum is an unsigned integer maximum in LDS (ds_max_u32), exact.
// Point i of the line (r0, c0) -> (r1, c1), n = max(|dr|, |dc|), m = min(|dr|, |dc|), is i steps along the major axis and
// (2 * m * i + n) / (2 * n) steps (integer division) along the minor one -- the closed form of the sequential algorithm (the rows are
// the major axis when |dr| > |dc|).  A ramp value is np.linspace's float64 sequence i * step + start, product and sum rounded
// separately (compiled with contraction off: the ISA holds v_mul_f64 / v_add_f64 there and no fused form), the last point `stop`
// itself, clipped to [0, 1] and rounded to fp32.  Dilation with the disk is the maximum over the disk's offsets; pixels outside the map
// are absent, which on a non-negative map is what scipy's reflecting border gives too, and they read as the identity 0 here.
//
// Shape.  One workgroup of 256 lanes per 32 x 256 tile of one problem's map.  It zeroes the tile with a halo of the disk radius in LDS
// (at most 48 x 272 words = 51 KB), walks the problem's segments with one lane per point (a segment whose bounding box misses the halo
// is skipped), keeps the points inside the halo with the LDS maximum, then every lane dilates one column of the tile out of LDS and
// writes it: consecutive lanes write consecutive floats of a row.  Every pixel of the map is written by exactly one workgroup, so the
// caller zero-fills nothing.
#include "batch_abi.h"
#include "../../include/simq.h"

#include <cmath>

namespace simq {

namespace {

constexpr int kTileRows = 32;
constexpr int kTileCols = 256;
constexpr int kThreads = kTileCols;
constexpr int kMaxRadius = SIMQ_INTENTION_MAX_RADIUS;             // 8
constexpr int kHaloCols = kTileCols + 2 * kMaxRadius;             // 272: the LDS row stride, whatever the radius
constexpr int kHaloWords = (kTileRows + 2 * kMaxRadius) * kHaloCols;

struct Desc {                                     // the packed device copy of one call's descriptors
    const simq_intention_segment* segs;
    const simq_intention_problem* probs;
    int rows, cols, radius, tiles_i, tiles_j;
};

// the fp32 bit pattern of ramp point i of `num`: (float)clip(linspace(start, stop, num)[i], 0, 1)
__device__ __forceinline__ unsigned ramp_bits(const simq_intention_segment& s, int i, int num) {
    // hipcc contracts a * b + c into v_fma_f64 by default; numpy rounds the product and the sum separately
#pragma clang fp contract(off)
    const double prod = (double)i * s.step;
    double y = prod + s.start;
    if (num > 1 && i == num - 1) y = s.stop;
    float v = (float)y;                           // (rounding is monotone: clipping after it equals clipping before it)
    v = v > 0.f ? v : 0.f;                        // also -0 -> +0, whose bit pattern would be the largest unsigned
    v = v < 1.f ? v : 1.f;
    return __float_as_uint(v);
}

__global__ void __launch_bounds__(kThreads) intention_maps_kernel(Desc d, float* __restrict__ out) {
    __shared__ unsigned halo[kHaloWords];
    __shared__ int any_point;
    const int tid = threadIdx.x;
    const int tiles = d.tiles_i * d.tiles_j;
    const int p = blockIdx.x / tiles, t = blockIdx.x - p * tiles;
    const int ti = t / d.tiles_j, tj = t - ti * d.tiles_j;
    const int R = d.radius;
    const int hi0 = ti * kTileRows - R, hj0 = tj * kTileCols - R;             // the map pixel of halo word (0, 0)
    const int hrows = kTileRows + 2 * R, hcols = kTileCols + 2 * R;
    const simq_intention_problem pr = d.probs[p];

    for (int k = tid; k < hrows * kHaloCols; k += kThreads) halo[k] = 0u;
    if (tid == 0) any_point = 0;
    __syncthreads();

    for (int k = 0; k < pr.seg_count; ++k) {
        const simq_intention_segment s = d.segs[pr.seg_begin + k];            // (uniform over the workgroup)
        if (max(s.r0, s.r1) < hi0 || min(s.r0, s.r1) >= hi0 + hrows || max(s.c0, s.c1) < hj0 || min(s.c0, s.c1) >= hj0 + hcols) continue;
        const int dr = s.r1 - s.r0, dc = s.c1 - s.c0;
        const int adr = abs(dr), adc = abs(dc);
        const bool steep = adr > adc;
        const int n = steep ? adr : adc, m = steep ? adc : adr;
        const int sr = dr > 0 ? 1 : -1, sc = dc > 0 ? 1 : -1;
        const int num = n + 1;
        const int drawn = num - (s.drop_last ? 1 : 0);
        const unsigned stored = __float_as_uint(s.value);
        for (int i = tid; i < drawn; i += kThreads) {
            int minor = 0;
            if (n > 0) minor = n < 32768 ? (int)((2u * (unsigned)m * (unsigned)i + (unsigned)n) / (2u * (unsigned)n))
                                         : (int)((2ull * (unsigned)m * (unsigned)i + (unsigned)n) / (2ull * (unsigned)n));
            const int r = s.r0 + sr * (steep ? i : minor), c = s.c0 + sc * (steep ? minor : i);
            const int li = r - hi0, lj = c - hj0;
            if (li < 0 || li >= hrows || lj < 0 || lj >= hcols) continue;
            atomicMax(&halo[li * kHaloCols + lj], s.mode == SIMQ_INTENTION_RAMP ? ramp_bits(s, i, num) : stored);
            any_point = 1;
        }
    }
    __syncthreads();

    const int gj = tj * kTileCols + tid;
    if (gj >= d.cols) return;
    float* o = out + ((int64_t)p * d.rows) * d.cols + gj;
    const bool draw = any_point != 0;
    const int R2 = R * R;
    for (int li = 0; li < kTileRows; ++li) {
        const int gi = ti * kTileRows + li;
        if (gi >= d.rows) break;
        unsigned v = 0u;
        if (draw) {
            for (int di = -R; di <= R; ++di) {
                const unsigned* row = &halo[(li + R + di) * kHaloCols + tid + R];
                for (int dj = -R; dj <= R; ++dj)
                    if (di * di + dj * dj <= R2) v = max(v, row[dj]);
            }
        }
        o[(int64_t)gi * d.cols] = __uint_as_float(v);
    }
}

}  // namespace

}  // namespace simq

using namespace simq;

extern "C" int64_t simq_intention_desc_bytes(int n_segments, int n) {
    if (n_segments < 0 || n < 0) return -1;
    return (int64_t)sizeof(simq_intention_segment) * n_segments + (int64_t)sizeof(simq_intention_problem) * n;
}

extern "C" int simq_intention_maps(const simq_intention_segment* segments, int n_segments, const simq_intention_problem* problems, int n,
                                   int rows, int cols, int radius, void* d_desc, int64_t desc_bytes, float* d_out, int64_t out_floats,
                                   void* stream) {
    SIMQ_REQUIRE(problems && d_desc && d_out, "intention_maps: NULL pointer");
    SIMQ_REQUIRE(n >= 1 && n <= (1 << 20), "intention_maps: n = %d (1 .. 2^20 problems)", n);
    SIMQ_REQUIRE(n_segments >= 0 && n_segments <= (1 << 24) && (n_segments == 0 || segments), "intention_maps: n_segments = %d with segments %s",
                 n_segments, segments ? "given" : "NULL");
    SIMQ_REQUIRE(rows >= 1 && cols >= 1 && (int64_t)rows * cols < (1 << 28), "intention_maps: maps of %d x %d (rows, cols >= 1, rows * cols < 2^28)",
                 rows, cols);
    SIMQ_REQUIRE(radius >= 0 && radius <= kMaxRadius, "intention_maps: radius = %d (0 .. %d: line thickness 1 .. %d)", radius, kMaxRadius,
                 kMaxRadius + 1);
    const int tiles_i = (rows + kTileRows - 1) / kTileRows, tiles_j = (cols + kTileCols - 1) / kTileCols;
    const int64_t blocks = (int64_t)n * tiles_i * tiles_j;
    SIMQ_REQUIRE(blocks <= 0x7fffffffLL, "intention_maps: %d maps of %d x %d take %lld workgroups (at most 2^31 - 1)", n, rows, cols,
                 (long long)blocks);
    SIMQ_REQUIRE(((uintptr_t)d_desc & 7) == 0 && ((uintptr_t)d_out & 3) == 0, "intention_maps: d_desc must be 8-byte and d_out 4-byte aligned");
    const int64_t need_desc = simq_intention_desc_bytes(n_segments, n);
    SIMQ_REQUIRE(desc_bytes >= need_desc, "intention_maps: d_desc holds %lld bytes, the descriptors take %lld", (long long)desc_bytes,
                 (long long)need_desc);
    const int64_t need_out = (int64_t)n * rows * cols;
    SIMQ_REQUIRE(out_floats >= need_out, "intention_maps: d_out holds %lld floats, %d maps of %d x %d take %lld", (long long)out_floats, n, rows,
                 cols, (long long)need_out);
    SIMQ_REQUIRE(!overlaps(d_out, need_out * 4, d_desc, need_desc), "intention_maps: d_out overlaps d_desc");
    for (int k = 0; k < n_segments; ++k) {
        const simq_intention_segment& s = segments[k];
        SIMQ_REQUIRE(s.r0 >= 0 && s.r0 < rows && s.r1 >= 0 && s.r1 < rows && s.c0 >= 0 && s.c0 < cols && s.c1 >= 0 && s.c1 < cols,
                     "intention_maps: segment %d: (%d, %d) -> (%d, %d) leaves the %d x %d map", k, s.r0, s.c0, s.r1, s.c1, rows, cols);
        SIMQ_REQUIRE(s.mode == SIMQ_INTENTION_STORE || s.mode == SIMQ_INTENTION_RAMP, "intention_maps: segment %d: mode %d", k, s.mode);
        SIMQ_REQUIRE(s.drop_last == 0 || s.drop_last == 1, "intention_maps: segment %d: drop_last = %d (0 or 1)", k, s.drop_last);
        if (s.mode == SIMQ_INTENTION_RAMP)
            SIMQ_REQUIRE(std::isfinite(s.start) && std::isfinite(s.stop) && std::isfinite(s.step),
                         "intention_maps: segment %d: start / stop / step is not finite", k);
        else
            SIMQ_REQUIRE(std::isfinite(s.value) && s.value >= 0.f && !std::signbit(s.value),
                         "intention_maps: segment %d: stored value %g (finite, >= 0 and not -0: the maximum is taken on bit patterns)", k,
                         (double)s.value);
    }
    for (int i = 0; i < n; ++i) {
        const simq_intention_problem& p = problems[i];
        SIMQ_REQUIRE(p.seg_count >= 0 && p.seg_begin >= 0 && (int64_t)p.seg_begin + p.seg_count <= n_segments,
                     "intention_maps: problem %d: segments [%d, %d + %d) outside the %d given", i, p.seg_begin, p.seg_begin, p.seg_count,
                     n_segments);
    }

    const HostBlock parts[2] = {{segments, sizeof(simq_intention_segment) * (size_t)n_segments},
                                {problems, sizeof(simq_intention_problem) * (size_t)n}};
    const char* at[2];
    hipStream_t s = static_cast<hipStream_t>(stream);
    SIMQ_CHECK_HIP(upload_descriptors(d_desc, parts, 2, at, s));
    Desc d;
    d.segs = reinterpret_cast<const simq_intention_segment*>(at[0]);
    d.probs = reinterpret_cast<const simq_intention_problem*>(at[1]);
    d.rows = rows;
    d.cols = cols;
    d.radius = radius;
    d.tiles_i = tiles_i;
    d.tiles_j = tiles_j;
    intention_maps_kernel<<<(unsigned)blocks, kThreads, 0, s>>>(d, d_out);
    SIMQ_CHECK_LAUNCH();
    note_launch("intention_maps");
    return 0;
}
