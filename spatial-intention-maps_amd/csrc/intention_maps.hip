// libsimq: batched global intention / history maps -- the line-drawing stage of Mapper.get_state
//   intention_maps_kernel    _create_global_intention_or_history_map (all five encodings)          envs.py:2301-2346
//                            the per-robot spatial maps of _get_intention_channels                 envs.py:2360-2366
//   intention_maps_shapes_kernel   the same maps for problems of several room shapes and line thicknesses in one launch
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
//
// Shapes.  simq_intention_maps_shapes draws problems that each have their own rows x cols, radius and place in d_out, in one launch:
// intention_maps_shapes_kernel differs from intention_maps_kernel only in how a workgroup finds its (problem, tile) -- a binary search
// over the prefix of the problems' tile counts, which travels in d_desc behind the segments and problems -- and in where it reads the
// shape and the radius.  Both kernels then call draw_tile, the one statement of the tile body: ramp_bits, the contraction pragma and the
// integer line rule exist once, no arithmetic is added, and the exactness argument above holds for either entry unchanged.  The LDS row
// stride is kHaloCols for every radius, so problems of different radii share a launch at no cost.
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

struct ShapedDesc {                               // ... and of a call whose problems carry their own shape, place and radius
    const simq_intention_segment* segs;
    const simq_intention_shaped_problem* probs;
    const int32_t* tile_begin;                    // [n + 1]: the first workgroup of every problem, then the grid size
    int n;
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

// Tile (ti, tj) of one rows x cols map at `map`, drawn from segs[seg_begin .. seg_begin + seg_count) and dilated with the disk of
// radius R: the whole body of both kernels.  Every argument is uniform over the workgroup; halo and any_point are its LDS.
__device__ __forceinline__ void draw_tile(unsigned* halo, int* any_point, const simq_intention_segment* __restrict__ segs, int seg_begin,
                                          int seg_count, int rows, int cols, int R, int ti, int tj, float* __restrict__ map) {
    const int tid = threadIdx.x;
    const int hi0 = ti * kTileRows - R, hj0 = tj * kTileCols - R;             // the map pixel of halo word (0, 0)
    const int hrows = kTileRows + 2 * R, hcols = kTileCols + 2 * R;

    for (int k = tid; k < hrows * kHaloCols; k += kThreads) halo[k] = 0u;
    if (tid == 0) *any_point = 0;
    __syncthreads();

    for (int k = 0; k < seg_count; ++k) {
        const simq_intention_segment s = segs[seg_begin + k];                 // (uniform over the workgroup)
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
            *any_point = 1;
        }
    }
    __syncthreads();

    const int gj = tj * kTileCols + tid;
    if (gj >= cols) return;
    float* o = map + gj;
    const bool draw = *any_point != 0;
    const int R2 = R * R;
    for (int li = 0; li < kTileRows; ++li) {
        const int gi = ti * kTileRows + li;
        if (gi >= rows) break;
        unsigned v = 0u;
        if (draw) {
            for (int di = -R; di <= R; ++di) {
                const unsigned* row = &halo[(li + R + di) * kHaloCols + tid + R];
                for (int dj = -R; dj <= R; ++dj)
                    if (di * di + dj * dj <= R2) v = max(v, row[dj]);
            }
        }
        o[(int64_t)gi * cols] = __uint_as_float(v);
    }
}

__global__ void __launch_bounds__(kThreads) intention_maps_kernel(Desc d, float* __restrict__ out) {
    __shared__ unsigned halo[kHaloWords];
    __shared__ int any_point;
    const int tiles = d.tiles_i * d.tiles_j;
    const int p = blockIdx.x / tiles, t = blockIdx.x - p * tiles;
    const int ti = t / d.tiles_j, tj = t - ti * d.tiles_j;
    const simq_intention_problem pr = d.probs[p];
    draw_tile(halo, &any_point, d.segs, pr.seg_begin, pr.seg_count, d.rows, d.cols, d.radius, ti, tj, out + ((int64_t)p * d.rows) * d.cols);
}

// Workgroup b belongs to the problem p with tile_begin[p] <= b < tile_begin[p + 1] (every problem has a tile, so the table rises
// strictly): a binary search on blockIdx.x, uniform over the workgroup -- scalar loads, at most 20 steps for n <= 2^20.
__global__ void __launch_bounds__(kThreads) intention_maps_shapes_kernel(ShapedDesc d, float* __restrict__ out) {
    __shared__ unsigned halo[kHaloWords];
    __shared__ int any_point;
    const int b = (int)blockIdx.x;
    int lo = 0, hi = d.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (d.tile_begin[mid] <= b) lo = mid; else hi = mid;
    }
    const simq_intention_shaped_problem pr = d.probs[lo];
    const int t = b - d.tile_begin[lo];
    const int tiles_j = (pr.cols + kTileCols - 1) / kTileCols;
    const int ti = t / tiles_j, tj = t - ti * tiles_j;
    draw_tile(halo, &any_point, d.segs, pr.seg_begin, pr.seg_count, pr.rows, pr.cols, pr.radius, ti, tj, out + pr.out_offset);
}

}  // namespace

}  // namespace simq

using namespace simq;

// what both entries ask of segment k whatever map it is drawn into: its mode, its flag, finite doubles, the stored-value rule
static int check_segment_values(const char* entry, const simq_intention_segment& s, int k) {
    SIMQ_REQUIRE(s.mode == SIMQ_INTENTION_STORE || s.mode == SIMQ_INTENTION_RAMP, "%s: segment %d: mode %d", entry, k, s.mode);
    SIMQ_REQUIRE(s.drop_last == 0 || s.drop_last == 1, "%s: segment %d: drop_last = %d (0 or 1)", entry, k, s.drop_last);
    if (s.mode == SIMQ_INTENTION_RAMP)
        SIMQ_REQUIRE(std::isfinite(s.start) && std::isfinite(s.stop) && std::isfinite(s.step), "%s: segment %d: start / stop / step is not finite",
                     entry, k);
    else
        SIMQ_REQUIRE(std::isfinite(s.value) && s.value >= 0.f && !std::signbit(s.value),
                     "%s: segment %d: stored value %g (finite, >= 0 and not -0: the maximum is taken on bit patterns)", entry, k, (double)s.value);
    return 0;
}

// the first segment of [begin, end) that no earlier call has handed out, by path halving over `next` (next[k] == k: not handed out yet)
static int next_unclaimed(std::vector<int>& next, int k) {
    while (next[k] != k) k = next[k] = next[next[k]];
    return k;
}

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
        if (check_segment_values("intention_maps", s, k)) return -1;
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

// ---- problems of several shapes, radii and places in one launch ---------------------------------------------------------------------

extern "C" int64_t simq_intention_shapes_desc_bytes(int n_segments, int n) {
    if (n_segments < 0 || n < 0) return -1;
    const int64_t prefix = ((int64_t)sizeof(int32_t) * ((int64_t)n + 1) + 7) & ~(int64_t)7;         // tile_begin[n + 1], padded to 8 bytes
    return (int64_t)sizeof(simq_intention_segment) * n_segments + (int64_t)sizeof(simq_intention_shaped_problem) * n + prefix;
}

extern "C" int simq_intention_maps_shapes(const simq_intention_segment* segments, int n_segments, const simq_intention_shaped_problem* problems,
                                          int n, void* d_desc, int64_t desc_bytes, float* d_out, int64_t out_floats, void* stream) {
    static_assert(sizeof(simq_intention_shaped_problem) % 8 == 0, "descriptors are padded to 8 bytes");
    SIMQ_REQUIRE(problems && d_desc && d_out, "intention_maps_shapes: NULL pointer");
    SIMQ_REQUIRE(n >= 1 && n <= (1 << 20), "intention_maps_shapes: n = %d (1 .. 2^20 problems)", n);
    SIMQ_REQUIRE(n_segments >= 0 && n_segments <= (1 << 24) && (n_segments == 0 || segments),
                 "intention_maps_shapes: n_segments = %d with segments %s", n_segments, segments ? "given" : "NULL");
    SIMQ_REQUIRE(((uintptr_t)d_desc & 7) == 0 && ((uintptr_t)d_out & 3) == 0,
                 "intention_maps_shapes: d_desc must be 8-byte and d_out 4-byte aligned");
    const int64_t need_desc = simq_intention_shapes_desc_bytes(n_segments, n);
    SIMQ_REQUIRE(desc_bytes >= need_desc, "intention_maps_shapes: d_desc holds %lld bytes, the descriptors and the tile table take %lld",
                 (long long)desc_bytes, (long long)need_desc);

    // per problem: shape, radius, segment range, place in d_out (and that place against d_desc); the prefix of the tile counts
    std::vector<int32_t> tile_begin((size_t)n + 1 + ((n + 1) & 1), 0);                                // (an even count: the padded block)
    std::vector<Span> spans((size_t)n);
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        const simq_intention_shaped_problem& p = problems[i];
        SIMQ_REQUIRE(p.rows >= 1 && p.cols >= 1 && (int64_t)p.rows * p.cols < (1 << 28),
                     "intention_maps_shapes: problem %d: a map of %d x %d (rows, cols >= 1, rows * cols < 2^28)", i, p.rows, p.cols);
        SIMQ_REQUIRE(p.radius >= 0 && p.radius <= kMaxRadius, "intention_maps_shapes: problem %d: radius = %d (0 .. %d: line thickness 1 .. %d)", i,
                     p.radius, kMaxRadius, kMaxRadius + 1);
        SIMQ_REQUIRE(p.seg_count >= 0 && p.seg_begin >= 0 && (int64_t)p.seg_begin + p.seg_count <= n_segments,
                     "intention_maps_shapes: problem %d: segments [%d, %d + %d) outside the %d given", i, p.seg_begin, p.seg_begin, p.seg_count,
                     n_segments);
        const int64_t cells = (int64_t)p.rows * p.cols;
        SIMQ_REQUIRE(fits(p.out_offset, cells, out_floats),
                     "intention_maps_shapes: problem %d: floats [%lld, %lld + %lld) of its %d x %d map lie outside the %lld of d_out", i,
                     (long long)p.out_offset, (long long)p.out_offset, (long long)cells, p.rows, p.cols, (long long)out_floats);
        SIMQ_REQUIRE(!overlaps(d_out + p.out_offset, cells * 4, d_desc, need_desc),
                     "intention_maps_shapes: problem %d: its map at float %lld of d_out overlaps d_desc", i, (long long)p.out_offset);
        spans[i] = {(uint64_t)p.out_offset, (uint64_t)(p.out_offset + cells), i};
        tile_begin[i] = (int32_t)blocks;
        blocks += (int64_t)((p.rows + kTileRows - 1) / kTileRows) * ((p.cols + kTileCols - 1) / kTileCols);
        SIMQ_REQUIRE(blocks <= 0x7fffffffLL, "intention_maps_shapes: problems 0 .. %d take %lld workgroups (at most 2^31 - 1)", i, (long long)blocks);
    }
    tile_begin[n] = (int32_t)blocks;
    if (const size_t i = first_overlap(spans))
        SIMQ_REQUIRE(false, "intention_maps_shapes: the maps of problems %d and %d overlap in d_out (floats [%llu, %llu) and [%llu, %llu))",
                     spans[i - 1].problem, spans[i].problem, (unsigned long long)spans[i - 1].lo, (unsigned long long)spans[i - 1].hi,
                     (unsigned long long)spans[i].lo, (unsigned long long)spans[i].hi);

    for (int k = 0; k < n_segments; ++k)
        if (check_segment_values("intention_maps_shapes", segments[k], k)) return -1;
    // Every segment ends inside the map of every problem that draws it.  Along each axis the problems claim their segments from the
    // smallest extent up, a segment once: whoever claims it has the smallest map it is drawn into, so a segment that fits there fits
    // every problem of its range, and the whole check is linear in segments and problems after the sort.
    std::vector<int> order((size_t)n), next((size_t)n_segments + 1);
    for (int axis = 0; axis < 2; ++axis) {
        for (int i = 0; i < n; ++i) order[i] = i;
        for (int k = 0; k <= n_segments; ++k) next[k] = k;
        std::sort(order.begin(), order.end(), [&](int a, int b) {
            const int ea = axis ? problems[a].cols : problems[a].rows, eb = axis ? problems[b].cols : problems[b].rows;
            return ea != eb ? ea < eb : a < b;
        });
        for (int i : order) {
            const simq_intention_shaped_problem& p = problems[i];
            const int extent = axis ? p.cols : p.rows, end = p.seg_begin + p.seg_count;
            for (int k = next_unclaimed(next, p.seg_begin); k < end; k = next_unclaimed(next, k)) {
                const simq_intention_segment& s = segments[k];
                const int a = axis ? s.c0 : s.r0, b = axis ? s.c1 : s.r1;
                SIMQ_REQUIRE(a >= 0 && a < extent && b >= 0 && b < extent,
                             "intention_maps_shapes: problem %d: segment %d: (%d, %d) -> (%d, %d) leaves the %d x %d map", i, k, s.r0, s.c0, s.r1,
                             s.c1, p.rows, p.cols);
                next[k] = k + 1;
            }
        }
    }

    const HostBlock parts[3] = {{segments, sizeof(simq_intention_segment) * (size_t)n_segments},
                                {problems, sizeof(simq_intention_shaped_problem) * (size_t)n},
                                {tile_begin.data(), sizeof(int32_t) * tile_begin.size()}};
    const char* at[3];
    hipStream_t s = static_cast<hipStream_t>(stream);
    SIMQ_CHECK_HIP(upload_descriptors(d_desc, parts, 3, at, s));
    ShapedDesc d;
    d.segs = reinterpret_cast<const simq_intention_segment*>(at[0]);
    d.probs = reinterpret_cast<const simq_intention_shaped_problem*>(at[1]);
    d.tile_begin = reinterpret_cast<const int32_t*>(at[2]);
    d.n = n;
    intention_maps_shapes_kernel<<<(unsigned)blocks, kThreads, 0, s>>>(d, d_out);
    SIMQ_CHECK_LAUNCH();
    note_launch("intention_maps_shapes");
    return 0;
}
