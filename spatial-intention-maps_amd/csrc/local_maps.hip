// libsimq: batched local state images -- the crop / rotation stage of Mapper.get_state
//   local_state_kernel       _get_local_map / _get_local_distance_map                              envs.py:2199-2215
//                            _create_global_robot_map + _create_global_overhead_map, per pixel     envs.py:2243-2275
//                            the constant (nonspatial intention) channels                          envs.py:2368-2375
//
// Exactness.  The reference's scipy.ndimage.rotate(order=0) maps an output index (oi, oj) to the input coordinate
// cc_h = offset[h] + (oi * R[h][0] + oj * R[h][1]) in float64 -- the two products summed first, then the offset -- and takes the
// input pixel floor(cc_h + 0.5) when 0 <= cc_h <= n - 1, else 0.  The centre of an even-sized rotated image lands within an ulp of
// x.5, so any other evaluation order (or a fused multiply-add) picks the neighbouring pixel there: the coordinate path is compiled with
// floating-point contraction off (rotate_index), and the ISA holds v_mul_f64 / v_add_f64 there and no v_fma_f64 / v_fmac_f64.  R, offset and the rotated shape come from the host
// (include/simq.h), so the device does no trigonometry.
//
// Shape.  One workgroup of 1024 lanes per problem.  Phase 0 computes each local pixel's global index once (36 KB of LDS); phase 1
// reduces the minimum of every DISTANCE channel over the 9216 pixels (wave shuffles, then LDS across the 16 waves); phase 2 walks the
// flattened (pixel, channel) index so that consecutive lanes write consecutive floats of the NHWC image.  Robot stamps are evaluated
// per pixel through the second rotation; no global robot map is materialised.
#include "batch_abi.h"
#include "../../include/simq.h"

#include <cmath>

namespace simq {

namespace {

constexpr int kW = SIMQ_STATE_WIDTH;              // 96
constexpr int kPix = kW * kW;                     // 9216
constexpr int kCrop = SIMQ_LOCAL_CROP;            // 136
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxShapeCrop = 193;                // ceil(136 * sqrt 2)
constexpr int kMaxShapeMask = 136;                // ceil(96 * sqrt 2)

struct Desc {                                     // the packed device copy of one call's descriptors
    const simq_local_map* maps;
    const simq_local_robot* robots;
    const simq_local_problem* probs;
    const simq_local_channel* chans;
    const float* masks;
    int C;
};

// input index along both axes of an n x n image for output index (oi, oj) of its rotation; false: outside (the pixel is 0)
__device__ __forceinline__ bool rotate_index(const simq_local_rotation& t, int n, int oi, int oj, int* i0, int* i1) {
    // HIP's __dmul_rn / __dadd_rn are plain * and + and hipcc contracts them into v_fmac_f64 by default: the pragma is what keeps every
    // product and sum of this function separately rounded (it travels with the operations when the function is inlined)
#pragma clang fp contract(off)
    const double di = (double)oi, dj = (double)oj, hi = (double)(n - 1);
    const double p00 = di * t.r[0], p01 = dj * t.r[1], p10 = di * t.r[2], p11 = dj * t.r[3];
    const double c0 = t.offset[0] + (p00 + p01);
    const double c1 = t.offset[1] + (p10 + p11);
    if (!(c0 >= 0.0 && c0 <= hi && c1 >= 0.0 && c1 <= hi)) return false;
    *i0 = min(max((int)floor(c0 + 0.5), 0), n - 1);
    *i1 = min(max((int)floor(c1 + 0.5), 0), n - 1);
    return true;
}

// max(0, max over the robots of value * rotated mask) at global pixel (gi, gj): the stamps of _create_global_robot_map
__device__ __forceinline__ float robot_value(const Desc& d, const simq_local_problem& p, int gi, int gj, bool seg) {
    float acc = 0.f;
    for (int k = 0; k < p.robot_count; ++k) {
        const simq_local_robot& r = d.robots[p.robot_begin + k];
        const int si = gi - (r.pixel_i - r.rot.shape[0] / 2), sj = gj - (r.pixel_j - r.rot.shape[1] / 2);
        if (si < 0 || si >= r.rot.shape[0] || sj < 0 || sj >= r.rot.shape[1]) continue;
        int mi, mj;
        if (!rotate_index(r.rot, kW, si, sj, &mi, &mj)) continue;      // (0 there: never above acc)
        const float v = d.masks[((int64_t)(seg ? r.seg_mask : r.mask) * kW + mi) * kW + mj] * (seg ? r.seg_value : r.map_value);
        if (v > acc) acc = v;
    }
    return acc;
}

__global__ void __launch_bounds__(kThreads) local_state_kernel(Desc d, float* __restrict__ out) {
    __shared__ int gidx[kPix];                    // gi * cols + gj of the local pixel, -1 outside the crop
    __shared__ float wave_min[kWaves];
    __shared__ float chan_min[SIMQ_LOCAL_MAX_CHANNELS];
    __shared__ int ch_kind[SIMQ_LOCAL_MAX_CHANNELS];              // the problem's channels, read once: kind, constant, map base pointer
    __shared__ float ch_value[SIMQ_LOCAL_MAX_CHANNELS];
    __shared__ const float* ch_map[SIMQ_LOCAL_MAX_CHANNELS];
    const simq_local_problem p = d.probs[blockIdx.x];
    const int tid = threadIdx.x, C = d.C;
    const int bi = p.rot.shape[0] / 2 - kW / 2, bj = p.rot.shape[1] / 2 - kW / 2;

    if (tid < C) {
        const simq_local_channel k = d.chans[(int64_t)blockIdx.x * C + tid];
        ch_kind[tid] = k.kind;
        ch_value[tid] = k.value;
        ch_map[tid] = (k.kind == SIMQ_LOCAL_MAP || k.kind == SIMQ_LOCAL_DISTANCE || k.kind == SIMQ_LOCAL_OVERHEAD) ? d.maps[k.map].d_data : nullptr;
    }
    for (int pix = tid; pix < kPix; pix += kThreads) {
        const int i = pix / kW, j = pix - i * kW;
        int ci, cj;
        gidx[pix] = rotate_index(p.rot, kCrop, i + bi, j + bj, &ci, &cj)
                        ? (p.pixel_i - kCrop / 2 + ci) * p.cols + (p.pixel_j - kCrop / 2 + cj) : -1;
    }
    __syncthreads();

    for (int c = 0; c < C; ++c) {
        if (ch_kind[c] != SIMQ_LOCAL_DISTANCE) continue;                 // (uniform over the workgroup)
        const float* m = ch_map[c];
        float v = INFINITY;
        for (int pix = tid; pix < kPix; pix += kThreads) {
            const int g = gidx[pix];
            v = min_nan(v, g >= 0 ? m[g] : 0.f);
        }
        v = wave_reduce(v, min_nan);
        if ((tid & 63) == 0) wave_min[tid >> 6] = v;
        __syncthreads();
        if (tid == 0) chan_min[c] = reduce_waves(wave_min, kWaves, min_nan);
        __syncthreads();
    }

    float* o = out + (int64_t)blockIdx.x * kPix * C;
    const int items = kPix * C;
    for (int it = tid; it < items; it += kThreads) {
        const int pix = it / C, c = it - pix * C;
        const int kind = ch_kind[c];
        const float* m = ch_map[c];
        const int g = gidx[pix];
        float v = 0.f;
        if (kind == SIMQ_LOCAL_CONSTANT) {
            v = ch_value[c];
        } else if (kind == SIMQ_LOCAL_DISTANCE) {
            v = (g >= 0 ? m[g] : 0.f) - chan_min[c];
        } else if (g >= 0) {
            if (kind == SIMQ_LOCAL_MAP) {
                v = m[g];
            } else {
                const int gi = g / p.cols, gj = g - gi * p.cols;
                v = robot_value(d, p, gi, gj, kind == SIMQ_LOCAL_OVERHEAD);
                if (kind == SIMQ_LOCAL_OVERHEAD && !(v > 0.f)) v = m[g];
            }
        }
        o[it] = v;
    }
}

bool finite_rotation(const simq_local_rotation& t) {
    for (double x : t.r)
        if (!std::isfinite(x)) return false;
    return std::isfinite(t.offset[0]) && std::isfinite(t.offset[1]);
}

}  // namespace

}  // namespace simq

using namespace simq;

extern "C" int64_t simq_local_state_desc_bytes(int n_maps, int n_robots, int n, int n_channels) {
    if (n_maps < 0 || n_robots < 0 || n < 0 || n_channels < 0) return -1;
    return (int64_t)sizeof(simq_local_map) * n_maps + (int64_t)sizeof(simq_local_robot) * n_robots +
           (int64_t)sizeof(simq_local_problem) * n + (int64_t)sizeof(simq_local_channel) * n * n_channels;
}

extern "C" int simq_local_state_images(const simq_local_map* maps, int n_maps, const float* d_masks, int n_masks,
                                       const simq_local_robot* robots, int n_robots, const simq_local_problem* problems, int n,
                                       const simq_local_channel* channels, int n_channels, void* d_desc, int64_t desc_bytes, float* d_out,
                                       int64_t out_floats, void* stream) {
    SIMQ_REQUIRE(problems && channels && d_desc && d_out, "local_state_images: NULL pointer");
    SIMQ_REQUIRE(n >= 1 && n <= (1 << 20), "local_state_images: n = %d (1 .. 2^20 problems)", n);
    SIMQ_REQUIRE(n_channels >= 1 && n_channels <= SIMQ_LOCAL_MAX_CHANNELS, "local_state_images: n_channels = %d (1 .. %d)", n_channels,
                 SIMQ_LOCAL_MAX_CHANNELS);
    SIMQ_REQUIRE(n_maps >= 0 && n_maps <= (1 << 24) && (n_maps == 0 || maps), "local_state_images: n_maps = %d with maps %s", n_maps,
                 maps ? "given" : "NULL");
    SIMQ_REQUIRE(n_robots >= 0 && n_robots <= (1 << 24) && (n_robots == 0 || (robots && d_masks && n_masks >= 1)),
                 "local_state_images: n_robots = %d needs robots and a mask bank (n_masks = %d)", n_robots, n_masks);
    SIMQ_REQUIRE(n_masks >= 0 && n_masks <= (1 << 16), "local_state_images: n_masks = %d (0 .. 2^16)", n_masks);
    SIMQ_REQUIRE(((uintptr_t)d_desc & 7) == 0 && ((uintptr_t)d_out & 3) == 0, "local_state_images: d_desc must be 8-byte and d_out 4-byte aligned");
    const int64_t need_desc = simq_local_state_desc_bytes(n_maps, n_robots, n, n_channels);
    SIMQ_REQUIRE(desc_bytes >= need_desc, "local_state_images: d_desc holds %lld bytes, the descriptors take %lld", (long long)desc_bytes,
                 (long long)need_desc);
    const int64_t need_out = (int64_t)n * kPix * n_channels;
    SIMQ_REQUIRE(out_floats >= need_out, "local_state_images: d_out holds %lld floats, %d x 96 x 96 x %d images take %lld",
                 (long long)out_floats, n, n_channels, (long long)need_out);
    const int64_t out_bytes = need_out * 4;
    SIMQ_REQUIRE(!overlaps(d_out, out_bytes, d_desc, need_desc), "local_state_images: d_out overlaps d_desc");
    for (int k = 0; k < n_maps; ++k) {
        const simq_local_map& m = maps[k];
        SIMQ_REQUIRE(m.d_data && ((uintptr_t)m.d_data & 3) == 0, "local_state_images: map %d: NULL or misaligned d_data", k);
        SIMQ_REQUIRE(m.rows >= kCrop && m.cols >= kCrop && (int64_t)m.rows * m.cols < (1 << 28),
                     "local_state_images: map %d is %d x %d (rows, cols >= %d, rows * cols < 2^28)", k, m.rows, m.cols, kCrop);
        SIMQ_REQUIRE(!overlaps(d_out, out_bytes, m.d_data, (int64_t)m.rows * m.cols * 4), "local_state_images: d_out overlaps map %d", k);
    }
    if (n_masks > 0 && d_masks)
        SIMQ_REQUIRE(!overlaps(d_out, out_bytes, d_masks, (int64_t)n_masks * kPix * 4), "local_state_images: d_out overlaps the mask bank");
    for (int k = 0; k < n_robots; ++k) {
        const simq_local_robot& r = robots[k];
        SIMQ_REQUIRE(r.mask >= 0 && r.mask < n_masks && r.seg_mask >= 0 && r.seg_mask < n_masks,
                     "local_state_images: robot %d: mask %d / seg_mask %d outside the bank of %d", k, r.mask, r.seg_mask, n_masks);
        SIMQ_REQUIRE(r.rot.shape[0] >= kW && r.rot.shape[0] <= kMaxShapeMask && r.rot.shape[1] >= kW && r.rot.shape[1] <= kMaxShapeMask,
                     "local_state_images: robot %d: rotated mask shape %d x %d outside [%d, %d]", k, r.rot.shape[0], r.rot.shape[1], kW,
                     kMaxShapeMask);
        SIMQ_REQUIRE(finite_rotation(r.rot), "local_state_images: robot %d: rotation is not finite", k);
    }
    for (int i = 0; i < n; ++i) {
        const simq_local_problem& p = problems[i];
        SIMQ_REQUIRE(p.rows >= kCrop && p.cols >= kCrop && (int64_t)p.rows * p.cols < (1 << 28),
                     "local_state_images: problem %d: maps of %d x %d (rows, cols >= %d, rows * cols < 2^28)", i, p.rows, p.cols, kCrop);
        SIMQ_REQUIRE(p.pixel_i >= kCrop / 2 && p.pixel_i <= p.rows - kCrop / 2 && p.pixel_j >= kCrop / 2 && p.pixel_j <= p.cols - kCrop / 2,
                     "local_state_images: problem %d: the %d x %d crop around pixel (%d, %d) leaves its %d x %d map", i, kCrop, kCrop,
                     p.pixel_i, p.pixel_j, p.rows, p.cols);
        SIMQ_REQUIRE(p.rot.shape[0] >= kCrop && p.rot.shape[0] <= kMaxShapeCrop && p.rot.shape[1] >= kCrop && p.rot.shape[1] <= kMaxShapeCrop,
                     "local_state_images: problem %d: rotated crop shape %d x %d outside [%d, %d]", i, p.rot.shape[0], p.rot.shape[1], kCrop,
                     kMaxShapeCrop);
        SIMQ_REQUIRE(finite_rotation(p.rot), "local_state_images: problem %d: rotation is not finite", i);
        SIMQ_REQUIRE(p.robot_count >= 0 && p.robot_begin >= 0 && (int64_t)p.robot_begin + p.robot_count <= n_robots,
                     "local_state_images: problem %d: robots [%d, %d + %d) outside the %d given", i, p.robot_begin, p.robot_begin,
                     p.robot_count, n_robots);
        for (int k = p.robot_begin; k < p.robot_begin + p.robot_count; ++k) {
            const simq_local_robot& r = robots[k];
            const int si = r.pixel_i - r.rot.shape[0] / 2, sj = r.pixel_j - r.rot.shape[1] / 2;
            SIMQ_REQUIRE(si >= 0 && si + r.rot.shape[0] <= p.rows && sj >= 0 && sj + r.rot.shape[1] <= p.cols,
                         "local_state_images: problem %d: the stamp of robot %d at pixel (%d, %d) leaves the %d x %d map", i, k, r.pixel_i,
                         r.pixel_j, p.rows, p.cols);
        }
        for (int c = 0; c < n_channels; ++c) {
            const simq_local_channel& ch = channels[(int64_t)i * n_channels + c];
            SIMQ_REQUIRE(ch.kind >= SIMQ_LOCAL_MAP && ch.kind <= SIMQ_LOCAL_CONSTANT, "local_state_images: problem %d channel %d: kind %d", i, c,
                         ch.kind);
            if (ch.kind == SIMQ_LOCAL_MAP || ch.kind == SIMQ_LOCAL_DISTANCE || ch.kind == SIMQ_LOCAL_OVERHEAD) {
                SIMQ_REQUIRE(ch.map >= 0 && ch.map < n_maps, "local_state_images: problem %d channel %d: map %d outside the %d given", i, c,
                             ch.map, n_maps);
                SIMQ_REQUIRE(maps[ch.map].rows == p.rows && maps[ch.map].cols == p.cols,
                             "local_state_images: problem %d channel %d: map %d is %d x %d, the problem's maps are %d x %d", i, c, ch.map,
                             maps[ch.map].rows, maps[ch.map].cols, p.rows, p.cols);
            }
        }
    }

    const HostBlock parts[4] = {{maps, sizeof(simq_local_map) * (size_t)n_maps},
                                {robots, sizeof(simq_local_robot) * (size_t)n_robots},
                                {problems, sizeof(simq_local_problem) * (size_t)n},
                                {channels, sizeof(simq_local_channel) * (size_t)n * n_channels}};
    const char* at[4];
    hipStream_t s = static_cast<hipStream_t>(stream);
    SIMQ_CHECK_HIP(upload_descriptors(d_desc, parts, 4, at, s));
    Desc d;
    d.maps = reinterpret_cast<const simq_local_map*>(at[0]);
    d.robots = reinterpret_cast<const simq_local_robot*>(at[1]);
    d.probs = reinterpret_cast<const simq_local_problem*>(at[2]);
    d.chans = reinterpret_cast<const simq_local_channel*>(at[3]);
    d.masks = d_masks;
    d.C = n_channels;
    local_state_kernel<<<n, kThreads, 0, s>>>(d, d_out);
    SIMQ_CHECK_LAUNCH();
    note_launch("local_state");
    return 0;
}
