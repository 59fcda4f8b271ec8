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
#include <type_traits>

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

struct SlotDesc : Desc {                          // simq_local_state_images_slots: problem p is written to pool slot slots[p]
    const int64_t* slots;
    int64_t pool_slots;
};

// where problem p's [96][96][C] image begins: the dense batch, or the problem's pool slot (NULL: a slot outside the pool -- the host has
// refused those, this guards a table changed behind its back)
template <typename OT>
__device__ __forceinline__ OT* image_of(const Desc& d, OT* out, unsigned p) {
    return out + (int64_t)p * kPix * d.C;
}
template <typename OT>
__device__ __forceinline__ OT* image_of(const SlotDesc& d, OT* pool, unsigned p) {
    const int64_t slot = d.slots[p];
    return slot >= 0 && slot < d.pool_slots ? pool + slot * ((int64_t)kPix * d.C) : nullptr;
}

struct PoolDesc : Desc {                          // simq_local_state_images_pools: problem p is written to slot dests[p].slot of pool dests[p].pool
    const simq_local_pool* pools;
    const simq_local_dest* dests;
    int n_pools;
};

struct PoolImage {                                // an image in one of several pools: where it begins and what its elements are
    void* base;
    bool bf16;
};

// Both table entries are indexed by values that are uniform over the workgroup (blockIdx, then the entry just read), so they are scalar
// loads and `bf16` is a scalar: the branch on it at the store is taken by the whole workgroup.  NULL as in the slot form: a pool index or
// a slot outside its table.
__device__ __forceinline__ PoolImage image_of(const PoolDesc& d, void*, unsigned p) {
    const simq_local_dest t = d.dests[p];
    if (t.pool < 0 || t.pool >= d.n_pools) return {nullptr, false};
    const simq_local_pool q = d.pools[t.pool];
    if (t.slot < 0 || t.slot >= q.pool_slots) return {nullptr, false};
    const int64_t slot_bytes = (int64_t)kPix * d.C * (q.bf16 ? 2 : 4);
    return {static_cast<char*>(q.d_pool) + t.slot * slot_bytes, q.bf16 != 0};
}

template <typename OT>
__device__ __forceinline__ bool no_image(const OT* o) { return o == nullptr; }
__device__ __forceinline__ bool no_image(const PoolImage& o) { return o.base == nullptr; }

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

// what is stored for the fp32 value v of one state element: v itself, or -- a pool of bf16 states (simq_plan_options.bf16_states) --
// v rounded ONCE with the conversion the first convolution applies to an fp32 state, so that the bits in the pool are the bits that
// convolution would have made of the fp32 state
__device__ __forceinline__ void store_state(float* o, float v) { *o = v; }
__device__ __forceinline__ void store_state(uint16_t* o, float v) { *o = __builtin_bit_cast(uint16_t, (__bf16)v); }

// element `it` of an image: of a typed one, or of a pool image as the pool's type (the one branch of the pools form)
template <typename OT>
__device__ __forceinline__ void store_element(OT* o, int it, float v) { store_state(o + it, v); }
__device__ __forceinline__ void store_element(const PoolImage& o, int it, float v) {
    if (o.bf16)
        store_state(static_cast<uint16_t*>(o.base) + it, v);
    else
        store_state(static_cast<float*>(o.base) + it, v);
}

// D: Desc (out is the [n][96][96][C] batch), SlotDesc (out is the pool) or PoolDesc (out is unused: the pools are in the descriptor);
// OT: float, or uint16_t for bf16 states (PoolDesc: void, the type comes with the problem's pool); everything but the image's base and
// the last store is the same code
template <typename D, typename OT>
__global__ void __launch_bounds__(kThreads) local_state_kernel(D d, OT* __restrict__ out) {
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

    const auto o = image_of(d, out, blockIdx.x);
    if constexpr (!std::is_same<D, Desc>::value)
        if (no_image(o)) return;                                         // (uniform over the workgroup)
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
        store_element(o, it, v);
    }
}

bool finite_rotation(const simq_local_rotation& t) {
    for (double x : t.r)
        if (!std::isfinite(x)) return false;
    return std::isfinite(t.offset[0]) && std::isfinite(t.offset[1]);
}


// The checks both entry points make of their host descriptors, in the order simq_local_state_images has always made them; `who` heads
// the refusal.  Everything about the output is the entry point's own.
int check_counts(const char* who, const simq_local_map* maps, int n_maps, const float* d_masks, int n_masks, const simq_local_robot* robots,
                 int n_robots, int n, int n_channels) {
    SIMQ_REQUIRE(n >= 1 && n <= (1 << 20), "%s: n = %d (1 .. 2^20 problems)", who, n);
    SIMQ_REQUIRE(n_channels >= 1 && n_channels <= SIMQ_LOCAL_MAX_CHANNELS, "%s: n_channels = %d (1 .. %d)", who, n_channels,
                 SIMQ_LOCAL_MAX_CHANNELS);
    SIMQ_REQUIRE(n_maps >= 0 && n_maps <= (1 << 24) && (n_maps == 0 || maps), "%s: n_maps = %d with maps %s", who, n_maps,
                 maps ? "given" : "NULL");
    SIMQ_REQUIRE(n_robots >= 0 && n_robots <= (1 << 24) && (n_robots == 0 || (robots && d_masks && n_masks >= 1)),
                 "%s: n_robots = %d needs robots and a mask bank (n_masks = %d)", who, n_robots, n_masks);
    SIMQ_REQUIRE(n_masks >= 0 && n_masks <= (1 << 16), "%s: n_masks = %d (0 .. 2^16)", who, n_masks);
    return 0;
}

int check_map(const char* who, const simq_local_map& m, int k) {
    SIMQ_REQUIRE(m.d_data && ((uintptr_t)m.d_data & 3) == 0, "%s: map %d: NULL or misaligned d_data", who, k);
    SIMQ_REQUIRE(m.rows >= kCrop && m.cols >= kCrop && (int64_t)m.rows * m.cols < (1 << 28),
                 "%s: map %d is %d x %d (rows, cols >= %d, rows * cols < 2^28)", who, k, m.rows, m.cols, kCrop);
    return 0;
}

int check_tables(const char* who, const simq_local_map* maps, int n_maps, int n_masks, const simq_local_robot* robots, int n_robots,
                 const simq_local_problem* problems, int n, const simq_local_channel* channels, int n_channels) {
    for (int k = 0; k < n_robots; ++k) {
        const simq_local_robot& r = robots[k];
        SIMQ_REQUIRE(r.mask >= 0 && r.mask < n_masks && r.seg_mask >= 0 && r.seg_mask < n_masks,
                     "%s: robot %d: mask %d / seg_mask %d outside the bank of %d", who, k, r.mask, r.seg_mask, n_masks);
        SIMQ_REQUIRE(r.rot.shape[0] >= kW && r.rot.shape[0] <= kMaxShapeMask && r.rot.shape[1] >= kW && r.rot.shape[1] <= kMaxShapeMask,
                     "%s: robot %d: rotated mask shape %d x %d outside [%d, %d]", who, k, r.rot.shape[0], r.rot.shape[1], kW, kMaxShapeMask);
        SIMQ_REQUIRE(finite_rotation(r.rot), "%s: robot %d: rotation is not finite", who, k);
    }
    for (int i = 0; i < n; ++i) {
        const simq_local_problem& p = problems[i];
        SIMQ_REQUIRE(p.rows >= kCrop && p.cols >= kCrop && (int64_t)p.rows * p.cols < (1 << 28),
                     "%s: problem %d: maps of %d x %d (rows, cols >= %d, rows * cols < 2^28)", who, i, p.rows, p.cols, kCrop);
        SIMQ_REQUIRE(p.pixel_i >= kCrop / 2 && p.pixel_i <= p.rows - kCrop / 2 && p.pixel_j >= kCrop / 2 && p.pixel_j <= p.cols - kCrop / 2,
                     "%s: problem %d: the %d x %d crop around pixel (%d, %d) leaves its %d x %d map", who, i, kCrop, kCrop, p.pixel_i,
                     p.pixel_j, p.rows, p.cols);
        SIMQ_REQUIRE(p.rot.shape[0] >= kCrop && p.rot.shape[0] <= kMaxShapeCrop && p.rot.shape[1] >= kCrop && p.rot.shape[1] <= kMaxShapeCrop,
                     "%s: problem %d: rotated crop shape %d x %d outside [%d, %d]", who, i, p.rot.shape[0], p.rot.shape[1], kCrop,
                     kMaxShapeCrop);
        SIMQ_REQUIRE(finite_rotation(p.rot), "%s: problem %d: rotation is not finite", who, i);
        SIMQ_REQUIRE(p.robot_count >= 0 && p.robot_begin >= 0 && (int64_t)p.robot_begin + p.robot_count <= n_robots,
                     "%s: problem %d: robots [%d, %d + %d) outside the %d given", who, i, p.robot_begin, p.robot_begin, p.robot_count,
                     n_robots);
        for (int k = p.robot_begin; k < p.robot_begin + p.robot_count; ++k) {
            const simq_local_robot& r = robots[k];
            const int si = r.pixel_i - r.rot.shape[0] / 2, sj = r.pixel_j - r.rot.shape[1] / 2;
            SIMQ_REQUIRE(si >= 0 && si + r.rot.shape[0] <= p.rows && sj >= 0 && sj + r.rot.shape[1] <= p.cols,
                         "%s: problem %d: the stamp of robot %d at pixel (%d, %d) leaves the %d x %d map", who, i, k, r.pixel_i, r.pixel_j,
                         p.rows, p.cols);
        }
        for (int c = 0; c < n_channels; ++c) {
            const simq_local_channel& ch = channels[(int64_t)i * n_channels + c];
            SIMQ_REQUIRE(ch.kind >= SIMQ_LOCAL_MAP && ch.kind <= SIMQ_LOCAL_CONSTANT, "%s: problem %d channel %d: kind %d", who, i, c, ch.kind);
            if (ch.kind == SIMQ_LOCAL_MAP || ch.kind == SIMQ_LOCAL_DISTANCE || ch.kind == SIMQ_LOCAL_OVERHEAD) {
                SIMQ_REQUIRE(ch.map >= 0 && ch.map < n_maps, "%s: problem %d channel %d: map %d outside the %d given", who, i, c, ch.map,
                             n_maps);
                SIMQ_REQUIRE(maps[ch.map].rows == p.rows && maps[ch.map].cols == p.cols,
                             "%s: problem %d channel %d: map %d is %d x %d, the problem's maps are %d x %d", who, i, c, ch.map,
                             maps[ch.map].rows, maps[ch.map].cols, p.rows, p.cols);
            }
        }
    }
    return 0;
}

// the descriptor tables of one call, packed into d_desc behind each other; `more`: the n_more (0 .. 2) blocks of the entry's own behind
// them -- the n pool slots, or the pool table and the destinations -- and more_at where each of those lies on the device
template <typename D>
int upload_tables(D* d, const simq_local_map* maps, int n_maps, const float* d_masks, const simq_local_robot* robots, int n_robots,
                  const simq_local_problem* problems, int n, const simq_local_channel* channels, int n_channels, const HostBlock* more,
                  int n_more, void* d_desc, const char** more_at, hipStream_t s) {
    HostBlock parts[6] = {{maps, sizeof(simq_local_map) * (size_t)n_maps},
                          {robots, sizeof(simq_local_robot) * (size_t)n_robots},
                          {problems, sizeof(simq_local_problem) * (size_t)n},
                          {channels, sizeof(simq_local_channel) * (size_t)n * n_channels}};
    for (int k = 0; k < n_more; ++k) parts[4 + k] = more[k];
    const char* at[6];
    SIMQ_CHECK_HIP(upload_descriptors(d_desc, parts, 4 + n_more, at, s));
    d->maps = reinterpret_cast<const simq_local_map*>(at[0]);
    d->robots = reinterpret_cast<const simq_local_robot*>(at[1]);
    d->probs = reinterpret_cast<const simq_local_problem*>(at[2]);
    d->chans = reinterpret_cast<const simq_local_channel*>(at[3]);
    d->masks = d_masks;
    d->C = n_channels;
    for (int k = 0; k < n_more; ++k) more_at[k] = at[4 + k];
    return 0;
}

}  // namespace

}  // namespace simq

using namespace simq;

extern "C" int64_t simq_local_state_desc_bytes(int n_maps, int n_robots, int n, int n_channels) {
    if (n_maps < 0 || n_robots < 0 || n < 0 || n_channels < 0) return -1;
    return (int64_t)sizeof(simq_local_map) * n_maps + (int64_t)sizeof(simq_local_robot) * n_robots +
           (int64_t)sizeof(simq_local_problem) * n + (int64_t)sizeof(simq_local_channel) * n * n_channels;
}

extern "C" int64_t simq_local_state_slots_desc_bytes(int n_maps, int n_robots, int n, int n_channels) {
    const int64_t tables = simq_local_state_desc_bytes(n_maps, n_robots, n, n_channels);
    return tables < 0 ? -1 : tables + (int64_t)sizeof(int64_t) * n;
}

extern "C" int64_t simq_local_state_pools_desc_bytes(int n_maps, int n_robots, int n, int n_channels, int n_pools) {
    const int64_t slots = simq_local_state_slots_desc_bytes(n_maps, n_robots, n, n_channels);
    return slots < 0 || n_pools < 0 ? -1 : slots + (int64_t)sizeof(simq_local_pool) * n_pools + (int64_t)sizeof(simq_local_dest) * n;
}

namespace {

// the element word of the refusals: the fp32 entries keep the texts they have always had
template <typename OT> struct StateElem;
template <> struct StateElem<float> { static const char* plural() { return "floats"; } };
template <> struct StateElem<uint16_t> { static const char* plural() { return "bf16 elements"; } };

// simq_local_state_images / simq_local_state_images_bf16: one body, OT the element type of d_out
template <typename OT>
int state_images(const char* who, const char* family, const simq_local_map* maps, int n_maps, const float* d_masks, int n_masks,
                 const simq_local_robot* robots, int n_robots, const simq_local_problem* problems, int n, const simq_local_channel* channels,
                 int n_channels, void* d_desc, int64_t desc_bytes, OT* d_out, int64_t out_elems, void* stream) {
    constexpr int kElem = (int)sizeof(OT);
    SIMQ_REQUIRE(problems && channels && d_desc && d_out, "%s: NULL pointer", who);
    if (int rc = check_counts(who, maps, n_maps, d_masks, n_masks, robots, n_robots, n, n_channels)) return rc;
    SIMQ_REQUIRE(((uintptr_t)d_desc & 7) == 0 && ((uintptr_t)d_out & (kElem - 1)) == 0, "%s: d_desc must be 8-byte and d_out %d-byte aligned", who, kElem);
    const int64_t need_desc = simq_local_state_desc_bytes(n_maps, n_robots, n, n_channels);
    SIMQ_REQUIRE(desc_bytes >= need_desc, "%s: d_desc holds %lld bytes, the descriptors take %lld", who, (long long)desc_bytes,
                 (long long)need_desc);
    const int64_t need_out = (int64_t)n * kPix * n_channels;
    SIMQ_REQUIRE(out_elems >= need_out, "%s: d_out holds %lld %s, %d x 96 x 96 x %d images take %lld", who,
                 (long long)out_elems, StateElem<OT>::plural(), n, n_channels, (long long)need_out);
    const int64_t out_bytes = need_out * kElem;
    SIMQ_REQUIRE(!overlaps(d_out, out_bytes, d_desc, need_desc), "%s: d_out overlaps d_desc", who);
    for (int k = 0; k < n_maps; ++k) {
        if (int rc = check_map(who, maps[k], k)) return rc;
        SIMQ_REQUIRE(!overlaps(d_out, out_bytes, maps[k].d_data, (int64_t)maps[k].rows * maps[k].cols * 4), "%s: d_out overlaps map %d", who, k);
    }
    if (n_masks > 0 && d_masks)
        SIMQ_REQUIRE(!overlaps(d_out, out_bytes, d_masks, (int64_t)n_masks * kPix * 4), "%s: d_out overlaps the mask bank", who);
    if (int rc = check_tables(who, maps, n_maps, n_masks, robots, n_robots, problems, n, channels, n_channels)) return rc;

    hipStream_t s = static_cast<hipStream_t>(stream);
    Desc d;
    if (int rc = upload_tables(&d, maps, n_maps, d_masks, robots, n_robots, problems, n, channels, n_channels, nullptr, 0, d_desc, nullptr, s)) return rc;
    local_state_kernel<Desc, OT><<<n, kThreads, 0, s>>>(d, d_out);
    SIMQ_CHECK_LAUNCH();
    note_launch(family);
    return 0;
}

// simq_local_state_images_slots / simq_local_state_images_slots_bf16: pool slots of 96 * 96 * C elements of OT
template <typename OT>
int state_images_slots(const char* who, const char* family, const simq_local_map* maps, int n_maps, const float* d_masks, int n_masks,
                       const simq_local_robot* robots, int n_robots, const simq_local_problem* problems, int n,
                       const simq_local_channel* channels, int n_channels, const int64_t* slots, void* d_desc, int64_t desc_bytes, OT* d_pool,
                       int64_t pool_slots, void* stream) {
    constexpr int kElem = (int)sizeof(OT);
    SIMQ_REQUIRE(problems && channels && slots && d_desc && d_pool, "%s: NULL pointer", who);
    if (int rc = check_counts(who, maps, n_maps, d_masks, n_masks, robots, n_robots, n, n_channels)) return rc;
    SIMQ_REQUIRE(pool_slots >= 1 && pool_slots <= ((int64_t)1 << 40) / (kPix * 4), "%s: pool_slots = %lld (1 .. 2^40 bytes of pool)", who,
                 (long long)pool_slots);
    SIMQ_REQUIRE(((uintptr_t)d_desc & 7) == 0 && ((uintptr_t)d_pool & (kElem - 1)) == 0,
                 "%s: d_desc must be 8-byte and d_pool %d-byte aligned", who, kElem);
    const int64_t need_desc = simq_local_state_slots_desc_bytes(n_maps, n_robots, n, n_channels);
    SIMQ_REQUIRE(desc_bytes >= need_desc, "%s: d_desc holds %lld bytes, the descriptors and the slot table take %lld", who,
                 (long long)desc_bytes, (long long)need_desc);
    std::vector<int64_t> sorted;
    int64_t which = 0;
    const int bad = check_slots(slots, n, pool_slots, sorted, &which);
    SIMQ_REQUIRE(bad != 1, "%s: slot %lld outside the pool of %lld", who, (long long)which, (long long)pool_slots);
    SIMQ_REQUIRE(bad != 2, "%s: slot %lld is named twice", who, (long long)which);
    // the pool as a whole may hold what the launch reads (a map in another slot): only the slots written must be clear of it
    const int64_t item_bytes = (int64_t)kPix * n_channels * kElem;
    int64_t hit = written_slot_in(sorted, d_pool, item_bytes, pool_slots, d_desc, need_desc);
    SIMQ_REQUIRE(hit == -1, "%s: slot %lld overlaps d_desc", who, (long long)hit);
    for (int k = 0; k < n_maps; ++k) {
        if (int rc = check_map(who, maps[k], k)) return rc;
        hit = written_slot_in(sorted, d_pool, item_bytes, pool_slots, maps[k].d_data, (int64_t)maps[k].rows * maps[k].cols * 4);
        SIMQ_REQUIRE(hit == -1, "%s: slot %lld overlaps map %d", who, (long long)hit, k);
    }
    if (n_masks > 0 && d_masks) {
        hit = written_slot_in(sorted, d_pool, item_bytes, pool_slots, d_masks, (int64_t)n_masks * kPix * 4);
        SIMQ_REQUIRE(hit == -1, "%s: slot %lld overlaps the mask bank", who, (long long)hit);
    }
    if (int rc = check_tables(who, maps, n_maps, n_masks, robots, n_robots, problems, n, channels, n_channels)) return rc;

    hipStream_t s = static_cast<hipStream_t>(stream);
    SlotDesc d;
    const HostBlock table = {slots, sizeof(int64_t) * (size_t)n};
    const char* slots_at = nullptr;
    if (int rc = upload_tables(&d, maps, n_maps, d_masks, robots, n_robots, problems, n, channels, n_channels, &table, 1, d_desc, &slots_at, s)) return rc;
    d.slots = reinterpret_cast<const int64_t*>(slots_at);
    d.pool_slots = pool_slots;
    local_state_kernel<SlotDesc, OT><<<n, kThreads, 0, s>>>(d, d_pool);
    SIMQ_CHECK_LAUNCH();
    note_launch(family);
    return 0;
}

// simq_local_state_images_pools: the slots entry's checks, pool by pool
int state_images_pools(const char* who, const simq_local_map* maps, int n_maps, const float* d_masks, int n_masks, const simq_local_robot* robots,
                       int n_robots, const simq_local_problem* problems, int n, const simq_local_channel* channels, int n_channels,
                       const simq_local_pool* pools, int n_pools, const simq_local_dest* dests, void* d_desc, int64_t desc_bytes,
                       void* stream) {
    SIMQ_REQUIRE(problems && channels && pools && dests && d_desc, "%s: NULL pointer", who);
    if (int rc = check_counts(who, maps, n_maps, d_masks, n_masks, robots, n_robots, n, n_channels)) return rc;
    SIMQ_REQUIRE(n_pools >= 1 && n_pools <= SIMQ_LOCAL_MAX_POOLS, "%s: n_pools = %d (1 .. %d)", who, n_pools, SIMQ_LOCAL_MAX_POOLS);
    int64_t item_bytes[SIMQ_LOCAL_MAX_POOLS];
    for (int k = 0; k < n_pools; ++k) {
        const simq_local_pool& q = pools[k];
        SIMQ_REQUIRE(q.bf16 == 0 || q.bf16 == 1, "%s: pool %d: bf16 = %d (0: fp32 elements, 1: bf16)", who, k, q.bf16);
        const int elem = q.bf16 ? 2 : 4;
        SIMQ_REQUIRE(q.d_pool, "%s: pool %d: NULL d_pool", who, k);
        SIMQ_REQUIRE(((uintptr_t)q.d_pool & (elem - 1)) == 0, "%s: pool %d: d_pool must be %d-byte aligned", who, k, elem);
        SIMQ_REQUIRE(q.pool_slots >= 1 && q.pool_slots <= ((int64_t)1 << 40) / (kPix * 4), "%s: pool %d: pool_slots = %lld (1 .. 2^40 bytes of pool)",
                     who, k, (long long)q.pool_slots);
        item_bytes[k] = (int64_t)kPix * n_channels * elem;
    }
    SIMQ_REQUIRE(((uintptr_t)d_desc & 7) == 0, "%s: d_desc must be 8-byte aligned", who);
    const int64_t need_desc = simq_local_state_pools_desc_bytes(n_maps, n_robots, n, n_channels, n_pools);
    SIMQ_REQUIRE(desc_bytes >= need_desc, "%s: d_desc holds %lld bytes, the descriptors, the pool table and the destinations take %lld", who,
                 (long long)desc_bytes, (long long)need_desc);
    for (int a = 0; a < n_pools; ++a)
        for (int b = a + 1; b < n_pools; ++b)
            SIMQ_REQUIRE(!overlaps(pools[a].d_pool, pools[a].pool_slots * item_bytes[a], pools[b].d_pool, pools[b].pool_slots * item_bytes[b]),
                         "%s: pool %d overlaps pool %d", who, a, b);
    std::vector<int64_t> named[SIMQ_LOCAL_MAX_POOLS], sorted[SIMQ_LOCAL_MAX_POOLS];
    for (int p = 0; p < n; ++p) {
        SIMQ_REQUIRE(dests[p].pool >= 0 && dests[p].pool < n_pools, "%s: problem %d: pool %d outside the %d given", who, p, dests[p].pool, n_pools);
        named[dests[p].pool].push_back(dests[p].slot);
    }
    for (int k = 0; k < n_pools; ++k) {
        int64_t which = 0;
        const int bad = check_slots(named[k].data(), (int)named[k].size(), pools[k].pool_slots, sorted[k], &which);
        SIMQ_REQUIRE(bad != 1, "%s: slot %lld outside pool %d of %lld", who, (long long)which, k, (long long)pools[k].pool_slots);
        SIMQ_REQUIRE(bad != 2, "%s: slot %lld of pool %d is named twice", who, (long long)which, k);
    }
    // as in the slots entry, only the slots written must be clear of what the launch reads: a pool may hold a map in another slot
    for (int k = 0; k < n_pools; ++k) {
        const int64_t hit = written_slot_in(sorted[k], pools[k].d_pool, item_bytes[k], pools[k].pool_slots, d_desc, need_desc);
        SIMQ_REQUIRE(hit == -1, "%s: slot %lld of pool %d overlaps d_desc", who, (long long)hit, k);
    }
    for (int m = 0; m < n_maps; ++m) {
        if (int rc = check_map(who, maps[m], m)) return rc;
        for (int k = 0; k < n_pools; ++k) {
            const int64_t hit = written_slot_in(sorted[k], pools[k].d_pool, item_bytes[k], pools[k].pool_slots, maps[m].d_data,
                                                (int64_t)maps[m].rows * maps[m].cols * 4);
            SIMQ_REQUIRE(hit == -1, "%s: slot %lld of pool %d overlaps map %d", who, (long long)hit, k, m);
        }
    }
    if (n_masks > 0 && d_masks)
        for (int k = 0; k < n_pools; ++k) {
            const int64_t hit = written_slot_in(sorted[k], pools[k].d_pool, item_bytes[k], pools[k].pool_slots, d_masks, (int64_t)n_masks * kPix * 4);
            SIMQ_REQUIRE(hit == -1, "%s: slot %lld of pool %d overlaps the mask bank", who, (long long)hit, k);
        }
    if (int rc = check_tables(who, maps, n_maps, n_masks, robots, n_robots, problems, n, channels, n_channels)) return rc;

    hipStream_t s = static_cast<hipStream_t>(stream);
    PoolDesc d;
    const HostBlock tables[2] = {{pools, sizeof(simq_local_pool) * (size_t)n_pools}, {dests, sizeof(simq_local_dest) * (size_t)n}};
    const char* at[2] = {nullptr, nullptr};
    if (int rc = upload_tables(&d, maps, n_maps, d_masks, robots, n_robots, problems, n, channels, n_channels, tables, 2, d_desc, at, s)) return rc;
    d.pools = reinterpret_cast<const simq_local_pool*>(at[0]);
    d.dests = reinterpret_cast<const simq_local_dest*>(at[1]);
    d.n_pools = n_pools;
    local_state_kernel<PoolDesc, void><<<n, kThreads, 0, s>>>(d, nullptr);
    SIMQ_CHECK_LAUNCH();
    note_launch("local_state_pools");
    return 0;
}

}  // namespace

extern "C" int simq_local_state_images(const simq_local_map* maps, int n_maps, const float* d_masks, int n_masks,
                                       const simq_local_robot* robots, int n_robots, const simq_local_problem* problems, int n,
                                       const simq_local_channel* channels, int n_channels, void* d_desc, int64_t desc_bytes, float* d_out,
                                       int64_t out_floats, void* stream) {
    return state_images<float>("local_state_images", "local_state", maps, n_maps, d_masks, n_masks, robots, n_robots, problems, n, channels,
                               n_channels, d_desc, desc_bytes, d_out, out_floats, stream);
}

extern "C" int simq_local_state_images_bf16(const simq_local_map* maps, int n_maps, const float* d_masks, int n_masks,
                                            const simq_local_robot* robots, int n_robots, const simq_local_problem* problems, int n,
                                            const simq_local_channel* channels, int n_channels, void* d_desc, int64_t desc_bytes,
                                            uint16_t* d_out, int64_t out_elems, void* stream) {
    return state_images<uint16_t>("local_state_images_bf16", "local_state_bf16", maps, n_maps, d_masks, n_masks, robots, n_robots, problems, n,
                                  channels, n_channels, d_desc, desc_bytes, d_out, out_elems, stream);
}

extern "C" int simq_local_state_images_slots(const simq_local_map* maps, int n_maps, const float* d_masks, int n_masks,
                                             const simq_local_robot* robots, int n_robots, const simq_local_problem* problems, int n,
                                             const simq_local_channel* channels, int n_channels, const int64_t* slots, void* d_desc,
                                             int64_t desc_bytes, float* d_pool, int64_t pool_slots, void* stream) {
    return state_images_slots<float>("local_state_images_slots", "local_state_slots", maps, n_maps, d_masks, n_masks, robots, n_robots, problems,
                                     n, channels, n_channels, slots, d_desc, desc_bytes, d_pool, pool_slots, stream);
}

extern "C" int simq_local_state_images_slots_bf16(const simq_local_map* maps, int n_maps, const float* d_masks, int n_masks,
                                                  const simq_local_robot* robots, int n_robots, const simq_local_problem* problems, int n,
                                                  const simq_local_channel* channels, int n_channels, const int64_t* slots, void* d_desc,
                                                  int64_t desc_bytes, uint16_t* d_pool, int64_t pool_slots, void* stream) {
    return state_images_slots<uint16_t>("local_state_images_slots_bf16", "local_state_slots_bf16", maps, n_maps, d_masks, n_masks, robots,
                                        n_robots, problems, n, channels, n_channels, slots, d_desc, desc_bytes, d_pool, pool_slots, stream);
}

extern "C" int simq_local_state_images_pools(const simq_local_map* maps, int n_maps, const float* d_masks, int n_masks,
                                             const simq_local_robot* robots, int n_robots, const simq_local_problem* problems, int n,
                                             const simq_local_channel* channels, int n_channels, const simq_local_pool* pools, int n_pools,
                                             const simq_local_dest* dests, void* d_desc, int64_t desc_bytes, void* stream) {
    return state_images_pools("local_state_images_pools", maps, n_maps, d_masks, n_masks, robots, n_robots, problems, n, channels, n_channels,
                              pools, n_pools, dests, d_desc, desc_bytes, stream);
}
