// Intention-prediction head over typed states (train.py:143-158, policies.py:97-117): the three kernels of simq_train_intention_step and of
// DQNIntentionPolicy on bf16 replay pools.  All HBM-bound.
//   intention_split      s[:, :, :-1] and s[:, :, -1] of a [pixels][C] state, fp32 or bf16 in, fp32 or bf16 head out     train.py:145-146
//   bce_state            BCEWithLogitsLoss against the last state channel read in place, loss summed without atomics      train.py:149-150
//   sigmoid_concat_x     concat(state, sigmoid(logit)), the element types of state and out chosen independently          policies.py:107-108
// Split and concat move a tile of kTile pixels per block.  kTile * C elements are a whole number of 16-byte vectors for every C and both
// element sizes, so with 16-byte aligned arrays every full tile is loaded as uint4, staged through LDS and stored as uint4; the last,
// partial tile and arrays that are not 16-byte aligned move element by element (consecutive lanes still write consecutive elements).
#include "batch_abi.h"

namespace simq {

namespace {

constexpr int kTile = 256;               // pixels per block (= lanes per block)
constexpr int kBceBlocks = 1024;         // most per-block partial sums of bce_state (its scratch holds this many doubles)

// one element, as its bits, from the input type to the output type: same type -- the bits (NaN payloads kept); fp32 -> bf16 -- the stem
// kernels' (__bf16)v, as states_to_bf16_kernel; bf16 -> fp32 -- the exact widening
template <bool IN16, bool OUT16>
__device__ __forceinline__ uint32_t cvt_bits(uint32_t b) {
    if (IN16 == OUT16) return b;
    if (OUT16) return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)__builtin_bit_cast(float, b));
    return b << 16;
}

template <bool IS16>
__device__ __forceinline__ uint32_t load_bits(const void* base, int64_t i) {
    return IS16 ? (uint32_t)static_cast<const uint16_t*>(base)[i] : static_cast<const uint32_t*>(base)[i];
}

template <bool IS16>
__device__ __forceinline__ void store_bits(void* base, int64_t i, uint32_t b) {
    if (IS16) static_cast<uint16_t*>(base)[i] = (uint16_t)b;
    else static_cast<uint32_t*>(base)[i] = b;
}

// OUT16 ? 8 : 4 consecutive output elements (their bits) as one 16-byte vector
template <bool OUT16>
__device__ __forceinline__ uint4 pack_vec(const uint32_t* e) {
    if (OUT16) return make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
    return make_uint4(e[0], e[1], e[2], e[3]);
}

__device__ __forceinline__ float sigmoid_of(float xv) {      // the expression of sigmoid_concat_kernel / bce_logits_kernel (learner.hip)
    const float e = __expf(-fabsf(xv));
    return xv >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// ---- split ---------------------------------------------------------------------------------------------------------------------------
// state [pixels][C] -> head [pixels][C-1] (+ last [pixels] fp32 unless NULL).  One block per tile of kTile pixels; dynamic LDS:
// kTile * C input elements (vec: 0 bytes are touched otherwise).
template <bool IN16, bool OUT16>
__global__ void __launch_bounds__(kTile) intention_split_kernel(const void* __restrict__ state, void* __restrict__ head, float* __restrict__ last,
                                                                int64_t pixels, int C, int vec) {
    extern __shared__ uint4 tile4[];
    const int64_t p0 = (int64_t)blockIdx.x * kTile;
    const int npx = (int)(pixels - p0 < kTile ? pixels - p0 : kTile);
    const int Ch = C - 1, tid = threadIdx.x;
    if (vec && npx == kTile) {
        constexpr int IN_EPV = IN16 ? 8 : 4, OUT_EPV = OUT16 ? 8 : 4;      // elements per 16-byte vector
        const int nvin = kTile / IN_EPV * C, nvout = kTile / OUT_EPV * Ch;
        const uint4* src4 = static_cast<const uint4*>(state) + (int64_t)blockIdx.x * nvin;
        for (int v = tid; v < nvin; v += kTile) tile4[v] = src4[v];
        __syncthreads();
        const void* tile = tile4;
        uint4* dst4 = static_cast<uint4*>(head) + (int64_t)blockIdx.x * nvout;
        for (int v = tid; v < nvout; v += kTile) {
            const int o = v * OUT_EPV;
            int p = o / Ch, ch = o - p * Ch;
            uint32_t e[OUT_EPV];
#pragma unroll
            for (int k = 0; k < OUT_EPV; ++k) {
                e[k] = cvt_bits<IN16, OUT16>(load_bits<IN16>(tile, p * C + ch));
                if (++ch == Ch) { ch = 0; ++p; }
            }
            dst4[v] = pack_vec<OUT16>(e);
        }
        if (last && tid < kTile / 4) {
            uint32_t e[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) e[k] = cvt_bits<IN16, false>(load_bits<IN16>(tile, (4 * tid + k) * C + Ch));
            reinterpret_cast<uint4*>(last + p0)[tid] = pack_vec<false>(e);
        }
        return;
    }
    const int64_t in0 = p0 * C, out0 = p0 * Ch;
    for (int o = tid; o < npx * Ch; o += kTile) {
        const int p = o / Ch, ch = o - p * Ch;
        store_bits<OUT16>(head, out0 + o, cvt_bits<IN16, OUT16>(load_bits<IN16>(state, in0 + (int64_t)p * C + ch)));
    }
    if (last && tid < npx) store_bits<false>(last, p0 + tid, cvt_bits<IN16, false>(load_bits<IN16>(state, in0 + (int64_t)tid * C + Ch)));
}

// ---- concat --------------------------------------------------------------------------------------------------------------------------
// out [pixels][Cs+1] = concat(state [pixels][Cs], sigmoid(logit [pixels])), prob [pixels] fp32 unless NULL.  Dynamic LDS (vec): kTile * Cs
// input elements (a whole number of 16-byte vectors), then kTile floats of sigmoids.
template <bool IN16, bool OUT16>
__global__ void __launch_bounds__(kTile) sigmoid_concat_x_kernel(const void* __restrict__ state, const float* __restrict__ logit,
                                                                 void* __restrict__ out, float* __restrict__ prob, int64_t pixels, int Cs, int vec) {
    extern __shared__ uint4 tile4[];
    const int64_t p0 = (int64_t)blockIdx.x * kTile;
    const int npx = (int)(pixels - p0 < kTile ? pixels - p0 : kTile);
    const int Co = Cs + 1, tid = threadIdx.x;
    if (vec && npx == kTile) {
        constexpr int IN_EPV = IN16 ? 8 : 4, OUT_EPV = OUT16 ? 8 : 4;
        const int nvin = kTile / IN_EPV * Cs, nvout = kTile / OUT_EPV * Co;
        const uint4* src4 = static_cast<const uint4*>(state) + (int64_t)blockIdx.x * nvin;
        for (int v = tid; v < nvin; v += kTile) tile4[v] = src4[v];
        float* sig = reinterpret_cast<float*>(tile4 + nvin);
        if (tid < kTile / 4) {
            const float4 x = reinterpret_cast<const float4*>(logit + p0)[tid];
            const float4 s = make_float4(sigmoid_of(x.x), sigmoid_of(x.y), sigmoid_of(x.z), sigmoid_of(x.w));
            reinterpret_cast<float4*>(sig)[tid] = s;
            if (prob) reinterpret_cast<float4*>(prob + p0)[tid] = s;
        }
        __syncthreads();
        const void* tile = tile4;
        uint4* dst4 = static_cast<uint4*>(out) + (int64_t)blockIdx.x * nvout;
        for (int v = tid; v < nvout; v += kTile) {
            const int o = v * OUT_EPV;
            int p = o / Co, ch = o - p * Co;
            uint32_t e[OUT_EPV];
#pragma unroll
            for (int k = 0; k < OUT_EPV; ++k) {
                if (ch < Cs) e[k] = cvt_bits<IN16, OUT16>(load_bits<IN16>(tile, p * Cs + ch));
                else e[k] = cvt_bits<false, OUT16>(__builtin_bit_cast(uint32_t, sig[p]));      // ((__bf16)sigmoid for a bf16 out: what the Q-network's stem would do to it)
                if (++ch == Co) { ch = 0; ++p; }
            }
            dst4[v] = pack_vec<OUT16>(e);
        }
        return;
    }
    const int64_t in0 = p0 * Cs, out0 = p0 * Co;
    for (int o = tid; o < npx * Co; o += kTile) {
        const int p = o / Co, ch = o - p * Co;
        uint32_t b;
        if (ch < Cs) {
            b = cvt_bits<IN16, OUT16>(load_bits<IN16>(state, in0 + (int64_t)p * Cs + ch));
        } else {
            const float s = sigmoid_of(logit[p0 + p]);
            if (prob) prob[p0 + p] = s;
            b = cvt_bits<false, OUT16>(__builtin_bit_cast(uint32_t, s));
        }
        store_bits<OUT16>(out, out0 + o, b);
    }
}

// ---- BCE against the last state channel ------------------------------------------------------------------------------------------------
// The terms and the gradient are bce_logits_kernel's expressions, element for element, with t = state[p][C-1] read in place (a bf16 state
// widened exactly).  Block b leaves the fp64 sum of its terms in partial[b]: a lane adds its terms in index order, the block folds its 256
// lanes in a fixed tree.  bce_fold_kernel then adds the partials in block order: no atomics, the same bits on every run.
template <bool IN16>
__global__ void __launch_bounds__(256) bce_state_kernel(const float* __restrict__ x, const void* __restrict__ state, size_t n, int C,
                                                        float inv_n, float* __restrict__ dx, double* __restrict__ partial) {
    __shared__ double sm[256];
    double acc = 0.0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float xv = x[i], tv = __builtin_bit_cast(float, cvt_bits<IN16, false>(load_bits<IN16>(state, (int64_t)i * C + C - 1)));
        const float e = __expf(-fabsf(xv));
        acc += (double)(fmaxf(xv, 0.f) - xv * tv + log1pf(e));
        const float sig = xv >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        if (dx) dx[i] = (sig - tv) * inv_n;
    }
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sm[0];
}

// one block: lane t adds partials [4t, 4t + 4) in order, lane 0 then adds the 256 lane sums in order
__global__ void __launch_bounds__(256) bce_fold_kernel(const double* __restrict__ partial, int count, double* __restrict__ loss_sum) {
    __shared__ double sm[256];
    double acc = 0.0;
    for (int k = 0; k < kBceBlocks / 256; ++k) {
        const int i = threadIdx.x * (kBceBlocks / 256) + k;
        if (i < count) acc += partial[i];
    }
    sm[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int t = 0; t < 256; ++t) total += sm[t];
        *loss_sum = total;
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int64_t bce_state_scratch_bytes() { return (int64_t)kBceBlocks * sizeof(double); }

int launch_intention_split(const void* state, int state_bf16, void* head, int head_bf16, float* last, int64_t pixels, int C, hipStream_t stream) {
    const size_t lds = (size_t)kTile * C * (state_bf16 ? 2 : 4);
    // (a tile that does not fit 64 KB of LDS -- C > 64 fp32 channels -- moves element by element like an unaligned one)
    const int vec = aligned16(state) && aligned16(head) && (!last || aligned16(last)) && lds <= 65536;
    const dim3 grid((unsigned)((pixels + kTile - 1) / kTile)), block(kTile);
    const size_t shm = vec ? lds : 0;
    if (state_bf16 && head_bf16) hipLaunchKernelGGL((intention_split_kernel<true, true>), grid, block, shm, stream, state, head, last, pixels, C, vec);
    else if (state_bf16) hipLaunchKernelGGL((intention_split_kernel<true, false>), grid, block, shm, stream, state, head, last, pixels, C, vec);
    else if (head_bf16) hipLaunchKernelGGL((intention_split_kernel<false, true>), grid, block, shm, stream, state, head, last, pixels, C, vec);
    else hipLaunchKernelGGL((intention_split_kernel<false, false>), grid, block, shm, stream, state, head, last, pixels, C, vec);
    SIMQ_CHECK_LAUNCH();
    note_launch("intention_split");
    return 0;
}

int launch_sigmoid_concat_x(const void* state, int state_bf16, const float* logit, void* out, int out_bf16, float* prob, int64_t pixels, int Cs,
                            hipStream_t stream) {
    const size_t lds = (size_t)kTile * Cs * (state_bf16 ? 2 : 4) + kTile * sizeof(float);
    const int vec = aligned16(state) && aligned16(logit) && aligned16(out) && (!prob || aligned16(prob)) && lds <= 65536;
    const dim3 grid((unsigned)((pixels + kTile - 1) / kTile)), block(kTile);
    const size_t shm = vec ? lds : 0;
    if (state_bf16 && out_bf16) hipLaunchKernelGGL((sigmoid_concat_x_kernel<true, true>), grid, block, shm, stream, state, logit, out, prob, pixels, Cs, vec);
    else if (state_bf16) hipLaunchKernelGGL((sigmoid_concat_x_kernel<true, false>), grid, block, shm, stream, state, logit, out, prob, pixels, Cs, vec);
    else if (out_bf16) hipLaunchKernelGGL((sigmoid_concat_x_kernel<false, true>), grid, block, shm, stream, state, logit, out, prob, pixels, Cs, vec);
    else hipLaunchKernelGGL((sigmoid_concat_x_kernel<false, false>), grid, block, shm, stream, state, logit, out, prob, pixels, Cs, vec);
    SIMQ_CHECK_LAUNCH();
    note_launch("sigmoid_concat_x");
    return 0;
}

int launch_bce_state(const float* x, const void* state, int state_bf16, int64_t n, int C, float* dx, double* loss_sum, void* scratch,
                     hipStream_t stream) {
    int blocks = (int)((n + 255) / 256);
    if (blocks > kBceBlocks) blocks = kBceBlocks;
    double* partial = static_cast<double*>(scratch);
    const float inv_n = (float)(1.0 / (double)n);
    if (state_bf16) hipLaunchKernelGGL((bce_state_kernel<true>), dim3(blocks), dim3(256), 0, stream, x, state, (size_t)n, C, inv_n, dx, partial);
    else hipLaunchKernelGGL((bce_state_kernel<false>), dim3(blocks), dim3(256), 0, stream, x, state, (size_t)n, C, inv_n, dx, partial);
    SIMQ_CHECK_LAUNCH();
    hipLaunchKernelGGL(bce_fold_kernel, dim3(1), dim3(256), 0, stream, partial, blocks, loss_sum);
    SIMQ_CHECK_LAUNCH();
    note_launch("bce_state");
    return 0;
}

}  // namespace simq
