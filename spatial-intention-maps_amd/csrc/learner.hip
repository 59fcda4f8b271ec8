// Learner-side kernels of the DQN TD step (reference train.py:108-141) for gfx950.
// All HBM-bound; each replaces a chain of small torch ops + a host sync in the reference:
//   q_argmax / q_gather        output.view(B,-1).max(1)[1] / .gather(1, a)     train.py:115,121-122,124 ; policies.py:64
//   scatter_next_values        next_state_values[non_final_mask] = ...         train.py:116,122
//   td_huber                   y = r + g*v ; |q-y| ; smooth_l1_loss ; dLoss/dQ  train.py:126-129 (+ autograd seed)
//   clip_sgd                   clip_grad_norm_ + optim.SGD(momentum, wd).step  train.py:133-135,186
//   replay_gather              torch.cat([transform_fn(s) for s in batch.state]).to(device)  train.py:109,112
#include "batch_abi.h"

namespace simq {

namespace {

__device__ __forceinline__ bool better(float bv, int bi, float av, int ai) {
    // true if (bv, bi) should replace (av, ai): larger value, or equal value at a smaller index (first-index tie-break).  A NaN is
    // larger than every number and equal to another NaN, as tensor.max(1) orders it: the first NaN of a row wins
    const bool bnan = bv != bv, anan = av != av;
    if (bnan || anan) return bnan && (!anan || bi < ai);
    return (bv > av) || (bv == av && bi < ai);
}

__global__ void __launch_bounds__(1024) q_argmax_kernel(const float* __restrict__ q, int n, int64_t* index, float* maxv) {
    __shared__ float sv[1024];
    __shared__ int si[1024];
    const float* row = q + (size_t)blockIdx.x * n;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += 1024) {
        float v = row[i];
        if (better(v, i, bv, bi)) { bv = v; bi = i; }
    }
    sv[threadIdx.x] = bv;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int s = 512; s >= 1; s >>= 1) {
        if (threadIdx.x < s) {
            float ov = sv[threadIdx.x + s];
            int oi = si[threadIdx.x + s];
            if (better(ov, oi, sv[threadIdx.x], si[threadIdx.x])) { sv[threadIdx.x] = ov; si[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (index) index[blockIdx.x] = si[0] == 0x7fffffff ? 0 : si[0];
        if (maxv) maxv[blockIdx.x] = sv[0];
    }
}

__global__ void q_gather_kernel(const float* __restrict__ q, int rows, int n, const int64_t* __restrict__ index,
                                float* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows) out[i] = q[(size_t)i * n + index[i]];
}

__global__ void scatter_next_values_kernel(const float* __restrict__ values, const int32_t* __restrict__ pos, int n,
                                           float* nsv, int batch) {
    // ONE block walks the rows: the zero fill completes (block barrier) before the scatter
    for (int i = threadIdx.x; i < batch; i += blockDim.x) nsv[i] = 0.f;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) nsv[pos[i]] = values[i];
}

__global__ void __launch_bounds__(256) td_huber_kernel(const float* __restrict__ q, int batch, int n,
                                                       const int64_t* __restrict__ action,
                                                       const float* __restrict__ reward,
                                                       const float* __restrict__ nsv, float gamma, float grad_scale,
                                                       float* q_sa, float* y, float* td, float* out4, float* dq) {
    __shared__ float sl[256], st[256];
    float ls = 0.f, ts = 0.f;
    for (int i = threadIdx.x; i < batch; i += 256) {
        size_t o = (size_t)i * n + action[i];
        float qv = q[o];
        float yv = reward[i] + gamma * nsv[i];
        float d = qv - yv, ad = fabsf(d);
        q_sa[i] = qv;
        y[i] = yv;
        td[i] = ad;
        ls += ad < 1.f ? 0.5f * d * d : ad - 0.5f;          // smooth_l1, beta = 1
        ts += ad;
        if (dq) dq[o] = huber_grad(d) * grad_scale;
    }
    sl[threadIdx.x] = ls;
    st[threadIdx.x] = ts;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (threadIdx.x < s) { sl[threadIdx.x] += sl[threadIdx.x + s]; st[threadIdx.x] += st[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out4[0] = sl[0]; out4[1] = st[0]; out4[2] = 0.f; out4[3] = 0.f; }
}

__global__ void __launch_bounds__(256) sumsq_kernel(const float* __restrict__ g, size_t count, double* out) {
    __shared__ double sm[256];
    double acc = 0.0;
    size_t n4 = count / 4;
    float a = 0.f;
    int k = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 v = *reinterpret_cast<const float4*>(g + i * 4);
        a += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        if (++k == 16) { acc += (double)a; a = 0.f; k = 0; }   // bound the fp32 partial
    }
    acc += (double)a;
    if (blockIdx.x == 0 && threadIdx.x < (count & 3)) {
        float v = g[n4 * 4 + threadIdx.x];
        acc += (double)v * v;
    }
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) unsafeAtomicAdd(out, sm[0]);
}

__device__ __forceinline__ void sgd_elem(float& p, float& g, float& m, float coef, float lr, float mom, float wd,
                                         int first) {
    float gg = g * coef;
    g = gg;                       // clip_grad_norm_ scales .grad in place
    gg = fmaf(wd, p, gg);         // d_p = g + wd * p
    float mm = first ? gg : fmaf(mom, m, gg);
    m = mm;
    p = fmaf(-lr, mm, p);
}

__global__ void __launch_bounds__(256) clip_sgd_kernel(float* __restrict__ p, float* __restrict__ g,
                                                       float* __restrict__ m, size_t count, float max_norm, float lr,
                                                       float mom, float wd, int first, const double* sumsq,
                                                       float* total_norm) {
    float norm = (float)sqrt(*sumsq);
    float coef = 1.f;
    if (max_norm > 0.f) {         // clamp(max_norm / (norm + 1e-6), max = 1), which keeps the NaN of a NaN norm (fminf would answer 1)
        const float c = max_norm / (norm + 1e-6f);
        coef = c > 1.f ? 1.f : c;
    }
    if (total_norm && blockIdx.x == 0 && threadIdx.x == 0) *total_norm = norm;
    size_t n4 = count / 4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 pv = *reinterpret_cast<float4*>(p + i * 4), gv = *reinterpret_cast<float4*>(g + i * 4);
        float4 mv = first ? make_float4(0, 0, 0, 0) : *reinterpret_cast<float4*>(m + i * 4);
        sgd_elem(pv.x, gv.x, mv.x, coef, lr, mom, wd, first);
        sgd_elem(pv.y, gv.y, mv.y, coef, lr, mom, wd, first);
        sgd_elem(pv.z, gv.z, mv.z, coef, lr, mom, wd, first);
        sgd_elem(pv.w, gv.w, mv.w, coef, lr, mom, wd, first);
        *reinterpret_cast<float4*>(p + i * 4) = pv;
        *reinterpret_cast<float4*>(g + i * 4) = gv;
        *reinterpret_cast<float4*>(m + i * 4) = mv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (count & 3)) {
        size_t i = n4 * 4 + threadIdx.x;
        float pv = p[i], gv = g[i], mv = first ? 0.f : m[i];
        sgd_elem(pv, gv, mv, coef, lr, mom, wd, first);
        p[i] = pv; g[i] = gv; m[i] = mv;
    }
}

__global__ void replay_gather_kernel(const float* __restrict__ ring, size_t item4, const int64_t* __restrict__ index,
                                     float* __restrict__ out) {
    const float4* src = reinterpret_cast<const float4*>(ring) + (size_t)index[blockIdx.y] * item4;
    float4* dst = reinterpret_cast<float4*>(out) + (size_t)blockIdx.y * item4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < item4; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

// The inverse of replay_gather: source row blockIdx.y goes to pool slot slots[blockIdx.y].  Any item size: a row pair whose two
// addresses agree modulo 16 bytes moves as float4 between a scalar head (up to the destination's 16-byte boundary) and a scalar tail;
// a pair that does not agree (items of 4k + r floats put most rows there) moves float by float.  A slot outside the pool is skipped:
// the host has refused those, this guards a table changed behind its back.
__global__ void __launch_bounds__(256) replay_scatter_kernel(const float* __restrict__ src, int64_t item, const int64_t* __restrict__ slots,
                                                             float* __restrict__ pool, int64_t pool_slots) {
    const int64_t slot = slots[blockIdx.y];
    if (slot < 0 || slot >= pool_slots) return;
    const float* s = src + (int64_t)blockIdx.y * item;
    float* d = pool + slot * item;
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (int64_t)gridDim.x * blockDim.x;
    int64_t head = item, n4 = 0;                                         // floats before the float4 body, float4s of the body
    if ((((uintptr_t)s ^ (uintptr_t)d) & 15) == 0) {
        head = (int64_t)((16 - ((uintptr_t)d & 15)) & 15) / 4;
        if (head > item) head = item;
        n4 = (item - head) / 4;
    }
    const float4* s4 = reinterpret_cast<const float4*>(s + head);
    float4* d4 = reinterpret_cast<float4*>(d + head);
    for (int64_t i = lane; i < n4; i += lanes) d4[i] = s4[i];
    const int64_t body_end = head + n4 * 4, rest = head + (item - body_end);
    for (int64_t i = lane; i < rest; i += lanes) {                       // the head, then the tail
        const int64_t at = i < head ? i : body_end + (i - head);
        d[at] = s[at];
    }
}

// ---- states fp32 <-> bf16 (simq_plan_options.bf16_states: a replay pool of bf16 states) ------------------------------------------------
// to_bf16 is the conversion the stem kernels apply to an fp32 state, (__bf16)v: v_cvt_pk_bf16_f32 under the kernels' float mode (round to
// nearest even, denormals kept, overflow to +-Inf, a NaN stays a NaN).  to_f32 is the exact widening: the 16 bits become the high half.
// Groups of 8 elements move as 16-byte vectors (two float4 against one uint4) where BOTH addresses reach a 16-byte boundary after the
// same number of elements; the elements before the first such group and behind the last, or all of them when the two addresses never
// agree, move one by one.
__device__ __forceinline__ uint32_t bf16_pair(float a, float b) {
    return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)a) | ((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)b) << 16);
}
__device__ __forceinline__ float bf16_widen(uint32_t bits16) { return __builtin_bit_cast(float, bits16 << 16); }

// elements before the vector body (n: no body) for a 4-byte-element pointer f and a 2-byte-element pointer h that advance together
__device__ __forceinline__ int64_t states_head(const void* f, const void* h, int64_t n) {
    const int64_t a = (int64_t)(((uintptr_t)f & 15) >> 2), b = (int64_t)(((uintptr_t)h & 15) >> 1);      // a: 0..3 floats, b: 0..7 halves past a boundary
    if (((b - a) & 3) != 0) return n;
    const int64_t head = (8 - b) & 7;
    return head < n ? head : n;
}

__global__ void __launch_bounds__(256) states_to_bf16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t n) {
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (int64_t)gridDim.x * blockDim.x;
    const int64_t head = states_head(src, dst, n), n8 = (n - head) / 8;
    const float4* s4 = reinterpret_cast<const float4*>(src + head);
    uint4* d4 = reinterpret_cast<uint4*>(dst + head);
    for (int64_t i = lane; i < n8; i += lanes) {
        const float4 lo = s4[2 * i], hi = s4[2 * i + 1];
        d4[i] = make_uint4(bf16_pair(lo.x, lo.y), bf16_pair(lo.z, lo.w), bf16_pair(hi.x, hi.y), bf16_pair(hi.z, hi.w));
    }
    const int64_t body_end = head + n8 * 8, rest = head + (n - body_end);
    for (int64_t i = lane; i < rest; i += lanes) {                       // the head, then the tail
        const int64_t at = i < head ? i : body_end + (i - head);
        dst[at] = __builtin_bit_cast(uint16_t, (__bf16)src[at]);
    }
}

__global__ void __launch_bounds__(256) states_to_f32_kernel(const uint16_t* __restrict__ src, float* __restrict__ dst, int64_t n) {
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (int64_t)gridDim.x * blockDim.x;
    const int64_t head = states_head(dst, src, n), n8 = (n - head) / 8;
    const uint4* s4 = reinterpret_cast<const uint4*>(src + head);
    float4* d4 = reinterpret_cast<float4*>(dst + head);
    for (int64_t i = lane; i < n8; i += lanes) {
        const uint4 v = s4[i];
        d4[2 * i] = make_float4(bf16_widen(v.x & 0xffffu), bf16_widen(v.x >> 16), bf16_widen(v.y & 0xffffu), bf16_widen(v.y >> 16));
        d4[2 * i + 1] = make_float4(bf16_widen(v.z & 0xffffu), bf16_widen(v.z >> 16), bf16_widen(v.w & 0xffffu), bf16_widen(v.w >> 16));
    }
    const int64_t body_end = head + n8 * 8, rest = head + (n - body_end);
    for (int64_t i = lane; i < rest; i += lanes) {
        const int64_t at = i < head ? i : body_end + (i - head);
        dst[at] = bf16_widen(src[at]);
    }
}

// ---- intention-prediction head (train.py:143-158, policies.py:97-117) ---------------------------------------------
// BCEWithLogitsLoss (mean) and its gradient:  l = max(x,0) - x*t + log(1 + exp(-|x|)) ;  dl/dx = (sigmoid(x) - t) / N
__global__ void __launch_bounds__(256) bce_logits_kernel(const float* __restrict__ x, const float* __restrict__ t, size_t n,
                                                         float inv_n, float* __restrict__ dx, double* loss_sum) {
    __shared__ double sm[256];
    double acc = 0.0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float xv = x[i], tv = t[i];
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
    if (threadIdx.x == 0) unsafeAtomicAdd(loss_sum, sm[0]);
}

// x [pixels][C] -> head [pixels][C-1], last [pixels]   (s[:, :, :-1] and s[:, :, -1:], train.py:145-146)
__global__ void split_last_channel_kernel(const float* __restrict__ x, float* __restrict__ head, float* __restrict__ last,
                                          size_t pixels, int C) {
    for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < pixels; p += (size_t)gridDim.x * blockDim.x) {
        for (int c = 0; c < C - 1; ++c) head[p * (C - 1) + c] = x[p * C + c];
        last[p] = x[p * C + C - 1];
    }
}

// out [pixels][Cs+1] = concat(state [pixels][Cs], sigmoid(logit [pixels]))   (policies.py:107-108)
__global__ void sigmoid_concat_kernel(const float* __restrict__ state, const float* __restrict__ logit, float* __restrict__ out,
                                      float* __restrict__ prob, size_t pixels, int Cs) {
    for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < pixels; p += (size_t)gridDim.x * blockDim.x) {
        for (int c = 0; c < Cs; ++c) out[p * (Cs + 1) + c] = state[p * Cs + c];
        const float xv = logit[p];
        const float e = __expf(-fabsf(xv));
        const float sig = xv >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        out[p * (Cs + 1) + Cs] = sig;
        if (prob) prob[p] = sig;
    }
}

}  // namespace

int launch_bce_logits(const float* x, const float* t, int64_t n, float* dx, double* loss_sum, hipStream_t stream) {
    SIMQ_CHECK_HIP(hipMemsetAsync(loss_sum, 0, sizeof(double), stream));
    int blocks = (int)((n + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(bce_logits_kernel, dim3(blocks), dim3(256), 0, stream, x, t, (size_t)n, (float)(1.0 / (double)n), dx, loss_sum);
    SIMQ_CHECK_LAUNCH();
    return 0;
}

int launch_split_last_channel(const float* x, float* head, float* last, int64_t pixels, int C, hipStream_t stream) {
    int blocks = (int)((pixels + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(split_last_channel_kernel, dim3(blocks), dim3(256), 0, stream, x, head, last, (size_t)pixels, C);
    SIMQ_CHECK_LAUNCH();
    return 0;
}

int launch_sigmoid_concat(const float* state, const float* logit, float* out, float* prob, int64_t pixels, int Cs, hipStream_t stream) {
    int blocks = (int)((pixels + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(sigmoid_concat_kernel, dim3(blocks), dim3(256), 0, stream, state, logit, out, prob, (size_t)pixels, Cs);
    SIMQ_CHECK_LAUNCH();
    return 0;
}

int launch_q_argmax(const float* q, int rows, int n, int64_t* index, float* maxv, hipStream_t stream) {
    if (rows == 0) return 0;
    hipLaunchKernelGGL(q_argmax_kernel, dim3(rows), dim3(1024), 0, stream, q, n, index, maxv);   // one 1024-thread block per Q-map
    SIMQ_CHECK_LAUNCH();
    return 0;
}

int launch_q_gather(const float* q, int rows, int n, const int64_t* index, float* out, hipStream_t stream) {
    if (rows == 0) return 0;
    hipLaunchKernelGGL(q_gather_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, q, rows, n, index, out);
    SIMQ_CHECK_LAUNCH();
    return 0;
}

int launch_scatter_next_values(const float* values, const int32_t* pos, int n, float* nsv, int batch,
                               hipStream_t stream) {
    SIMQ_REQUIRE(batch >= 1 && batch <= 4096 && n >= 0 && n <= batch, "scatter_next_values: batch=%d n=%d unsupported (1 <= batch <= 4096, 0 <= n <= batch)", batch, n);
    hipLaunchKernelGGL(scatter_next_values_kernel, dim3(1), dim3(1024), 0, stream, values, pos, n, nsv, batch);
    SIMQ_CHECK_LAUNCH();
    return 0;
}

int launch_td_huber(const float* q, int batch, int n, const int64_t* action, const float* reward, const float* nsv,
                    float gamma, float grad_scale, float* q_sa, float* y, float* td, float* out4, float* dq,
                    hipStream_t stream) {
    if (dq) SIMQ_CHECK_HIP(hipMemsetAsync(dq, 0, sizeof(float) * (size_t)batch * n, stream));
    hipLaunchKernelGGL(td_huber_kernel, dim3(1), dim3(256), 0, stream, q, batch, n, action, reward, nsv, gamma,
                       grad_scale, q_sa, y, td, out4, dq);
    SIMQ_CHECK_LAUNCH();
    return 0;
}

int launch_clip_sgd(float* p, float* g, float* m, int64_t count, float max_norm, float lr, float momentum, float wd,
                    int first_step, void* scratch, float* total_norm, hipStream_t stream) {
    double* sumsq = reinterpret_cast<double*>(scratch);
    SIMQ_CHECK_HIP(hipMemsetAsync(sumsq, 0, sizeof(double), stream));
    hipLaunchKernelGGL(sumsq_kernel, dim3(1024), dim3(256), 0, stream, g, (size_t)count, sumsq);
    SIMQ_CHECK_LAUNCH();
    hipLaunchKernelGGL(clip_sgd_kernel, dim3(2048), dim3(256), 0, stream, p, g, m, (size_t)count, max_norm, lr,
                       momentum, wd, first_step, sumsq, total_norm);
    SIMQ_CHECK_LAUNCH();
    return 0;
}

int launch_replay_gather(const float* ring, int64_t item_floats, const int64_t* index, int count, float* out,
                         hipStream_t stream) {
    if (count == 0) return 0;
    SIMQ_REQUIRE(item_floats % 4 == 0, "replay_gather: item size must be a multiple of 4 floats");
    size_t item4 = (size_t)item_floats / 4;
    int bx = (int)((item4 + 255) / 256);
    if (bx > 16) bx = 16;
    hipLaunchKernelGGL(replay_gather_kernel, dim3(bx, count), dim3(256), 0, stream, ring, item4, index, out);
    SIMQ_CHECK_LAUNCH();
    return 0;
}

int launch_states_to_bf16(const float* src, uint16_t* dst, int64_t n, hipStream_t stream) {
    int blocks = (int)((n / 8 + 255) / 256);
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(states_to_bf16_kernel, dim3(blocks), dim3(256), 0, stream, src, dst, n);
    SIMQ_CHECK_LAUNCH();
    note_launch("states_to_bf16");
    return 0;
}

int launch_states_to_f32(const uint16_t* src, float* dst, int64_t n, hipStream_t stream) {
    int blocks = (int)((n / 8 + 255) / 256);
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(states_to_f32_kernel, dim3(blocks), dim3(256), 0, stream, src, dst, n);
    SIMQ_CHECK_LAUNCH();
    note_launch("states_to_f32");
    return 0;
}

int launch_replay_scatter(const float* src, int64_t item_floats, const int64_t* slots, int count, float* pool, int64_t pool_slots,
                          void* d_desc, int64_t desc_bytes, hipStream_t stream) {
    SIMQ_REQUIRE(src && slots && pool && d_desc, "replay_scatter: NULL pointer");
    SIMQ_REQUIRE(count >= 1 && count <= 65535, "replay_scatter: count = %d (1 .. 65535 rows: one grid row each)", count);
    SIMQ_REQUIRE(item_floats >= 1 && item_floats <= (1 << 28), "replay_scatter: item_floats = %lld (1 .. 2^28)", (long long)item_floats);
    const int64_t item_bytes = item_floats * 4;
    SIMQ_REQUIRE(pool_slots >= 1 && pool_slots <= ((int64_t)1 << 40) / item_bytes, "replay_scatter: pool_slots = %lld (1 .. 2^40 bytes of pool)",
                 (long long)pool_slots);
    SIMQ_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)pool & 3) == 0 && ((uintptr_t)d_desc & 7) == 0,
                 "replay_scatter: d_src and d_pool must be 4-byte, d_desc 8-byte aligned");
    const int64_t need_desc = (int64_t)sizeof(int64_t) * count, src_bytes = item_bytes * count;
    SIMQ_REQUIRE(desc_bytes >= need_desc, "replay_scatter: d_desc holds %lld bytes, the slot table takes %lld", (long long)desc_bytes,
                 (long long)need_desc);
    std::vector<int64_t> sorted;
    int64_t which = 0;
    const int bad = check_slots(slots, count, pool_slots, sorted, &which);
    SIMQ_REQUIRE(bad != 1, "replay_scatter: slot %lld outside the pool of %lld", (long long)which, (long long)pool_slots);
    SIMQ_REQUIRE(bad != 2, "replay_scatter: slot %lld is named twice", (long long)which);
    int64_t hit = written_slot_in(sorted, pool, item_bytes, pool_slots, src, src_bytes);
    SIMQ_REQUIRE(hit == -1, "replay_scatter: slot %lld overlaps d_src", (long long)hit);
    hit = written_slot_in(sorted, pool, item_bytes, pool_slots, d_desc, need_desc);
    SIMQ_REQUIRE(hit == -1, "replay_scatter: slot %lld overlaps d_desc", (long long)hit);
    SIMQ_REQUIRE(!overlaps(src, src_bytes, d_desc, need_desc), "replay_scatter: d_src overlaps d_desc");

    const HostBlock table = {slots, (size_t)need_desc};
    SIMQ_CHECK_HIP(upload_descriptors(d_desc, &table, 1, nullptr, stream));
    int bx = (int)((item_floats / 4 + 255) / 256);                       // (as replay_gather: up to 16 blocks of 256 lanes per row)
    bx = bx < 1 ? 1 : (bx > 16 ? 16 : bx);
    hipLaunchKernelGGL(replay_scatter_kernel, dim3(bx, count), dim3(256), 0, stream, src, item_floats, static_cast<const int64_t*>(d_desc), pool,
                       pool_slots);
    SIMQ_CHECK_LAUNCH();
    note_launch("replay_scatter");
    return 0;
}

}  // namespace simq
