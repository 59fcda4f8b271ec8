// libsimq: batched Q-map visualisations -- the state and output panels the training loop hands to tensorboard
//   state_output_kernel      get_state_output_visualization: panels and vertical bars                utils.py:116-131
//                            get_state_visualization / get_overhead_image                            utils.py:103-111
//                            scale_min_max, to_uint8_image, get_output_visualization                 utils.py:97-101, 113-114
//                            the transpose((2, 0, 1)) of its caller                                  train.py:292-304
//
// Exactness.  Everything the reference computes here is float32, one numpy operation per difference, quotient, product and sum (numpy >= 2:
// the python scalars 1e-6, 255.0, alpha and 1 - alpha become float32 before they meet the array).  The arithmetic is compiled with
// contraction off (hipcc would fuse the blend's second product into the sum: invisible at alpha = 0.5, one ulp off elsewhere) and the
// division is the compiler's correctly rounded one: 255 * x lands within an ulp of k + 0.5 often enough that a reciprocal multiply picks
// the neighbouring colour.  rintf rounds half to even, as np.round does.
//
// Shape.  One workgroup of 1024 lanes per problem.  Phase 1 reduces the minimum and the maximum of the whole [n][96][96] output (wave
// shuffles, then LDS across the 16 waves; no atomics, no workspace); phase 2 walks the flattened index of the image so that consecutive
// lanes write consecutive floats, in either layout.  The colour map sits in LDS (3 KB).
#include "batch_abi.h"
#include "../../include/simq.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace simq {

namespace {

constexpr int kW = SIMQ_STATE_WIDTH;              // 96
constexpr int kPix = kW * kW;                     // 9216
constexpr int kMaxOutputs = SIMQ_VISUALIZATION_MAX_OUTPUTS;
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kJet = 256 * 3;

// width of the image of an output with n channels: the state panel, a bar, n panels with a bar between two of them
constexpr int image_width(int n) { return kW + 1 + kW * n + (n - 1); }

// to_uint8_image(scale_min_max(.)) of one value: the difference, the quotient and the product each rounded to fp32 on its own
__device__ __forceinline__ int colour_index(float v, float mn, float d) {
#pragma clang fp contract(off)
    const float x = (v - mn) / d;
    const float t = rintf(255.f * x);
    return (int)fminf(fmaxf(t, 0.f), 255.f);      // (finite outputs give 0 .. 255 already; a NaN gives 0)
}

// get_output_visualization of one colour: hipcc contracts a * b + c * d into a product and v_fma_f32 by default
__device__ __forceinline__ float blend(float one_minus_alpha, float overhead, float alpha, float colour) {
#pragma clang fp contract(off)
    const float a = one_minus_alpha * overhead;
    const float b = alpha * colour;
    return a + b;
}

__global__ void __launch_bounds__(kThreads) state_output_kernel(const simq_visualization_problem* __restrict__ probs,
                                                                const float* __restrict__ jet_table, float alpha, float one_minus_alpha,
                                                                int chw, float* __restrict__ out) {
    __shared__ float jet[kJet];
    __shared__ float wave_min[kWaves], wave_max[kWaves];
    __shared__ float range[2];                    // the output's minimum, and (max - min) + 1e-6
    const simq_visualization_problem p = probs[blockIdx.x];              // (uniform over the workgroup)
    const int tid = threadIdx.x, n = p.n, C = p.channels;
    const float* __restrict__ state = p.d_state;
    const float* __restrict__ output = p.d_output;

    if (tid < kJet) jet[tid] = jet_table[tid];
    float lo = INFINITY, hi = -INFINITY;
    for (int k = tid; k < n * kPix; k += kThreads) {
        const float v = output[k];
        lo = min_nan(lo, v);
        hi = max_nan(hi, v);
    }
    lo = wave_reduce(lo, min_nan);                // (a NaN in the output stays: NaN everywhere, and k = 0 below)
    hi = wave_reduce(hi, max_nan);
    if ((tid & 63) == 0) {
        wave_min[tid >> 6] = lo;
        wave_max[tid >> 6] = hi;
    }
    __syncthreads();
    if (tid == 0) {
        const float a = reduce_waves(wave_min, kWaves, min_nan), b = reduce_waves(wave_max, kWaves, max_nan);
        range[0] = a;
        range[1] = (b - a) + 1e-6f;
    }
    __syncthreads();
    const float mn = range[0], d = range[1];

    // the state panel's three channels (get_state_visualization)
    const int ch0 = C >= 2 ? 1 : 0, ch2 = C >= 3 ? C - 1 : 0;
    const int W = image_width(n), items = kW * W * 3;
    float* o = out + p.out_offset;
    for (int it = tid; it < items; it += kThreads) {
        int i, w, c;
        if (chw) {
            c = it / (kW * W);
            const int r = it - c * (kW * W);
            i = r / W;
            w = r - i * W;
        } else {
            const int pix = it / 3;
            c = it - pix * 3;
            i = pix / W;
            w = pix - i * W;
        }
        float v = 0.f;                            // (the vertical bars)
        if (w < kW) {
            v = state[(i * kW + w) * C + (c == 0 ? ch0 : (c == 1 ? 0 : ch2))];
        } else if (w > kW) {
            const int q = (w - (kW + 1)) / (kW + 1), j = (w - (kW + 1)) - q * (kW + 1);
            if (j < kW) {
                const int k = colour_index(output[q * kPix + i * kW + j], mn, d);
                v = blend(one_minus_alpha, state[(i * kW + j) * C], alpha, jet[k * 3 + c]);
            }
        }
        o[it] = v;
    }
}

}  // namespace

}  // namespace simq

using namespace simq;

extern "C" int simq_state_output_visualizations(const simq_visualization_problem* problems, int n_problems,
                                                simq_visualization_problem* d_problems, const float* d_jet, double alpha, int chw,
                                                float* d_out, int64_t out_floats, void* stream) {
    SIMQ_REQUIRE(problems && d_problems && d_jet && d_out, "state_output_visualizations: NULL pointer");
    SIMQ_REQUIRE(n_problems >= 1 && n_problems <= (1 << 20), "state_output_visualizations: n_problems = %d (1 .. 2^20 problems)", n_problems);
    SIMQ_REQUIRE(std::isfinite(alpha), "state_output_visualizations: alpha is not finite");
    SIMQ_REQUIRE(chw == 0 || chw == 1, "state_output_visualizations: chw = %d (0: [96][W][3], 1: [3][96][W])", chw);
    SIMQ_REQUIRE(out_floats >= 0 && out_floats < (1LL << 40), "state_output_visualizations: out_floats = %lld (in [0, 2^40))",
                 (long long)out_floats);
    SIMQ_REQUIRE(((uintptr_t)d_problems & 7) == 0 && ((uintptr_t)d_jet & 3) == 0 && ((uintptr_t)d_out & 3) == 0,
                 "state_output_visualizations: d_problems must be 8-byte, d_jet and d_out 4-byte aligned");
    const uintptr_t top = (uintptr_t)1 << 63;
    const int64_t prob_bytes = (int64_t)sizeof(simq_visualization_problem) * n_problems;
    SIMQ_REQUIRE((uintptr_t)d_out < top && (uintptr_t)d_jet < top && (uintptr_t)d_problems < top,
                 "state_output_visualizations: a buffer address is not below 2^63");
    std::vector<Span> images, inputs;             // what the launch writes / what it reads
    images.reserve((size_t)n_problems);
    inputs.reserve(2 * (size_t)n_problems + 2);
    for (int i = 0; i < n_problems; ++i) {
        const simq_visualization_problem& p = problems[i];
        SIMQ_REQUIRE(p.n >= 1 && p.n <= kMaxOutputs, "state_output_visualizations: problem %d: n = %d (1 .. %d output channels)", i, p.n,
                     kMaxOutputs);
        SIMQ_REQUIRE(p.channels >= 1 && p.channels <= SIMQ_LOCAL_MAX_CHANNELS,
                     "state_output_visualizations: problem %d: channels = %d (1 .. %d state channels)", i, p.channels, SIMQ_LOCAL_MAX_CHANNELS);
        SIMQ_REQUIRE(p.d_state && p.d_output, "state_output_visualizations: problem %d: NULL d_state or d_output", i);
        SIMQ_REQUIRE(((uintptr_t)p.d_state & 3) == 0 && ((uintptr_t)p.d_output & 3) == 0,
                     "state_output_visualizations: problem %d: d_state and d_output must be 4-byte aligned", i);
        SIMQ_REQUIRE((uintptr_t)p.d_state < top && (uintptr_t)p.d_output < top,
                     "state_output_visualizations: problem %d: a buffer address is not below 2^63", i);
        const int64_t floats = (int64_t)kW * image_width(p.n) * 3;
        SIMQ_REQUIRE(fits(p.out_offset, floats, out_floats),
                     "state_output_visualizations: problem %d: image floats [%lld, %lld) outside the %lld of d_out", i, (long long)p.out_offset,
                     (long long)(p.out_offset + floats), (long long)out_floats);
        const uintptr_t o = (uintptr_t)(d_out + p.out_offset), s = (uintptr_t)p.d_state, q = (uintptr_t)p.d_output;
        images.push_back({o, o + 4 * (uintptr_t)floats, i});
        inputs.push_back({s, s + 4 * (uintptr_t)kPix * (uintptr_t)p.channels, i});
        inputs.push_back({q, q + 4 * (uintptr_t)kPix * (uintptr_t)p.n, i});
    }
    inputs.push_back({(uintptr_t)d_jet, (uintptr_t)d_jet + 4 * (uintptr_t)kJet, -1});
    inputs.push_back({(uintptr_t)d_problems, (uintptr_t)d_problems + (uintptr_t)prob_bytes, -2});
    const size_t clash = first_overlap(images);
    SIMQ_REQUIRE(clash == 0, "state_output_visualizations: the images of problems %d and %d share memory in d_out",
                 images[clash - 1].problem, images[clash].problem);
    // the images are sorted and disjoint: an input overlaps one of them iff it overlaps the last image that begins before the input ends
    for (const Span& in : inputs) {
        auto it = std::lower_bound(images.begin(), images.end(), Span{in.hi, 0, 0}, span_before);
        if (it == images.begin()) continue;
        --it;
        SIMQ_REQUIRE(it->hi <= in.lo, "state_output_visualizations: the image of problem %d overlaps %s%s", it->problem,
                     in.problem == -1 ? "d_jet" : (in.problem == -2 ? "d_problems" : "an input (state or output) of problem "),
                     in.problem >= 0 ? std::to_string(in.problem).c_str() : "");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const HostBlock block = {problems, (size_t)prob_bytes};
    SIMQ_CHECK_HIP(upload_descriptors(d_problems, &block, 1, nullptr, s));
    state_output_kernel<<<n_problems, kThreads, 0, s>>>(d_problems, d_jet, (float)alpha, (float)(1.0 - alpha), chw, d_out);
    SIMQ_CHECK_LAUNCH();
    note_launch("state_output_visualization");
    return 0;
}
