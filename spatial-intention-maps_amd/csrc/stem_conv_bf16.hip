// First convolution of the encoder (reference resnet.py:94: conv 7x7, stride 2, pad 3, Cin = 3..9 (wide-row form: 10..13) -> 64, no bias) on the bf16 matrix
// cores, for plain-bf16 plans.  The implicit-GEMM kernels need Cin % 32 == 0; with 3..9 input channels the fp32 kernel gathers its
// operands one float at a time (169 us at B = 128: 55 TF/s).  What this kernel uses instead:
//
//   * In NHWC the 7 taps x Cin channels of one filter ROW are 7*Cin CONTIGUOUS floats of x (35 at Cin = 5), starting at pixel
//     (2 oy + ky - 3, 2 ox - 3).  A row of the im2col matrix is therefore 7 contiguous runs, and the contraction becomes, per filter
//     row ky, K = 64 (7*Cin real values, zero weights behind them): two v_mfma_f32_16x16x32_bf16 k-steps.
//   * The A fragment of that MFMA is 8 consecutive k per lane = 8 consecutive floats of x: every lane loads its fragment STRAIGHT from
//     global memory (two dword-aligned global_load_dwordx4), masks the elements that fall outside the image row (left / right padding;
//     rows above / below the image are skipped per tile), converts to bf16 and feeds the matrix core.  No LDS for activations, no
//     packed copy of x.  k-groups that lie entirely behind the 7*Cin real values are not loaded (their weights are zero).
//   * The weights (64 x 7 x 64 bf16, rows padded to 456 elements: conflict-free ds_read_b128) sit in LDS for the lifetime of a block;
//     blocks are persistent (grid-stride over 16-pixel wave tiles, nine waves per block: 58 -> 42 us per launch at B = 128 against pairs of tiles on eight waves), so the weights are staged and the BatchNorm batch statistics of the
//     block (fp32 per lane -> fp64 per block) are pushed with atomics ONCE per block.
//   * Output: the pre-BatchNorm map as bf16 (like every other matrix-core convolution of a plain-bf16 plan; statistics from the fp32
//     accumulators).
//   * Cin = 10..13 (7*Cin = 70..91: simq_plan_options.stem_bf16 = 2): the same kernels with THREE k-steps per filter row
//     (K = 96, rows of 680 elements in LDS, one block of 16 waves per CU); the figures above are for Cin <= 9.
#include <cstdint>
#include <type_traits>

#include "common.h"

namespace simq {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
typedef float floatx4_a4 __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte load the compiler may not assume aligned
typedef uint16_t ushortx8_a2 __attribute__((ext_vector_type(8), aligned(2))); // ... of 8 bf16: the window starts at (2 ox - 3) * C ELEMENTS, odd for odd C

// The element type of x (simq_plan_options.bf16_states): float -- a lane's fragment is 8 floats (two 16-byte loads), masked as floats and
// rounded to bf16 -- or uint16_t -- the states ARE bf16: the fragment is ONE 16-byte load that may only assume 2-byte alignment,
// masked as 16-bit words (0 = +0.0) and handed to the matrix core as the bits lie in memory (no arithmetic touches them: NaN payloads
// and denormals pass).  Every index below counts ELEMENTS of x, never bytes, so the masks are the same code for both.
template <typename XE> struct Frag;
template <> struct Frag<float> {
    typedef float E;
    static __device__ __forceinline__ void load8(const float* src, float* v) {
        const floatx4_a4 lo = *reinterpret_cast<const floatx4_a4*>(src), hi = *reinterpret_cast<const floatx4_a4*>(src + 4);
        v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
        v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
    }
    static __device__ __forceinline__ __bf16 cvt(float v) { return (__bf16)v; }
};
template <> struct Frag<uint16_t> {
    typedef uint16_t E;
    static __device__ __forceinline__ void load8(const uint16_t* src, uint16_t* v) {
        const ushortx8_a2 w = *reinterpret_cast<const ushortx8_a2*>(src);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = w[q];
    }
    static __device__ __forceinline__ __bf16 cvt(uint16_t v) { return __builtin_bit_cast(__bf16, v); }
};

// Every kernel below carries the number of k-steps KS of a filter row as a template parameter:
//   KS = 2  the narrow form, 7 * Cin <= 63   (Cin 1..9):   KROW = 64, what every default plan launches
//   KS = 3  the wide-row form, 64 <= 7 * Cin <= 95 (Cin 10..13): KROW = 96 (simq_plan_options.stem_bf16 = 2, the *_wide entries)
constexpr int COUT = 64, R = 7;
template <int KS> struct Row {
    static constexpr int KROW = 32 * KS;               // K per filter row: 64 (7 * Cin <= 63 real) | 96 (7 * Cin <= 95 real)
    // LDS row of one output channel.  KS = 2: 456 bf16 = 228 dwords (36 mod 64: conflict-free).  KS = 3: 680 bf16 = 340 dwords = 20 mod 64:
    // a ds_read_b128 serves 16 lanes (fi = 0..15, one kg) per pass, lane fi starts at bank 20 fi mod 64 = 0 20 40 60 16 36 56 12 32 52 8
    // 28 48 4 24 44 -- sixteen different multiples of 4, four banks each: all 64 banks once, conflict-free (20 / 4 = 5 is odd)
    static constexpr int WROW = R * KROW + 8;
    static constexpr int SMEM_W = COUT * WROW * 2;     // 58 368 B | 87 040 B
    // waves per block (they share the LDS copy of the weights).  KS = 2: 9 x 512 blocks = one 16-pixel tile per wave and trip, two blocks
    // a CU, 4.5 waves per SIMD hide each other's load latency.  KS = 3: 87 KB of weights + statistics scratch no longer fit a CU's 160 KB
    // twice: ONE block of 16 waves (1024 threads, 4 waves per SIMD, 128 registers a lane) per CU -- the weights are staged once per CU
    // and x is read once (blocks owning half of the output channels would read x twice)
    static constexpr int NWAVE = KS == 2 ? 9 : 16;
    static constexpr int BLOCKS_PER_CU = KS == 2 ? 2 : 1;
    static constexpr int TILES = 2 * KS;               // 16-column tiles of a filter row in the weight gradient
};

template <typename XE>
struct StemArgs {
    const XE* x; const uint16_t* w16; uint16_t* y; double* stats;
    int B, H, W, C, Ho, Wo;
    unsigned x_bytes;
};

template <typename XE, int KS>
__global__ void __launch_bounds__(Row<KS>::NWAVE * 64, Row<KS>::BLOCKS_PER_CU) stem_conv_bf16_kernel(const StemArgs<XE> p) {
    typedef typename Frag<XE>::E E;
    constexpr int KROW = Row<KS>::KROW, WROW = Row<KS>::WROW, SMEM_W = Row<KS>::SMEM_W, NWAVE = Row<KS>::NWAVE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint16_t* wl = reinterpret_cast<uint16_t*>(smem);
    double* red = reinterpret_cast<double*>(smem + SMEM_W);          // [NWAVE][64][2]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // weights -> LDS (the prepared layout is already [cout][WROW]); all of a thread's loads before its first store
    {
        constexpr int NV = COUT * WROW / 8, TRIPS = (NV + NWAVE * 64 - 1) / (NWAVE * 64);
        uint4 v[TRIPS];
#pragma unroll
        for (int u = 0; u < TRIPS; ++u) {
            const int i = tid + u * NWAVE * 64;
            v[u] = i < NV ? reinterpret_cast<const uint4*>(p.w16)[i] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < TRIPS; ++u) {
            const int i = tid + u * NWAVE * 64;
            if (i < NV) reinterpret_cast<uint4*>(wl)[i] = v[u];
        }
    }
    __syncthreads();

    const long total = (long)p.B * p.H * p.W * p.C;                  // floats in x
    const int fi = lane & 15, kg = lane >> 4;
    const int rowf = p.W * p.C;                                      // floats per image row
    const int kreal = R * p.C;                                       // real k per filter row
    const int tiles_per_row = p.Wo / 16;
    const int ntiles = p.B * p.Ho * tiles_per_row;                   // 16-pixel tiles
    float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f};
    const uint16_t* wfrag = wl + fi * WROW + kg * 8;                  // + j * 16 * WROW + ky * KROW + s * 32

    // One wave = one 16-pixel x 64-channel tile at a time (round 3; a wave used to own a PAIR of tiles with every (filter row, k-step)
    // an exposed load latency: 58 us per launch at B = 128)
    for (int tile = blockIdx.x * NWAVE + wave; tile < ntiles; tile += gridDim.x * NWAVE) {
        floatx4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
        const int ox0 = (tile % tiles_per_row) * 16;
        const int r = tile / tiles_per_row;
        const int oy = r % p.Ho, b = r / p.Ho;
        // per lane: pointer to the first float of its k-group at filter row 0 (may lie outside the tensor: rows above / below the image
        // are skipped before it is used); per k-step whether some lane's 8-float fragment touches the left / right padding (ballot)
        const int e_lo = (2 * (ox0 + fi) - 3) * p.C + kg * 8;
        const XE* prow = p.x + ((long)(b * p.H + 2 * oy - 3) * rowf + e_lo);
        bool side[KS], real[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int e = e_lo + s * 32;
            // k-groups entirely behind the 7*Cin real values are not loaded (KS = 3: 7*Cin >= 64, the first two steps are real in every lane)
            real[s] = (KS == 3 && s < 2) || s * 32 + kg * 8 < kreal;
            side[s] = __builtin_amdgcn_ballot_w64((e < 0 || e + 8 > rowf) && real[s]) != 0;
        }
        // KS = 3: what a lane keeps of a fragment is one interval [qlo, qhi) of its 8 elements -- the left padding cuts in front, the right
        // padding and the end of the 7 * Cin real values behind.  The elements behind the real values of a partly real k-group (always in
        // the third step: 7 * Cin >= 64) are x values of the NEXT pixel; their weights are zero, but 0 * NaN is NaN, so they are cleared
        // to +0 like the padding and a NaN / Inf there reaches no output the convolution does not give it to (rules 1 and 2).
        // The interval is kept as four dword masks over the packed bf16 fragment per k-step, in vector registers: the 24 selects of the
        // narrow form's shape hold 24 loop-invariant lane masks in scalar registers, which three k-steps no longer have (spills)
        unsigned keep[KS][4];
        if constexpr (KS == 3) {
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const int e = e_lo + s * 32;
                const int qlo = max(0, -e), qhi = min(min(8, rowf - e), kreal - (s * 32 + kg * 8));
#pragma unroll
                for (int d = 0; d < 4; ++d)
                    keep[s][d] = ((2 * d >= qlo && 2 * d < qhi) ? 0xffffu : 0u) | ((2 * d + 1 >= qlo && 2 * d + 1 < qhi) ? 0xffff0000u : 0u);
            }
        }
#pragma unroll 1
        for (int ky = 0; ky < R; ++ky) {
            const int iy = 2 * oy + ky - 3;
            if ((unsigned)iy >= (unsigned)p.H) continue;                                      // wave-uniform: a padding row
            // the first row of the first image and the last row of the last: a fragment may reach outside the tensor
            const bool tensor_edge = (b == 0 && iy == 0) || (b == p.B - 1 && iy == p.H - 1);   // wave-uniform
            E v[KS][8];
            // fragments of all k-steps: 8 consecutive floats of x each, straight from global memory (dword-aligned 16-byte loads: the
            // window starts at (2 ox - 3) * C floats), all loads issued before the first mask.  (KS = 3: real[2] differs between the
            // lanes of a wave -- at Cin = 10 only k-group 0 of the third step holds real values -- so its loads are lane-divergent.)
#pragma unroll
            for (int s = 0; s < KS; ++s) {
#pragma unroll
                for (int q = 0; q < 8; ++q) v[s][q] = E(0);
                if (real[s]) {
                    const XE* src = prow + (ky * rowf + s * 32);
                    if (!tensor_edge) {
                        Frag<XE>::load8(src, v[s]);
                    } else if constexpr (KS == 2) {
                        const long g0 = src - p.x;
#pragma unroll
                        for (int q = 0; q < 8; ++q) v[s][q] = (g0 + q >= 0 && g0 + q < total) ? src[q] : E(0);
                    } else {
                        // An element outside the tensor lies left of the first row of the first image (e + q < 0) or right of the last row
                        // of the last (e + q >= rowf), where the keep masks clear it whatever was loaded: its ADDRESS is clamped into the
                        // tensor (v_max / v_min, no lane mask) and the load is unconditional.  Element indices fit 31 bits (the launcher
                        // checks).
                        const int g0 = (int)(src - p.x), last = (int)total - 1;
#pragma unroll
                        for (int q = 0; q < 8; ++q) v[s][q] = p.x[min(max(g0 + q, 0), last)];
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                if constexpr (KS == 2) {
                if (side[s]) {                                         // wave-uniform: some lane touches the left / right padding
                    const int e = e_lo + s * 32;
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[s][q] = ((unsigned)(e + q) < (unsigned)rowf) ? v[s][q] : E(0);
                }
                }
                bf16x8 af;
#pragma unroll
                for (int q = 0; q < 8; ++q) af[q] = Frag<XE>::cvt(v[s][q]);
                if constexpr (KS == 3) {                               // (a cleared element is +0.0 whatever it held, a NaN included)
                    uintx4 ab = __builtin_bit_cast(uintx4, af);
#pragma unroll
                    for (int d = 0; d < 4; ++d) ab[d] &= keep[s][d];
                    af = __builtin_bit_cast(bf16x8, ab);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bf16x8 bf = *reinterpret_cast<const bf16x8*>(wfrag + j * 16 * WROW + ky * KROW + s * 32);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[j], 0, 0, 0);
                }
            }
        }
        // ---- store (bf16) + statistics: lane holds column fi of N-tile j, rows 4 kg + r of the tile
        const size_t m0 = (size_t)tile * 16;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const float val = acc[j][r4];
                s0[j] += val; s1[j] += val * val;
                p.y[(m0 + 4 * kg + r4) * COUT + j * 16 + fi] = __builtin_bit_cast(uint16_t, (__bf16)val);
            }
    }
    if (!p.stats) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float a = s0[j], c = s1[j];
        a += __shfl_xor(a, 16); c += __shfl_xor(c, 16);
        a += __shfl_xor(a, 32); c += __shfl_xor(c, 32);
        if (kg == 0) { red[(wave * COUT + j * 16 + fi) * 2] = (double)a; red[(wave * COUT + j * 16 + fi) * 2 + 1] = (double)c; }
    }
    __syncthreads();
    if (tid < COUT) {
        double a = 0.0, c = 0.0;
#pragma unroll
        for (int w = 0; w < NWAVE; ++w) { a += red[(w * COUT + tid) * 2]; c += red[(w * COUT + tid) * 2 + 1]; }
        unsafeAtomicAdd(p.stats + tid, a);
        unsafeAtomicAdd(p.stats + COUT + tid, c);
    }
}

// w [64][7][7][C] fp32 (OHWI) -> w16 [64][WROW] bf16: element ky * KROW + kx * C + c, zeros elsewhere
template <int KS>
__global__ void stem_weight_prep_kernel(const float* __restrict__ w, uint16_t* __restrict__ w16, int C) {
    constexpr int KROW = Row<KS>::KROW, WROW = Row<KS>::WROW;
    const int total = COUT * WROW;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int o = i / WROW, e = i - o * WROW;
        const int ky = e / KROW, n = e - ky * KROW;
        float v = 0.f;
        if (ky < R && n < R * C) v = w[((size_t)o * R + ky) * R * C + n];
        w16[i] = __builtin_bit_cast(uint16_t, (__bf16)v);
    }
}

// ---- weight gradient of the same convolution -------------------------------------------------------------------------------------
//   dW[o][ky][n] = sum over output pixels of dy[pix][o] * xrow_ky[pix][n],   n = kx * C + c < 7 C
// The contraction runs over PIXELS, so the MFMA operands need 8 consecutive pixels per lane -- strided in both tensors.  Per chunk of
// 32 output pixels a block therefore stages both operands TRANSPOSED in LDS: dyT [64 o][32 pix] from the bf16 plane of dy, and for each
// filter row XT_ky [64 n][32 pix], filled by the forward kernel's fragment gather (8 consecutive floats of x per (pixel, k-group),
// padding masked, converted) with the 8 values scattered to 8 LDS rows.  After one barrier wave ky contracts its filter row:
// 4 + 4 ds_read_b128 fragments, 16 MFMAs (64 x 64 outputs over k = 32 pixels).  Blocks are persistent; every block leaves its 64 x 7 x 7C
// partial sums in a scratch slab and a second launch adds the slabs in a fixed order (deterministic; atomics over 15 680 addresses
// from 512 blocks would be neither that nor fast).
// The wide form (KS = 3): XT_ky is [96 n][32 pix] (LDS 58 880 B), wave ky contracts 64 x 96 -- six column tiles, 96 accumulator registers, one
// block per CU -- and a (pixel, filter row) has 12 k-groups, so the staging loop's slot index is divided, not shifted.
constexpr int TROW = 40;                               // LDS row: 32 pixels + 8 pad (80 B: conflict-free ds_read_b128 over 16 rows)
template <int KS> constexpr int wg_smem() { return (COUT + R * Row<KS>::KROW) * TROW * 2; }   // dyT + 7 x XT = 40 960 B | 58 880 B
constexpr int WG_WAVES = 8;

template <typename XE>
struct StemWgradArgs {
    const XE* x; const uint16_t* dy; float* partial;
    int B, H, W, C, Ho, Wo;
};

template <typename XE, int KS>
__global__ void __launch_bounds__(WG_WAVES * 64, Row<KS>::BLOCKS_PER_CU) stem_wgrad_bf16_kernel(const StemWgradArgs<XE> p) {
    typedef typename Frag<XE>::E E;
    constexpr int KROW = Row<KS>::KROW, NT = Row<KS>::TILES, NG = 4 * KS;   // columns, column tiles and k-groups of a filter row
    __shared__ __attribute__((aligned(16))) uint16_t lds[wg_smem<KS>() / 2];
    uint16_t* dyT = lds;                                // [64][TROW]
    uint16_t* XT = lds + COUT * TROW;                   // [7][KROW][TROW]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rowf = p.W * p.C, kreal = R * p.C;
    const int ngrp = (kreal + 7) / 8;                   // k-groups of a filter row that hold real values
    const long total = (long)p.B * p.H * p.W * p.C;
    const int tiles_per_row = p.Wo / 16;
    const int ntiles = p.B * p.Ho * tiles_per_row;
    const int nchunks = (ntiles + 1) / 2;
    const int fi = lane & 15, kg = lane >> 4;
    floatx4 acc[4][NT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        // ---- stage dyT: 32 pixels x 64 channels; lane -> (pixel, 8-channel group), 16-byte load, 8 scattered 2-byte stores
        if (tid < 256) {
            const int pix = tid >> 3, cg = tid & 7;
            const int tile = chunk * 2 + (pix >> 4);
            uint4 v = make_uint4(0, 0, 0, 0);
            if (tile < ntiles) v = *reinterpret_cast<const uint4*>(p.dy + ((size_t)tile * 16 + (pix & 15)) * COUT + cg * 8);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 8; ++q) dyT[(cg * 8 + q) * TROW + pix] = (uint16_t)(q & 1 ? w[q >> 1] >> 16 : w[q >> 1] & 0xffffu);
        }
        // ---- stage XT: slots (ky, tile, pixel, k-group); only the k-groups with real values (the others feed discarded columns)
        for (int f = tid; f < R * 2 * 16 * NG; f += WG_WAVES * 64) {
            int grp, i, t, ky;
            if constexpr (KS == 2) {
                grp = f & 7; i = (f >> 3) & 15; t = (f >> 7) & 1; ky = f >> 8;
            } else {
                const unsigned pix = (unsigned)f / NG;                  // 12 k-groups: no power of two
                grp = (int)((unsigned)f - pix * NG); i = pix & 15; t = (pix >> 4) & 1; ky = (int)(pix >> 5);
            }
            if (grp >= ngrp) continue;
            const int tile = chunk * 2 + t;
            E v[8] = {E(0), E(0), E(0), E(0), E(0), E(0), E(0), E(0)};
            if (tile < ntiles) {
                const int ox0 = (tile % tiles_per_row) * 16;
                const int r = tile / tiles_per_row;
                const int oy = r % p.Ho, b = r / p.Ho;
                const int iy = 2 * oy + ky - 3;
                if ((unsigned)iy < (unsigned)p.H) {
                    const int e = (2 * (ox0 + i) - 3) * p.C + grp * 8;                 // first float of the fragment inside the image row
                    const long g0 = (long)(b * p.H + iy) * rowf + e;
                    if (g0 >= 0 && g0 + 8 <= total) {
                        Frag<XE>::load8(p.x + g0, v);
                    } else {
#pragma unroll
                        for (int q = 0; q < 8; ++q) v[q] = (g0 + q >= 0 && g0 + q < total) ? p.x[g0 + q] : E(0);
                    }
                    if (e < 0 || e + 8 > rowf) {
#pragma unroll
                        for (int q = 0; q < 8; ++q) v[q] = ((unsigned)(e + q) < (unsigned)rowf) ? v[q] : E(0);   // left / right padding
                    }
                }
            }
            uint16_t* dst = XT + (ky * KROW + grp * 8) * TROW + t * 16 + i;
#pragma unroll
            for (int q = 0; q < 8; ++q) dst[q * TROW] = __builtin_bit_cast(uint16_t, Frag<XE>::cvt(v[q]));
        }
        __syncthreads();
        // ---- wave ky: out[o][n] += sum over the 32 pixels of dyT[o][pix] * XT_ky[n][pix]
        if (wave < R) {
            bf16x8 af[4], bf[NT];
            if constexpr (KS == 2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    af[j] = *reinterpret_cast<const bf16x8*>(dyT + (j * 16 + fi) * TROW + kg * 8);
                    bf[j] = *reinterpret_cast<const bf16x8*>(XT + (wave * KROW + j * 16 + fi) * TROW + kg * 8);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) af[j] = *reinterpret_cast<const bf16x8*>(dyT + (j * 16 + fi) * TROW + kg * 8);
#pragma unroll
                for (int j = 0; j < NT; ++j) bf[j] = *reinterpret_cast<const bf16x8*>(XT + (wave * KROW + j * 16 + fi) * TROW + kg * 8);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // ---- this block's partial sums: slab [64 o][7 ky][7 C]; lane holds out[o = i * 16 + 4 kg + r][n = j * 16 + fi]
    if (wave < R) {
        float* slab = p.partial + (size_t)blockIdx.x * COUT * R * kreal;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int o = i * 16 + 4 * kg + r, n = j * 16 + fi;
                    if (n < kreal) slab[((size_t)o * R + wave) * kreal + n] = acc[i][j][r];
                }
    }
}

// dw[e] = sum over the slabs (overwrites dw): 64 outputs x 4 slab lanes per block -- lane q adds slabs q, q + 4, ... (four loads in
// flight), the four partial sums are combined in lane order: a fixed summation tree, the same bits on every run
__global__ void __launch_bounds__(256) stem_wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw, int n, int slabs) {
    __shared__ float sm[256];
    const int e = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (e < n) {
        int s = q;
        for (; s + 12 < slabs; s += 16) {
            a0 += partial[(size_t)s * n + e]; a1 += partial[(size_t)(s + 4) * n + e];
            a2 += partial[(size_t)(s + 8) * n + e]; a3 += partial[(size_t)(s + 12) * n + e];
        }
        for (; s < slabs; s += 4) a0 += partial[(size_t)s * n + e];
    }
    sm[threadIdx.x] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (q == 0 && e < n) dw[e] = (sm[threadIdx.x] + sm[threadIdx.x + 64]) + (sm[threadIdx.x + 128] + sm[threadIdx.x + 192]);
}

}  // namespace

// slabs the weight-gradient launch will use for this batch (the caller provides slabs * 64 * 49 * C floats of scratch)
int stem_wgrad_bf16_slabs(int B, int H, int W) {
    const int nchunks = (B * (H / 2) * (W / 32) + 1) / 2;
    int blocks = (nchunks + 7) / 8;                                   // >= 8 chunks per block
    if (blocks > 512) blocks = 512;
    if (blocks < 1) blocks = 1;
    return blocks;
}

// ... when the scratch it is given holds capacity_bytes (< 0: as much as it asks for): never more slabs than fit, 0 when not even one
// does.  (A workspace slot holds B * 1 179 648 bytes and 9 B slabs of 12 544 C bytes fit it up to C = 10 and no further: DESIGN 26.)
int stem_wgrad_bf16_slabs_cap(int B, int H, int W, int C, int64_t capacity_bytes) {
    int slabs = stem_wgrad_bf16_slabs(B, H, W);
    if (capacity_bytes >= 0 && C >= 1) {
        const int64_t fit = capacity_bytes / ((int64_t)COUT * R * R * C * (int64_t)sizeof(float));
        if (fit < slabs) slabs = (int)fit;
    }
    return slabs;
}

// k-steps per filter row of the form that serves this convolution: 2 (7 * C <= 63), 3 (the wide-row form, 64 <= 7 * C <= 95), 0 = not served
int stem_conv_bf16_ksteps(int H, int W, int C, int cout, int k, int stride, int pad) {
    if (cout != COUT || k != R || stride != 2 || pad != 3 || C < 1 || H % 2 != 0 || W % 32 != 0) return 0;
    return R * C <= Row<2>::KROW - 1 ? 2 : R * C <= Row<3>::KROW - 1 ? 3 : 0;
}

namespace {

// The launch family of an operator, a row width and an input type, for the launch log and the refusal texts: the operator, + "_wide" for
// three k-steps, + "_x16" over bf16 states.  (String literals: the launch log keeps the pointer.)
#define SIMQ_STEM_FAMILIES(op) {op, op "_x16", op "_wide", op "_wide_x16"}
const char* stem_family(bool wgrad, int ks, bool bf16) {
    static const char* const names[2][4] = {SIMQ_STEM_FAMILIES("stem_conv_bf16"), SIMQ_STEM_FAMILIES("stem_wgrad_bf16")};
    return names[wgrad ? 1 : 0][(ks == 3 ? 2 : 0) + (bf16 ? 1 : 0)];
}
#undef SIMQ_STEM_FAMILIES

// The one place where (input type, row width) become template arguments: f(x as a pointer to its element type, the k-steps as a type),
// once ks is what the shape takes
template <int KS> using KSteps = std::integral_constant<int, KS>;
template <typename F>
int stem_dispatch(const char* family, StemX x, int ks, int H, int W, int C, F f) {
    SIMQ_REQUIRE(ks != 0 && stem_conv_bf16_ksteps(H, W, C, COUT, R, 2, 3) == ks, "%s: shape %dx%dx%d not covered", family, H, W, C);
    const float* xf = static_cast<const float*>(x.p);
    const uint16_t* x16 = static_cast<const uint16_t*>(x.p);
    if (ks == 2) return !x.bf16 ? f(xf, KSteps<2>()) : f(x16, KSteps<2>());
    return !x.bf16 ? f(xf, KSteps<3>()) : f(x16, KSteps<3>());
}

template <int KS, typename XE>
int stem_wgrad_bf16_impl(const char* family, const XE* x, const uint16_t* dy, float* dw, float* partial, int B, int H, int W, int C, hipStream_t stream,
                         int64_t partial_bytes) {
    SIMQ_REQUIRE(4.0 * B * H * W * C < 4294967000.0, "%s: input too large", family);     // (elements: the kernels index them with 31 bits to spare)
    StemWgradArgs<XE> p;
    p.x = x; p.dy = dy; p.partial = partial;
    p.B = B; p.H = H; p.W = W; p.C = C; p.Ho = H / 2; p.Wo = W / 2;
    // blocks are persistent over the chunks, so any slab count covers the batch: as many as the scratch holds, at most what the batch asks for
    const int slabs = stem_wgrad_bf16_slabs_cap(B, H, W, C, partial_bytes);
    SIMQ_REQUIRE(slabs >= 1, "%s: the partial-sum scratch holds %lld bytes, one slab of %d input channels takes %d", family, (long long)partial_bytes, C,
                 COUT * R * R * C * (int)sizeof(float));
    note_launch(family);
    hipLaunchKernelGGL((stem_wgrad_bf16_kernel<XE, KS>), dim3(slabs), dim3(WG_WAVES * 64), 0, stream, p);
    SIMQ_CHECK_LAUNCH();
    const int n = COUT * R * R * C;
    hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3((n + 63) / 64), dim3(256), 0, stream, partial, dw, n, slabs);
    SIMQ_CHECK_LAUNCH();
    return 0;
}

}  // namespace

// dy: bf16 [B][H/2][W/2][64];  dw: [64][7][7][C] fp32 (overwritten);  partial: stem_wgrad_bf16_slabs_cap(.., partial_bytes) * 64 * 49 * C floats
int launch_stem_wgrad_bf16(StemX x, int ks, const uint16_t* dy, float* dw, float* partial, int B, int H, int W, int C, hipStream_t stream,
                           int64_t partial_bytes) {
    const char* family = stem_family(true, ks, x.bf16);
    return stem_dispatch(family, x, ks, H, W, C, [&](auto* xe, auto k) {
        return stem_wgrad_bf16_impl<decltype(k)::value>(family, xe, dy, dw, partial, B, H, W, C, stream, partial_bytes);
    });
}

// bytes of the prepared weights: [64][WROW] bf16 (58 368 | 87 040)
int stem_conv_bf16_wbytes(int ks) { return COUT * (ks == 3 ? Row<3>::WROW : Row<2>::WROW) * 2; }

int launch_stem_weight_prep(const float* w, uint16_t* w16, int C, int ks, hipStream_t stream) {
    SIMQ_REQUIRE(ks == 2 || ks == 3, "stem_weight_prep: %d k-steps per filter row (2 or 3)", ks);
    void (*prep)(const float*, uint16_t*, int) = ks == 2 ? stem_weight_prep_kernel<2> : stem_weight_prep_kernel<3>;
    hipLaunchKernelGGL(prep, dim3(32), dim3(256), 0, stream, w, w16, C);
    SIMQ_CHECK_LAUNCH();
    return 0;
}

namespace {

template <int KS, typename XE>
int stem_conv_bf16_impl(const char* family, const XE* x, const uint16_t* w16, uint16_t* y, double* stats, int B, int H, int W, int C, hipStream_t stream) {
    constexpr int NWAVE = Row<KS>::NWAVE;
    const double xb = 4.0 * B * H * W * C;
    SIMQ_REQUIRE(xb < 4294967000.0, "%s: input exceeds the 4 GiB buffer-addressing limit", family);
    StemArgs<XE> p;
    p.x = x; p.w16 = w16; p.y = y; p.stats = stats;
    p.B = B; p.H = H; p.W = W; p.C = C; p.Ho = H / 2; p.Wo = W / 2;
    p.x_bytes = (unsigned)(xb / 4.0 * sizeof(XE));
    const int ntiles = B * p.Ho * (p.Wo / 16);
    int blocks = (ntiles + NWAVE - 1) / NWAVE;
    const int max_blocks = 256 * Row<KS>::BLOCKS_PER_CU;              // persistent blocks: two per CU (narrow), one per CU (wide)
    if (blocks > max_blocks) blocks = max_blocks;
    static bool attr_set = false;                                     // (one per instantiation)
    const int smem = Row<KS>::SMEM_W + NWAVE * COUT * 2 * (int)sizeof(double);
    if (!attr_set) {
        SIMQ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(stem_conv_bf16_kernel<XE, KS>), hipFuncAttributeMaxDynamicSharedMemorySize, smem));
        attr_set = true;
    }
    note_launch(family);
    hipLaunchKernelGGL((stem_conv_bf16_kernel<XE, KS>), dim3(blocks), dim3(NWAVE * 64), smem, stream, p);
    SIMQ_CHECK_LAUNCH();
    return 0;
}

}  // namespace

// y: bf16 [B][H/2][W/2][64];  stats: NULL or [2 * 64] doubles (accumulated into)
// (w16 in the layout launch_stem_weight_prep makes for the same ks)
int launch_stem_conv_bf16(StemX x, int ks, const uint16_t* w16, uint16_t* y, double* stats, int B, int H, int W, int C, hipStream_t stream) {
    const char* family = stem_family(false, ks, x.bf16);
    return stem_dispatch(family, x, ks, H, W, C, [&](auto* xe, auto k) {
        return stem_conv_bf16_impl<decltype(k)::value>(family, xe, w16, y, stats, B, H, W, C, stream);
    });
}

}  // namespace simq
