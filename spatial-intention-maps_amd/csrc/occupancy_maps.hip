// libsimq: batched occupancy maps -- what OccupancyMap.update derives from the occupancy map
//   occupancy_maps_kernel    configuration_space, cspace_thin (two disk dilations)                envs.py:2453, 2455
//                            closest_cspace_indices (Euclidean feature transform)                 envs.py:2454, read at 2522-2523
//
// Exactness.  Everything is integer.  A cell is dilated when an occupied cell lies at an offset di^2 + dj^2 <= r^2 inside the map:
// with v[i][j] the distance from (i, j) to the nearest occupied cell of its own column, that is "some |dj| <= r has
// v[i][j + dj] <= floor(sqrt(r^2 - dj^2))".  The closest free cell follows scipy's two one-dimensional passes: f0[i][j] is the nearest
// free row of column j (the smaller row on a tie), and the answer at (i, j) is the column j' that minimises
// (j' - j)^2 + (f0[i][j'] - i)^2, the smaller j' on a tie.  The search walks j' = j, j - 1, j + 1, j - 2, ... and stops once
// (j' - j)^2 alone exceeds the best distance: nothing further out can win or tie.  A candidate left of j has a smaller column than
// every earlier one and takes a tie; one right of j does not.
//
// Shape.  One workgroup of 256 lanes per problem, two byte planes of 256 rows x 260 bytes in LDS (133 KB of the 160 KB; the stride of
// 65 words keeps a column walk of adjacent lanes on distinct banks).  Column passes run one lane per column, down and up; the per-pixel
// phases run over the flat pixel index, so that consecutive lanes read consecutive LDS bytes and write consecutive elements of a row.
// Rows, columns and row indices fit a byte because SIMQ_OCCUPANCY_MAX_DIM is 256.
#include "batch_abi.h"
#include "../../include/simq.h"

#include <vector>

namespace simq {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxDim = SIMQ_OCCUPANCY_MAX_DIM;
constexpr int kMaxRadius = SIMQ_OCCUPANCY_MAX_RADIUS;
constexpr int kStride = kMaxDim + 4;              // bytes per LDS row: 65 words
static_assert(kMaxDim == kThreads && kMaxDim <= 256, "one lane per column; a row index must fit a byte");

// plane[i][j] (nonzero = set) -> the distance from (i, j) to the nearest set cell of column j, 255 when that is further or absent
__device__ __forceinline__ void column_distance(uint8_t* plane, int rows, int cols, int tid) {
    if (tid >= cols) return;
    uint8_t* c = plane + tid;
    int d = 255;
#pragma unroll 4
    for (int i = 0; i < rows; ++i) {
        d = c[i * kStride] ? 0 : min(d + 1, 255);
        c[i * kStride] = (uint8_t)d;
    }
    d = 255;
#pragma unroll 4
    for (int i = rows - 1; i >= 0; --i) {
        d = min((int)c[i * kStride], min(d + 1, 255));
        c[i * kStride] = (uint8_t)d;
    }
}

// half[k], k = 0 .. r: floor(sqrt(r^2 - k^2)), the half height of the disk at column offset k
__device__ __forceinline__ void disk_halves(int* half, int r, int tid) {
    if (tid > r) return;
    int w = 0;
    while ((w + 1) * (w + 1) + tid * tid <= r * r) ++w;
    half[tid] = w;
}

// some set cell of `dist`'s plane lies within the disk of radius r around (i, j)
__device__ __forceinline__ bool dilated(const uint8_t* dist, const int* half, int r, int i, int j, int cols) {
    const uint8_t* row = dist + i * kStride;
    const int lo = max(j - r, 0), hi = min(j + r, cols - 1);
    bool hit = false;
    for (int jj = lo; jj <= hi; ++jj) hit |= (int)row[jj] <= half[abs(jj - j)];
    return hit;
}

__global__ void __launch_bounds__(kThreads) occupancy_maps_kernel(const uint8_t* __restrict__ maps, int64_t maps_bytes,
                                                                  const simq_occupancy_problem* __restrict__ probs,
                                                                  uint8_t* __restrict__ cspace, uint8_t* __restrict__ thin, int64_t cspace_bytes,
                                                                  int32_t* __restrict__ closest, int64_t closest_ints,
                                                                  int32_t* __restrict__ status) {
    __shared__ uint8_t plane_a[kMaxDim * kStride];       // column distances, then f0
    __shared__ uint8_t plane_b[kMaxDim * kStride];       // the configuration space
    __shared__ int half_r[kMaxRadius + 1], half_t[kMaxRadius + 1];
    __shared__ int col_lo, col_hi;                       // the columns that hold a free cell: [col_lo, col_hi], empty when col_hi < 0
    __shared__ uint8_t col_free[kMaxDim];
    const int tid = threadIdx.x;
    const simq_occupancy_problem p = probs[blockIdx.x];
    const int R = p.rows, C = p.cols;
    const int64_t cells = (int64_t)R * C;
    if (R < 1 || R > kMaxDim || C < 1 || C > kMaxDim || p.radius < 0 || p.radius > kMaxRadius || p.thin_radius < 0 ||
        p.thin_radius > kMaxRadius || p.occupancy_offset < 0 || p.occupancy_offset > maps_bytes - cells || p.mask_offset < 0 ||
        p.mask_offset > maps_bytes - cells || p.out_offset < 0 || p.out_offset > cspace_bytes - cells ||
        2 * p.out_offset > closest_ints - 2 * cells) {
        if (tid == 0) status[blockIdx.x] = 2;            // (the host validated already: nothing is read or written)
        return;
    }
    const int n = R * C;
    const uint8_t* occ = maps + p.occupancy_offset;
    const uint8_t* mask = maps + p.mask_offset;
    uint8_t* o_cs = cspace + p.out_offset;
    uint8_t* o_thin = thin + p.out_offset;
    int32_t* o_row = closest + 2 * p.out_offset;
    int32_t* o_col = o_row + n;

    disk_halves(half_r, p.radius, tid);
    disk_halves(half_t, p.thin_radius, tid);
    if (tid == 0) {
        col_lo = kMaxDim;
        col_hi = -1;
    }
    for (int k = tid; k < n; k += kThreads) {
        const int i = k / C, j = k - i * C;
        plane_a[i * kStride + j] = occ[k] != 0;
    }
    __syncthreads();
    column_distance(plane_a, R, C, tid);
    __syncthreads();
    // configuration space: inside the room and not within `radius` of an occupied cell
    for (int k = tid; k < n; k += kThreads) {
        const int i = k / C, j = k - i * C;
        const uint8_t v = (mask[k] != 0 && !dilated(plane_a, half_r, p.radius, i, j, C)) ? 1 : 0;
        plane_b[i * kStride + j] = v;
        o_cs[k] = v;
    }
    __syncthreads();
    // thin space: not within `thin_radius` of an occupied cell of the room
    for (int k = tid; k < n; k += kThreads) {
        const int i = k / C, j = k - i * C;
        plane_a[i * kStride + j] = occ[k] != 0 && mask[k] != 0;
    }
    __syncthreads();
    column_distance(plane_a, R, C, tid);
    __syncthreads();
    for (int k = tid; k < n; k += kThreads) {
        const int i = k / C, j = k - i * C;
        o_thin[k] = dilated(plane_a, half_t, p.thin_radius, i, j, C) ? 0 : 1;
    }
    __syncthreads();

    // first pass of the feature transform: plane_a[i][j] = f0, the nearest free row of column j (the smaller row on a tie)
    if (tid < C) {
        const uint8_t* fr = plane_b + tid;
        uint8_t* f0 = plane_a + tid;
        int last = -1;
#pragma unroll 4
        for (int i = 0; i < R; ++i) {
            if (fr[i * kStride]) last = i;
            f0[i * kStride] = (uint8_t)(last < 0 ? 255 : last);       // 255 at a blocked cell: read back as "none above" (never < i)
        }
        col_free[tid] = last >= 0;
        if (last >= 0) {
            atomicMin(&col_lo, tid);
            atomicMax(&col_hi, tid);
        }
        int next = -1;
#pragma unroll 4
        for (int i = R - 1; i >= 0; --i) {
            if (fr[i * kStride]) {
                next = i;                                             // (f0 holds i already)
            } else {
                const int above = f0[i * kStride];
                const bool has_above = above < i, has_below = next >= 0;
                int f = 0;
                if (has_above && (!has_below || i - above <= next - i)) f = above;
                else if (has_below) f = next;
                f0[i * kStride] = (uint8_t)f;
            }
        }
    }
    __syncthreads();

    // second pass: the nearest column site of every blocked pixel
    const int clo = col_lo, chi = col_hi;
    for (int k = tid; k < n; k += kThreads) {
        const int i = k / C, j = k - i * C;
        int bi = i, bj = j;
        if (chi < 0) {
            bi = bj = -1;
        } else if (!plane_b[i * kStride + j]) {
            const uint8_t* f0 = plane_a + i * kStride;
            int best = 0x7fffffff;
            const int kmax = max(j - clo, chi - j);
            for (int s = max(max(clo - j, j - chi), 0); s <= kmax && s * s <= best; ++s) {
                const int jl = j - s, jr = j + s;
                if (jl >= clo && col_free[jl]) {
                    const int di = (int)f0[jl] - i, d2 = s * s + di * di;
                    if (d2 <= best) { best = d2; bi = f0[jl]; bj = jl; }
                }
                if (s > 0 && jr <= chi && col_free[jr]) {
                    const int di = (int)f0[jr] - i, d2 = s * s + di * di;
                    if (d2 < best) { best = d2; bi = f0[jr]; bj = jr; }
                }
            }
        }
        o_row[k] = bi;
        o_col[k] = bj;
    }
    if (tid == 0) status[blockIdx.x] = chi < 0 ? 1 : 0;
}

}  // namespace

}  // namespace simq

using namespace simq;

extern "C" int simq_occupancy_maps(const uint8_t* d_maps, int64_t maps_bytes, const simq_occupancy_problem* problems, int n,
                                   simq_occupancy_problem* d_problems, uint8_t* d_cspace, uint8_t* d_thin, int64_t cspace_bytes,
                                   int32_t* d_closest, int64_t closest_ints, int32_t* d_status, void* stream) {
    SIMQ_REQUIRE(d_maps && problems && d_problems && d_cspace && d_thin && d_closest && d_status, "occupancy_maps: NULL pointer");
    SIMQ_REQUIRE(n >= 1 && n <= (1 << 20), "occupancy_maps: n = %d (1 .. 2^20 problems)", n);
    SIMQ_REQUIRE(maps_bytes >= 0 && cspace_bytes >= 0 && closest_ints >= 0 && maps_bytes < (1LL << 40) && cspace_bytes < (1LL << 40) &&
                     closest_ints < (1LL << 40),
                 "occupancy_maps: buffer sizes %lld, %lld, %lld (each in [0, 2^40))", (long long)maps_bytes, (long long)cspace_bytes,
                 (long long)closest_ints);
    SIMQ_REQUIRE(((uintptr_t)d_problems & 7) == 0 && ((uintptr_t)d_closest & 3) == 0 && ((uintptr_t)d_status & 3) == 0,
                 "occupancy_maps: d_problems must be 8-byte, d_closest and d_status 4-byte aligned");
    std::vector<Span> spans;
    spans.reserve(n);
    for (int i = 0; i < n; ++i) {
        const simq_occupancy_problem& p = problems[i];
        SIMQ_REQUIRE(p.rows >= 1 && p.rows <= kMaxDim && p.cols >= 1 && p.cols <= kMaxDim,
                     "occupancy_maps: problem %d is %d x %d (rows, cols in 1 .. %d)", i, p.rows, p.cols, kMaxDim);
        SIMQ_REQUIRE(p.radius >= 0 && p.radius <= kMaxRadius, "occupancy_maps: problem %d: radius = %d (0 .. %d)", i, p.radius, kMaxRadius);
        SIMQ_REQUIRE(p.thin_radius >= 0 && p.thin_radius <= kMaxRadius, "occupancy_maps: problem %d: thin_radius = %d (0 .. %d)", i,
                     p.thin_radius, kMaxRadius);
        const int64_t cells = (int64_t)p.rows * p.cols;
        SIMQ_REQUIRE(fits(p.occupancy_offset, cells, maps_bytes),
                     "occupancy_maps: problem %d: occupancy bytes [%lld, %lld) outside the %lld of d_maps", i, (long long)p.occupancy_offset,
                     (long long)(p.occupancy_offset + cells), (long long)maps_bytes);
        SIMQ_REQUIRE(fits(p.mask_offset, cells, maps_bytes),
                     "occupancy_maps: problem %d: room mask bytes [%lld, %lld) outside the %lld of d_maps", i, (long long)p.mask_offset,
                     (long long)(p.mask_offset + cells), (long long)maps_bytes);
        SIMQ_REQUIRE(fits(p.out_offset, cells, cspace_bytes),
                     "occupancy_maps: problem %d: output bytes [%lld, %lld) outside the %lld of d_cspace / d_thin", i, (long long)p.out_offset,
                     (long long)(p.out_offset + cells), (long long)cspace_bytes);
        SIMQ_REQUIRE(2 * p.out_offset <= closest_ints - 2 * cells,
                     "occupancy_maps: problem %d: closest ints [%lld, %lld) outside the %lld of d_closest", i, (long long)(2 * p.out_offset),
                     (long long)(2 * p.out_offset + 2 * cells), (long long)closest_ints);
        spans.push_back({(uint64_t)p.out_offset, (uint64_t)(p.out_offset + cells), i});
    }
    const size_t clash = first_overlap(spans);
    SIMQ_REQUIRE(clash == 0, "occupancy_maps: two problems' outputs overlap at byte %lld", (long long)spans[clash].lo);
    // every buffer the launch writes against every other buffer of the call
    const int64_t prob_bytes = (int64_t)sizeof(simq_occupancy_problem) * n, status_bytes = 4LL * n;
    const Buffer bufs[] = {
        {"d_cspace", d_cspace, cspace_bytes, true}, {"d_thin", d_thin, cspace_bytes, true}, {"d_closest", d_closest, closest_ints * 4, true},
        {"d_status", d_status, status_bytes, true}, {"d_maps", d_maps, maps_bytes, false}, {"d_problems", d_problems, prob_bytes, true}};
    int a = 0, b = 0;
    SIMQ_REQUIRE(!first_conflict(bufs, 6, &a, &b), "occupancy_maps: %s overlaps %s", bufs[a].name, bufs[b].name);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const HostBlock block = {problems, (size_t)prob_bytes};
    SIMQ_CHECK_HIP(upload_descriptors(d_problems, &block, 1, nullptr, s));
    occupancy_maps_kernel<<<n, kThreads, 0, s>>>(d_maps, maps_bytes, d_problems, d_cspace, d_thin, cspace_bytes, d_closest, closest_ints, d_status);
    SIMQ_CHECK_LAUNCH();
    note_launch("occupancy_maps");
    return 0;
}
