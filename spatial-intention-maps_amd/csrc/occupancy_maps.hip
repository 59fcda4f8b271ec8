// libsimq: batched occupancy maps -- what OccupancyMap.update derives from the occupancy map
//   occupancy_maps_kernel        configuration_space, cspace_thin (two disk dilations)            envs.py:2453, 2455
//                                closest_cspace_indices (Euclidean feature transform)             envs.py:2454, read at 2522-2523
//   occupancy_maps_large_kernel  the same for maps no LDS holds: the plane in a workspace in global memory
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
//
// The large form.  One workgroup of 1 024 lanes per problem, rows and columns up to SIMQ_OCCUPANCY_LARGE_MAX_DIM.  Plane a (column
// distances, then f0) is 16 bits a cell, dense, in the caller's workspace; plane b is the configuration space where the kernel has
// just written it in d_cspace.  Columns and pixels are looped over the block.  The column passes, the dilation test and the
// second-pass search are the device functions below, stated once over the plane's element type and stride.  col_free, the disk
// halves and col_lo / col_hi stay in LDS.  Memory order: the one workgroup runs on one compute unit, and __syncthreads() between
// two phases is a workgroup-scope release and acquire, which orders the plain vector stores of a phase before the loads of the
// next (DESIGN.md section 23's argument); no agent-scope fence, no global atomic.  What the kernel reads back -- the plane, d_cspace --
// is reached through pointers that are neither const __restrict__ nor uniform, so no such load is a scalar load.
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
constexpr int kLargeThreads = 1024;
constexpr int kLargeMaxDim = SIMQ_OCCUPANCY_LARGE_MAX_DIM;
static_assert(kLargeMaxDim < 0xFFFF, "a row index, and the mark for none, must fit 16 bits");

// the large form's plane: one uint16 per cell, rounded up to 16 bytes
__host__ __device__ inline int64_t large_work_bytes(int64_t cells) { return (2 * cells + 15) & ~(int64_t)15; }

// One column c[0], c[stride], ... of a plane (nonzero = set) -> the distance from each cell to the nearest set cell of the column,
// 255 when that is further or absent (more than any radius)
template <typename T>
__device__ __forceinline__ void column_distance(T* c, int rows, int stride) {
    int d = 255;
#pragma unroll 4
    for (int i = 0; i < rows; ++i) {
        d = c[i * stride] ? 0 : min(d + 1, 255);
        c[i * stride] = (T)d;
    }
    d = 255;
#pragma unroll 4
    for (int i = rows - 1; i >= 0; --i) {
        d = min((int)c[i * stride], min(d + 1, 255));
        c[i * stride] = (T)d;
    }
}

// half[k], k = 0 .. r: floor(sqrt(r^2 - k^2)), the half height of the disk at column offset k
__device__ __forceinline__ void disk_halves(int* half, int r, int tid) {
    if (tid > r) return;
    int w = 0;
    while ((w + 1) * (w + 1) + tid * tid <= r * r) ++w;
    half[tid] = w;
}

// some set cell lies within the disk of radius r around column j of `row`, a row of column distances
template <typename T>
__device__ __forceinline__ bool dilated(const T* row, const int* half, int r, int j, int cols) {
    const int lo = max(j - r, 0), hi = min(j + r, cols - 1);
    bool hit = false;
    for (int jj = lo; jj <= hi; ++jj) hit |= (int)row[jj] <= half[abs(jj - j)];
    return hit;
}

// First pass of the feature transform over one column, free where fr[i * fr_stride] != 0: f0[i * f0_stride] = the nearest free row
// of the column, the smaller row on a tie.  Between its two walks, down and up, has_free(last) is told the last free row of the
// column, -1 when it holds none (f0 is not read then).
template <typename T, typename HasFree>
__device__ __forceinline__ void nearest_free_rows(const uint8_t* fr, int fr_stride, T* f0, int f0_stride, int R, HasFree has_free) {
    constexpr int kNone = (T)~(T)0;                   // at a blocked cell: read back as "none above" (never < i)
    int last = -1;
#pragma unroll 4
    for (int i = 0; i < R; ++i) {
        if (fr[i * fr_stride]) last = i;
        f0[i * f0_stride] = (T)(last < 0 ? kNone : last);
    }
    has_free(last);
    int next = -1;
#pragma unroll 4
    for (int i = R - 1; i >= 0; --i) {
        if (fr[i * fr_stride]) {
            next = i;                                 // (f0 holds i already)
        } else {
            const int above = f0[i * f0_stride];
            const bool has_above = above < i, has_below = next >= 0;
            int f = 0;
            if (has_above && (!has_below || i - above <= next - i)) f = above;
            else if (has_below) f = next;
            f0[i * f0_stride] = (T)f;
        }
    }
}

// Second pass: the nearest column site (bi, bj) of the blocked pixel (i, j), f0 being row i of the first pass and [clo, chi] the
// columns that hold a free cell
template <typename T>
__device__ __forceinline__ int2 nearest_site(const T* f0, const uint8_t* col_free, int clo, int chi, int i, int j) {
    int bj = j, bi = i;                               // (in this order occupancy_maps_kernel's code comes out as it was before the large form)
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
    return make_int2(bi, bj);
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
    if (tid < C) column_distance(plane_a + tid, R, kStride);
    __syncthreads();
    // configuration space: inside the room and not within `radius` of an occupied cell
    for (int k = tid; k < n; k += kThreads) {
        const int i = k / C, j = k - i * C;
        const uint8_t v = (mask[k] != 0 && !dilated(plane_a + i * kStride, half_r, p.radius, j, C)) ? 1 : 0;
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
    if (tid < C) column_distance(plane_a + tid, R, kStride);
    __syncthreads();
    for (int k = tid; k < n; k += kThreads) {
        const int i = k / C, j = k - i * C;
        o_thin[k] = dilated(plane_a + i * kStride, half_t, p.thin_radius, j, C) ? 0 : 1;
    }
    __syncthreads();

    // first pass of the feature transform: plane_a[i][j] = f0, the nearest free row of column j (the smaller row on a tie)
    if (tid < C) {
        nearest_free_rows(plane_b + tid, kStride, plane_a + tid, kStride, R, [&](int last) {
            col_free[tid] = last >= 0;
            if (last >= 0) {
                atomicMin(&col_lo, tid);
                atomicMax(&col_hi, tid);
            }
        });
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
            const int2 site = nearest_site(plane_a + i * kStride, col_free, clo, chi, i, j);
            bi = site.x;
            bj = site.y;
        }
        o_row[k] = bi;
        o_col[k] = bj;
    }
    if (tid == 0) status[blockIdx.x] = chi < 0 ? 1 : 0;
}

// The phases of occupancy_maps_kernel with plane a in the workspace (16 bits a cell, C cells a row) and d_cspace as plane b.
// `cspace` and `work` are read back after they are written: neither is const or __restrict__.
__global__ void __launch_bounds__(kLargeThreads) occupancy_maps_large_kernel(const uint8_t* __restrict__ maps, int64_t maps_bytes,
                                                                             const simq_occupancy_large_problem* __restrict__ probs,
                                                                             uint8_t* cspace, uint8_t* __restrict__ thin, int64_t cspace_bytes,
                                                                             int32_t* __restrict__ closest, int64_t closest_ints,
                                                                             int32_t* __restrict__ status, char* work, int64_t work_bytes) {
    __shared__ int half_r[kMaxRadius + 1], half_t[kMaxRadius + 1];
    __shared__ int col_lo, col_hi;                       // the columns that hold a free cell: [col_lo, col_hi], empty when col_hi < 0
    __shared__ uint8_t col_free[kLargeMaxDim];
    const int tid = threadIdx.x;
    const simq_occupancy_large_problem p = probs[blockIdx.x];
    const int R = p.rows, C = p.cols;
    const int64_t cells = (int64_t)R * C;
    if (R < 1 || R > kLargeMaxDim || C < 1 || C > kLargeMaxDim || cells >= SIMQ_GRID_MAX_CELLS || p.radius < 0 || p.radius > kMaxRadius ||
        p.thin_radius < 0 || p.thin_radius > kMaxRadius || p.occupancy_offset < 0 || p.occupancy_offset > maps_bytes - cells ||
        p.mask_offset < 0 || p.mask_offset > maps_bytes - cells || p.out_offset < 0 || p.out_offset > cspace_bytes - cells ||
        2 * p.out_offset > closest_ints - 2 * cells || !work || p.work_offset < 0 || (p.work_offset & 15) != 0 ||
        p.work_offset > work_bytes - large_work_bytes(cells)) {
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
    uint16_t* plane_a = reinterpret_cast<uint16_t*>(work + p.work_offset);       // column distances, then f0

    disk_halves(half_r, p.radius, tid);
    disk_halves(half_t, p.thin_radius, tid);
    if (tid == 0) {
        col_lo = kLargeMaxDim;
        col_hi = -1;
    }
    for (int k = tid; k < n; k += kLargeThreads) plane_a[k] = occ[k] != 0;
    __syncthreads();
    for (int j = tid; j < C; j += kLargeThreads) column_distance(plane_a + j, R, C);
    __syncthreads();
    // configuration space: inside the room and not within `radius` of an occupied cell
    for (int k = tid; k < n; k += kLargeThreads) {
        const int i = k / C, j = k - i * C;
        o_cs[k] = (mask[k] != 0 && !dilated(plane_a + i * C, half_r, p.radius, j, C)) ? 1 : 0;
    }
    __syncthreads();
    // thin space: not within `thin_radius` of an occupied cell of the room
    for (int k = tid; k < n; k += kLargeThreads) plane_a[k] = occ[k] != 0 && mask[k] != 0;
    __syncthreads();
    for (int j = tid; j < C; j += kLargeThreads) column_distance(plane_a + j, R, C);
    __syncthreads();
    for (int k = tid; k < n; k += kLargeThreads) {
        const int i = k / C, j = k - i * C;
        o_thin[k] = dilated(plane_a + i * C, half_t, p.thin_radius, j, C) ? 0 : 1;
    }
    __syncthreads();

    // first pass of the feature transform: plane_a[i][j] = f0, the nearest free row of column j (the smaller row on a tie)
    for (int j = tid; j < C; j += kLargeThreads) {
        nearest_free_rows(o_cs + j, C, plane_a + j, C, R, [&](int last) {
            col_free[j] = last >= 0;
            if (last >= 0) {
                atomicMin(&col_lo, j);
                atomicMax(&col_hi, j);
            }
        });
    }
    __syncthreads();

    // second pass: the nearest column site of every blocked pixel
    const int clo = col_lo, chi = col_hi;
    for (int k = tid; k < n; k += kLargeThreads) {
        const int i = k / C, j = k - i * C;
        int bi = i, bj = j;
        if (chi < 0) {
            bi = bj = -1;
        } else if (!o_cs[k]) {
            const int2 site = nearest_site(plane_a + i * C, col_free, clo, chi, i, j);
            bi = site.x;
            bj = site.y;
        }
        o_row[k] = bi;
        o_col[k] = bj;
    }
    if (tid == 0) status[blockIdx.x] = chi < 0 ? 1 : 0;
}

// Every rule both entry points share (`who` names the entry point in the refusal), in the order the refusals come: the call's
// pointers and extents, then problem by problem the shape against max_dim, the radii and the ranges; each(i, p) holds the entry
// point's own rule for problem i and returns 0 or -1 with the error set.  The problems' output spans are left in `spans`, checked.
template <typename Problem, typename Each>
int check_problems(const char* who, const Problem* problems, int n, int max_dim, const void* d_problems, const void* d_closest,
                   const void* d_status, int64_t maps_bytes, int64_t cspace_bytes, int64_t closest_ints, Each each) {
    SIMQ_REQUIRE(n >= 1 && n <= (1 << 20), "%s: n = %d (1 .. 2^20 problems)", who, n);
    SIMQ_REQUIRE(maps_bytes >= 0 && cspace_bytes >= 0 && closest_ints >= 0 && maps_bytes < (1LL << 40) && cspace_bytes < (1LL << 40) &&
                     closest_ints < (1LL << 40),
                 "%s: buffer sizes %lld, %lld, %lld (each in [0, 2^40))", who, (long long)maps_bytes, (long long)cspace_bytes,
                 (long long)closest_ints);
    SIMQ_REQUIRE(((uintptr_t)d_problems & 7) == 0 && ((uintptr_t)d_closest & 3) == 0 && ((uintptr_t)d_status & 3) == 0,
                 "%s: d_problems must be 8-byte, d_closest and d_status 4-byte aligned", who);
    std::vector<Span> spans;
    spans.reserve(n);
    for (int i = 0; i < n; ++i) {
        const Problem& p = problems[i];
        SIMQ_REQUIRE(p.rows >= 1 && p.rows <= max_dim && p.cols >= 1 && p.cols <= max_dim,
                     "%s: problem %d is %d x %d (rows, cols in 1 .. %d)", who, i, p.rows, p.cols, max_dim);
        SIMQ_REQUIRE(p.radius >= 0 && p.radius <= kMaxRadius, "%s: problem %d: radius = %d (0 .. %d)", who, i, p.radius, kMaxRadius);
        SIMQ_REQUIRE(p.thin_radius >= 0 && p.thin_radius <= kMaxRadius, "%s: problem %d: thin_radius = %d (0 .. %d)", who, i, p.thin_radius,
                     kMaxRadius);
        const int64_t cells = (int64_t)p.rows * p.cols;
        SIMQ_REQUIRE(fits(p.occupancy_offset, cells, maps_bytes), "%s: problem %d: occupancy bytes [%lld, %lld) outside the %lld of d_maps", who,
                     i, (long long)p.occupancy_offset, (long long)(p.occupancy_offset + cells), (long long)maps_bytes);
        SIMQ_REQUIRE(fits(p.mask_offset, cells, maps_bytes), "%s: problem %d: room mask bytes [%lld, %lld) outside the %lld of d_maps", who, i,
                     (long long)p.mask_offset, (long long)(p.mask_offset + cells), (long long)maps_bytes);
        SIMQ_REQUIRE(fits(p.out_offset, cells, cspace_bytes), "%s: problem %d: output bytes [%lld, %lld) outside the %lld of d_cspace / d_thin",
                     who, i, (long long)p.out_offset, (long long)(p.out_offset + cells), (long long)cspace_bytes);
        SIMQ_REQUIRE(2 * p.out_offset <= closest_ints - 2 * cells, "%s: problem %d: closest ints [%lld, %lld) outside the %lld of d_closest", who,
                     i, (long long)(2 * p.out_offset), (long long)(2 * p.out_offset + 2 * cells), (long long)closest_ints);
        if (each(i, p) != 0) return -1;
        spans.push_back({(uint64_t)p.out_offset, (uint64_t)(p.out_offset + cells), i});
    }
    const size_t clash = first_overlap(spans);
    SIMQ_REQUIRE(clash == 0, "%s: two problems' outputs overlap at byte %lld", who, (long long)spans[clash].lo);
    return 0;
}

// every buffer the launch writes against every other buffer of the call
int check_buffers(const char* who, const Buffer* bufs, int nb) {
    int a = 0, b = 0;
    SIMQ_REQUIRE(!first_conflict(bufs, nb, &a, &b), "%s: %s overlaps %s", who, bufs[a].name, bufs[b].name);
    return 0;
}

}  // namespace

}  // namespace simq

using namespace simq;

extern "C" int simq_occupancy_maps(const uint8_t* d_maps, int64_t maps_bytes, const simq_occupancy_problem* problems, int n,
                                   simq_occupancy_problem* d_problems, uint8_t* d_cspace, uint8_t* d_thin, int64_t cspace_bytes,
                                   int32_t* d_closest, int64_t closest_ints, int32_t* d_status, void* stream) {
    static const char who[] = "occupancy_maps";
    SIMQ_REQUIRE(d_maps && problems && d_problems && d_cspace && d_thin && d_closest && d_status, "%s: NULL pointer", who);
    if (check_problems(who, problems, n, kMaxDim, d_problems, d_closest, d_status, maps_bytes, cspace_bytes, closest_ints,
                       [](int, const simq_occupancy_problem&) { return 0; }) != 0)
        return -1;
    const int64_t prob_bytes = (int64_t)sizeof(simq_occupancy_problem) * n, status_bytes = 4LL * n;
    const Buffer bufs[] = {
        {"d_cspace", d_cspace, cspace_bytes, true}, {"d_thin", d_thin, cspace_bytes, true}, {"d_closest", d_closest, closest_ints * 4, true},
        {"d_status", d_status, status_bytes, true}, {"d_maps", d_maps, maps_bytes, false}, {"d_problems", d_problems, prob_bytes, true}};
    if (check_buffers(who, bufs, 6) != 0) return -1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const HostBlock block = {problems, (size_t)prob_bytes};
    SIMQ_CHECK_HIP(upload_descriptors(d_problems, &block, 1, nullptr, s));
    occupancy_maps_kernel<<<n, kThreads, 0, s>>>(d_maps, maps_bytes, d_problems, d_cspace, d_thin, cspace_bytes, d_closest, closest_ints, d_status);
    SIMQ_CHECK_LAUNCH();
    note_launch("occupancy_maps");
    return 0;
}

extern "C" int64_t simq_occupancy_maps_large_work_bytes(int32_t rows, int32_t cols) {
    if (rows < 1 || rows > kLargeMaxDim || cols < 1 || cols > kLargeMaxDim || (int64_t)rows * cols >= SIMQ_GRID_MAX_CELLS) return -1;
    return large_work_bytes((int64_t)rows * cols);
}

extern "C" int simq_occupancy_maps_large(const uint8_t* d_maps, int64_t maps_bytes, const simq_occupancy_large_problem* problems, int n,
                                         simq_occupancy_large_problem* d_problems, uint8_t* d_cspace, uint8_t* d_thin, int64_t cspace_bytes,
                                         int32_t* d_closest, int64_t closest_ints, int32_t* d_status, void* d_work, int64_t work_bytes,
                                         void* stream) {
    static const char who[] = "occupancy_maps_large";
    SIMQ_REQUIRE(d_maps && problems && d_problems && d_cspace && d_thin && d_closest && d_status && d_work, "%s: NULL pointer", who);
    SIMQ_REQUIRE(work_bytes >= 0 && work_bytes < (1LL << 40) && ((uintptr_t)d_work & 15) == 0,
                 "%s: d_work must be 16-byte aligned and work_bytes = %lld in [0, 2^40)", who, (long long)work_bytes);
    std::vector<Span> work_spans;
    const auto inside_the_workspace = [&](int i, const simq_occupancy_large_problem& p) {
        const int64_t cells = (int64_t)p.rows * p.cols;
        SIMQ_REQUIRE(cells < SIMQ_GRID_MAX_CELLS, "%s: problem %d is %d x %d (rows * cols < 2^22: what the stages behind it take)", who, i,
                     p.rows, p.cols);
        const int64_t need = large_work_bytes(cells);
        SIMQ_REQUIRE(p.work_offset % 16 == 0 && fits(p.work_offset, need, work_bytes),
                     "%s: problem %d: work_offset: bytes [%lld, %lld) outside the %lld of d_work, or not at a multiple of 16", who, i,
                     (long long)p.work_offset, (long long)(p.work_offset + need), (long long)work_bytes);
        work_spans.push_back({(uint64_t)p.work_offset, (uint64_t)(p.work_offset + need), i});
        return 0;
    };
    if (check_problems(who, problems, n, kLargeMaxDim, d_problems, d_closest, d_status, maps_bytes, cspace_bytes, closest_ints,
                       inside_the_workspace) != 0)
        return -1;
    const size_t clash = first_overlap(work_spans);
    SIMQ_REQUIRE(clash == 0, "%s: problems %d and %d overlap in d_work at byte %lld", who, work_spans[clash - 1].problem,
                 work_spans[clash].problem, (long long)work_spans[clash].lo);
    const int64_t prob_bytes = (int64_t)sizeof(simq_occupancy_large_problem) * n, status_bytes = 4LL * n;
    const Buffer bufs[] = {{"d_cspace", d_cspace, cspace_bytes, true},     {"d_thin", d_thin, cspace_bytes, true},
                           {"d_closest", d_closest, closest_ints * 4, true}, {"d_status", d_status, status_bytes, true},
                           {"d_maps", d_maps, maps_bytes, false},          {"d_problems", d_problems, prob_bytes, true},
                           {"d_work", d_work, work_bytes, true}};
    if (check_buffers(who, bufs, 7) != 0) return -1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const HostBlock block = {problems, (size_t)prob_bytes};
    SIMQ_CHECK_HIP(upload_descriptors(d_problems, &block, 1, nullptr, s));
    occupancy_maps_large_kernel<<<n, kLargeThreads, 0, s>>>(d_maps, maps_bytes, d_problems, d_cspace, d_thin, cspace_bytes, d_closest,
                                                            closest_ints, d_status, static_cast<char*>(d_work), work_bytes);
    SIMQ_CHECK_LAUNCH();
    note_launch("occupancy_maps_large");
    return 0;
}

