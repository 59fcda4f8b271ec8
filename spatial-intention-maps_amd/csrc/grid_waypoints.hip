// libsimq: batched shortest-path waypoints on 8-connected grids -- SPFA's parents and the dense path, bit for bit
//   grid_paths_kernel<InLds>  GridGraph._spfa + the walk of GridGraph.shortest_path               shortest_paths.pyx:69-114, 126-137
//                             (+ the front half of OccupancyMap.shortest_path: straight-line test, closest free cells   envs.py:2477-2490)
//   grid_paths_kernel<InHbm>  the same with the search state in a workspace in global memory: windows over the LDS cap
//
// The search, the stages in front of it and why the search itself has to be emulated are grid_spfa.h's, shared with
// action_waypoints.hip.  What is this file's own: the walk from the target into the caller's path buffer under its capacity, and
// the optional parent and distance images over the full grid.  Both kernels are one template over where the state lies (InLds, InHbm),
// and both entry points one validation (check_problems, check_buffers): what differs is the state's home and what bounds it.
#include "batch_abi.h"
#include "grid_spfa.h"
#include "../../include/simq.h"

#include <algorithm>
#include <vector>

namespace simq {

namespace {

using namespace grid_spfa;

// kCapped: the window must fit LDS (simq_grid_path_problem); otherwise any window inside the grid (simq_grid_path_large_problem)
template <bool kCapped, typename Problem>
__device__ __forceinline__ bool descriptor_ok(const Problem& p, const int32_t* closest, const int32_t* parents, const float* dist) {
    if (p.rows < 1 || p.cols < 1 || (int64_t)p.rows * p.cols >= SIMQ_GRID_MAX_CELLS) return false;
    if (p.src_i < 0 || p.src_i >= p.rows || p.src_j < 0 || p.src_j >= p.cols) return false;
    if (p.tgt_i < 0 || p.tgt_i >= p.rows || p.tgt_j < 0 || p.tgt_j >= p.cols) return false;
    if (p.grid_offset < 0 || p.path_offset < 0 || p.path_capacity < 1) return false;
    if (p.box_rows < 0 || p.box_cols < 0 || p.box_i0 < 0 || p.box_j0 < 0 || p.box_i0 > p.rows - p.box_rows ||
        p.box_j0 > p.cols - p.box_cols)
        return false;
    if (kCapped && (int64_t)(p.box_rows + 2) * (p.box_cols + 2) > SIMQ_GRID_PATH_MAX_BOX_CELLS) return false;
    if ((p.closest_offset >= 0 && !closest) || (p.parents_offset >= 0 && !parents) || (p.dist_offset >= 0 && !dist)) return false;
    return true;
}

// Where the state lies: the descriptor, the kernel's last argument, the rule that argument adds to the descriptor's, the state's memory.
struct InLds {
    using Problem = simq_grid_path_problem;
    using State = Lds;
    using Arg = unsigned;                               // the dynamic LDS of the launch, bytes
    static constexpr bool kCapped = true;
    static __device__ __forceinline__ bool room(const Problem& p, Arg have) { return lds_bytes(p.box_rows, p.box_cols) <= (int64_t)have; }
    static __device__ __forceinline__ char* memory(const Problem&, Arg) {
        extern __shared__ __attribute__((aligned(16))) char smem[];
        return smem;
    }
};
// No LDS: how many of these wavefronts a compute unit holds is a matter of registers alone, and the others' pops hide the latency
// of one's loads.
struct InHbm {
    using Problem = simq_grid_path_large_problem;
    using State = Hbm;
    struct Arg {                                        // the caller's workspace
        char* work;
        int64_t bytes;
    };
    static constexpr bool kCapped = false;
    static __device__ __forceinline__ bool room(const Problem& p, Arg w) {
        return w.work && p.work_offset >= 0 && (p.work_offset & 15) == 0 && p.work_offset <= w.bytes - work_bytes(p.box_rows, p.box_cols);
    }
    static __device__ __forceinline__ char* memory(const Problem& p, Arg w) { return w.work + p.work_offset; }
};

// One problem by one wavefront: the descriptor again, the front stages, the search with its state where Where says, the walk and
// the images.
template <typename Where>
__global__ void __launch_bounds__(kLanes) grid_paths_kernel(const uint8_t* __restrict__ grids, const int32_t* __restrict__ closest,
                                                            const typename Where::Problem* __restrict__ probs, int32_t* __restrict__ paths,
                                                            int32_t* __restrict__ lengths, int32_t* __restrict__ endpoints,
                                                            int32_t* __restrict__ parents_out, float* __restrict__ dist_out,
                                                            int32_t* __restrict__ status, typename Where::Arg where) {
    const typename Where::Problem p = probs[blockIdx.x];
    const int lane = threadIdx.x;
    if (!descriptor_ok<Where::kCapped>(p, closest, parents_out, dist_out) || !Where::room(p, where)) {
        if (lane == 0) status[blockIdx.x] = 2;          // (the host validated already: nothing is read or written)
        return;
    }
    const int R = p.rows, C = p.cols, n = R * C;
    const uint8_t* g = grids + p.grid_offset;
    int si = p.src_i, sj = p.src_j, ti = p.tgt_i, tj = p.tgt_j;

    // ---- OccupancyMap.shortest_path's straight-line test, on the pixels as given (envs.py:2483-2485)
    if (p.thin_offset >= 0) {
        const uint8_t* thin = grids + p.thin_offset;
        if (!line_hits([&](int r, int c) { return thin[r * C + c] != 1; }, si, sj, ti, tj, lane)) {
            if (lane == 0) {
                status[blockIdx.x] = 1;
                lengths[blockIdx.x] = 0;
                int32_t* e = endpoints + 4 * (int64_t)blockIdx.x;
                e[0] = si; e[1] = sj; e[2] = ti; e[3] = tj;
            }
            return;
        }
    }
    // ---- OccupancyMap._closest_valid_cspace_indices (envs.py:2488-2489, 2522-2523)
    if (p.closest_offset >= 0) {
        const int32_t* cl = closest + p.closest_offset;
        if (!snap(cl, R, C, si, sj) || !snap(cl, R, C, ti, tj)) {
            if (lane == 0) status[blockIdx.x] = 2;
            return;
        }
    }

    // ---- every free cell must lie inside the declared window
    const Window box = {p.box_i0, p.box_j0, p.box_rows, p.box_cols};
    if (!free_cells_inside(g, n, C, box, lane)) {
        if (lane == 0) status[blockIdx.x] = 2;
        return;
    }

    // ---- the search over the window + halo
    const typename Where::State lds(Where::memory(p, where), box);
    const float inf = 2.f * (float)n;                    // self.inf = 2 * max_num_verts (exact: < 2^24)
    const bool tgt_in = box.holds(ti, tj);
    const int s_l = box.holds(si, sj) ? lds.index(box, si, sj) : -1;
    const int vertices = init_window<false>(lds, g, C, box, s_l, inf, lane);
    const bool searched = s_l >= 0 && lds.flg[s_l] != 0; // edges leave a free cell only: a blocked source relaxes nothing
    int st = searched ? search<false>(lds, s_l, vertices + 1, lane) : 0;

    // ---- the walk from the target (shortest_paths.pyx:126-137)
    if (lane == 0) {
        int32_t* path = paths + 2 * p.path_offset;
        int len = 1;
        path[0] = ti;
        path[1] = tj;
        if (searched && tgt_in) {
            int i = ti, j = tj;
            int v = lds.index(box, ti, tj);
            while (v != s_l && len <= lds.N) {
                const int pk = lds.par[v];
                if (pk == kNoParent) break;
                i -= dir_di(pk);
                j -= dir_dj(pk);
                v -= dir_di(pk) * lds.W + dir_dj(pk);
                if (len < p.path_capacity) { path[2 * len] = i; path[2 * len + 1] = j; }
                ++len;
            }
        }
        lengths[blockIdx.x] = len;
        int32_t* e = endpoints + 4 * (int64_t)blockIdx.x;
        e[0] = si; e[1] = sj; e[2] = ti; e[3] = tj;
        if (st == 0 && len > p.path_capacity) st = 3;
        status[blockIdx.x] = st;
    }

    // ---- the optional images over the full grid, from the state
    if (p.parents_offset >= 0 || p.dist_offset >= 0) {
        int32_t* po = p.parents_offset >= 0 ? parents_out + p.parents_offset : nullptr;
        float* dout = p.dist_offset >= 0 ? dist_out + p.dist_offset : nullptr;
        for (int r = 0; r < R; ++r) {
            for (int c = lane; c < C; c += kLanes) {
                int32_t pv = -1;
                float x = r == si && c == sj ? 0.f : -1.f;
                if (box.holds(r, c)) {
                    const int l = lds.index(box, r, c);
                    const int pk = lds.par[l];
                    if (pk != kNoParent) pv = (r - dir_di(pk)) * C + (c - dir_dj(pk));
                    const float d = lds.dist[l];
                    x = d == inf ? -1.f : d;
                }
                if (po) po[r * C + c] = pv;
                if (dout) dout[r * C + c] = x;
            }
        }
    }
}

int disjoint(const char* who, std::vector<Span>& spans, const char* what) {
    const size_t i = first_overlap(spans);
    SIMQ_REQUIRE(i == 0, "%s: problems %d and %d overlap in %s at element %lld", who, spans[i - 1].problem, spans[i].problem, what,
                 (long long)spans[i].lo);
    return 0;
}

// Every rule of a descriptor array that both entry points share (`who` names the entry point in the refusal), in the order the
// refusals come; `each(i, p)` holds the entry point's own rule for problem i and returns 0 or -1 with the error set.
template <typename Problem, typename Each>
int check_problems(const char* who, const Problem* problems, int n, int64_t grids_bytes, const int32_t* d_closest, int64_t closest_ints,
                   int64_t path_pairs, const int32_t* d_parents, int64_t parents_ints, const float* d_dist, int64_t dist_floats, Each each) {
    SIMQ_REQUIRE(n >= 1 && n <= (1 << 24), "%s: n = %d (1 .. 2^24 problems)", who, n);
    std::vector<Span> path_spans, parent_spans, dist_spans;
    path_spans.reserve(n);
    for (int i = 0; i < n; ++i) {
        const Problem& p = problems[i];
        SIMQ_REQUIRE(p.rows >= 1 && p.cols >= 1 && (int64_t)p.rows * p.cols < SIMQ_GRID_MAX_CELLS,
                     "%s: problem %d is %d x %d (rows, cols >= 1, rows * cols < 2^22)", who, i, p.rows, p.cols);
        SIMQ_REQUIRE(p.src_i >= 0 && p.src_i < p.rows && p.src_j >= 0 && p.src_j < p.cols,
                     "%s: problem %d: source (%d, %d) outside its %d x %d grid", who, i, p.src_i, p.src_j, p.rows, p.cols);
        SIMQ_REQUIRE(p.tgt_i >= 0 && p.tgt_i < p.rows && p.tgt_j >= 0 && p.tgt_j < p.cols,
                     "%s: problem %d: target (%d, %d) outside its %d x %d grid", who, i, p.tgt_i, p.tgt_j, p.rows, p.cols);
        const int64_t cells = (int64_t)p.rows * p.cols;
        SIMQ_REQUIRE(fits(p.grid_offset, cells, grids_bytes),
                     "%s: problem %d: grid_offset: bytes [%lld, %lld) outside the %lld of d_grids", who, i, (long long)p.grid_offset,
                     (long long)(p.grid_offset + cells), (long long)grids_bytes);
        SIMQ_REQUIRE(p.thin_offset == -1 || fits(p.thin_offset, cells, grids_bytes),
                     "%s: problem %d: thin_offset: bytes [%lld, %lld) outside the %lld of d_grids (-1: no straight-line test)", who, i,
                     (long long)p.thin_offset, (long long)(p.thin_offset + cells), (long long)grids_bytes);
        SIMQ_REQUIRE(p.closest_offset == -1 || (d_closest && fits(p.closest_offset, 2 * cells, closest_ints)),
                     "%s: problem %d: closest_offset: ints [%lld, %lld) outside the %lld of d_closest (-1: no snap)", who, i,
                     (long long)p.closest_offset, (long long)(p.closest_offset + 2 * cells), (long long)(d_closest ? closest_ints : 0));
        SIMQ_REQUIRE(p.box_rows >= 0 && p.box_cols >= 0 && p.box_i0 >= 0 && p.box_j0 >= 0 && p.box_i0 <= p.rows - p.box_rows &&
                         p.box_j0 <= p.cols - p.box_cols,
                     "%s: problem %d: box rows [%d, %d + %d), columns [%d, %d + %d) outside its %d x %d grid", who, i, p.box_i0, p.box_i0,
                     p.box_rows, p.box_j0, p.box_j0, p.box_cols, p.rows, p.cols);
        if (each(i, p) != 0) return -1;
        SIMQ_REQUIRE(p.path_capacity >= 1, "%s: problem %d: path_capacity = %d (>= 1 pair)", who, i, p.path_capacity);
        SIMQ_REQUIRE(fits(p.path_offset, p.path_capacity, path_pairs),
                     "%s: problem %d: path_offset: pairs [%lld, %lld) outside the %lld of d_paths", who, i, (long long)p.path_offset,
                     (long long)(p.path_offset + p.path_capacity), (long long)path_pairs);
        path_spans.push_back({(uint64_t)p.path_offset, (uint64_t)(p.path_offset + p.path_capacity), i});
        SIMQ_REQUIRE(p.parents_offset == -1 || (d_parents && fits(p.parents_offset, cells, parents_ints)),
                     "%s: problem %d: parents_offset: ints [%lld, %lld) outside the %lld of d_parents (-1: no parent image)", who, i,
                     (long long)p.parents_offset, (long long)(p.parents_offset + cells), (long long)(d_parents ? parents_ints : 0));
        if (p.parents_offset >= 0) parent_spans.push_back({(uint64_t)p.parents_offset, (uint64_t)(p.parents_offset + cells), i});
        SIMQ_REQUIRE(p.dist_offset == -1 || (d_dist && fits(p.dist_offset, cells, dist_floats)),
                     "%s: problem %d: dist_offset: floats [%lld, %lld) outside the %lld of d_dist (-1: no distance image)", who, i,
                     (long long)p.dist_offset, (long long)(p.dist_offset + cells), (long long)(d_dist ? dist_floats : 0));
        if (p.dist_offset >= 0) dist_spans.push_back({(uint64_t)p.dist_offset, (uint64_t)(p.dist_offset + cells), i});
    }
    if (disjoint(who, path_spans, "d_paths") || disjoint(who, parent_spans, "d_parents") || disjoint(who, dist_spans, "d_dist")) return -1;
    return 0;
}

// alignment, and the buffers against each other: an output may share no byte with another buffer of the call.  This walk is
// not batch_abi.h's first_conflict: it names the written buffer first, meets a buffer's alignment before its pairs and skips an
// empty buffer, and which refusal comes first when several rules are broken is part of an entry point's behaviour.
int check_buffers(const char* who, const Buffer* bufs, const int* align, int nb) {
    for (int a = 0; a < nb; ++a) {
        SIMQ_REQUIRE((uintptr_t)bufs[a].p % align[a] == 0, "%s: %s is not %d-byte aligned", who, bufs[a].name, align[a]);
        for (int b = 0; b < nb; ++b) {
            if (a == b || !bufs[a].written || bufs[a].bytes <= 0 || bufs[b].bytes <= 0 || (bufs[b].written && b < a)) continue;
            SIMQ_REQUIRE(!overlaps(bufs[a].p, bufs[a].bytes, bufs[b].p, bufs[b].bytes), "%s: %s and %s overlap", who, bufs[a].name,
                         bufs[b].name);
        }
    }
    return 0;
}

}  // namespace

}  // namespace simq

using namespace simq;

extern "C" int simq_grid_paths(const uint8_t* d_grids, int64_t grids_bytes, const int32_t* d_closest, int64_t closest_ints,
                               const simq_grid_path_problem* problems, int n, simq_grid_path_problem* d_problems, int32_t* d_paths,
                               int64_t path_pairs, int32_t* d_lengths, int32_t* d_endpoints, int32_t* d_parents, int64_t parents_ints,
                               float* d_dist, int64_t dist_floats, int32_t* d_status, void* stream) {
    static const char who[] = "grid_paths";
    SIMQ_REQUIRE(d_grids && problems && d_problems && d_paths && d_lengths && d_endpoints && d_status, "%s: NULL pointer", who);
    int64_t lds = 0;
    const auto under_the_cap = [&](int i, const simq_grid_path_problem& p) {
        SIMQ_REQUIRE((int64_t)(p.box_rows + 2) * (p.box_cols + 2) <= SIMQ_GRID_PATH_MAX_BOX_CELLS,
                     "%s: problem %d: box of %d x %d cells plus its halo is %lld cells, over SIMQ_GRID_PATH_MAX_BOX_CELLS = %d "
                     "(the search state lives in LDS; simq_grid_paths_large takes it)", who, i, p.box_rows, p.box_cols,
                     (long long)(p.box_rows + 2) * (p.box_cols + 2), SIMQ_GRID_PATH_MAX_BOX_CELLS);
        lds = std::max(lds, lds_bytes(p.box_rows, p.box_cols));
        return 0;
    };
    if (check_problems(who, problems, n, grids_bytes, d_closest, closest_ints, path_pairs, d_parents, parents_ints, d_dist, dist_floats,
                       under_the_cap) != 0)
        return -1;
    const Buffer bufs[] = {
        {"d_grids", d_grids, grids_bytes, false},
        {"d_closest", d_closest, d_closest ? 4 * closest_ints : 0, false},
        {"d_problems", d_problems, (int64_t)sizeof(simq_grid_path_problem) * n, true},
        {"d_paths", d_paths, 8 * path_pairs, true},
        {"d_lengths", d_lengths, 4 * (int64_t)n, true},
        {"d_endpoints", d_endpoints, 16 * (int64_t)n, true},
        {"d_parents", d_parents, d_parents ? 4 * parents_ints : 0, true},
        {"d_dist", d_dist, d_dist ? 4 * dist_floats : 0, true},
        {"d_status", d_status, 4 * (int64_t)n, true},
    };
    const int align[] = {1, 4, 8, 4, 4, 4, 4, 4, 4};
    if (check_buffers(who, bufs, align, (int)(sizeof(bufs) / sizeof(bufs[0]))) != 0) return -1;
    lds = (lds + 15) & ~(int64_t)15;
    SIMQ_REQUIRE(lds <= kLdsBudget, "%s: %lld bytes of LDS over the %d of a compute unit", who, (long long)lds, kLdsBudget);

    hipStream_t s = static_cast<hipStream_t>(stream);
    SIMQ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(grid_paths_kernel<InLds>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kLdsBudget));
    const HostBlock block = {problems, sizeof(simq_grid_path_problem) * (size_t)n};
    SIMQ_CHECK_HIP(upload_descriptors(d_problems, &block, 1, nullptr, s));
    grid_paths_kernel<InLds><<<n, kLanes, (size_t)lds, s>>>(d_grids, d_closest, d_problems, d_paths, d_lengths, d_endpoints, d_parents, d_dist,
                                                     d_status, (unsigned)lds);
    SIMQ_CHECK_LAUNCH();
    note_launch("grid_waypoints");
    return 0;
}

extern "C" int64_t simq_grid_paths_large_work_bytes(int32_t box_rows, int32_t box_cols) {
    if (box_rows < 0 || box_cols < 0 || (int64_t)box_rows * box_cols >= SIMQ_GRID_MAX_CELLS) return -1;
    return work_bytes(box_rows, box_cols);
}

extern "C" int simq_grid_paths_large(const uint8_t* d_grids, int64_t grids_bytes, const int32_t* d_closest, int64_t closest_ints,
                                     const simq_grid_path_large_problem* problems, int n, simq_grid_path_large_problem* d_problems,
                                     int32_t* d_paths, int64_t path_pairs, int32_t* d_lengths, int32_t* d_endpoints, int32_t* d_parents,
                                     int64_t parents_ints, float* d_dist, int64_t dist_floats, int32_t* d_status, void* d_work,
                                     int64_t work_bytes_have, void* stream) {
    static const char who[] = "grid_paths_large";
    SIMQ_REQUIRE(d_grids && problems && d_problems && d_paths && d_lengths && d_endpoints && d_status && d_work, "%s: NULL pointer", who);
    std::vector<Span> work_spans;
    const auto inside_the_workspace = [&](int i, const simq_grid_path_large_problem& p) {
        const int64_t need = work_bytes(p.box_rows, p.box_cols);
        SIMQ_REQUIRE(p.work_offset % 16 == 0 && fits(p.work_offset, need, work_bytes_have),
                     "%s: problem %d: work_offset: bytes [%lld, %lld) outside the %lld of d_work, or not at a multiple of 16", who, i,
                     (long long)p.work_offset, (long long)(p.work_offset + need), (long long)work_bytes_have);
        work_spans.push_back({(uint64_t)p.work_offset, (uint64_t)(p.work_offset + need), i});
        return 0;
    };
    if (check_problems(who, problems, n, grids_bytes, d_closest, closest_ints, path_pairs, d_parents, parents_ints, d_dist, dist_floats,
                       inside_the_workspace) != 0 ||
        disjoint(who, work_spans, "d_work") != 0)
        return -1;
    const Buffer bufs[] = {
        {"d_grids", d_grids, grids_bytes, false},
        {"d_closest", d_closest, d_closest ? 4 * closest_ints : 0, false},
        {"d_problems", d_problems, (int64_t)sizeof(simq_grid_path_large_problem) * n, true},
        {"d_paths", d_paths, 8 * path_pairs, true},
        {"d_lengths", d_lengths, 4 * (int64_t)n, true},
        {"d_endpoints", d_endpoints, 16 * (int64_t)n, true},
        {"d_parents", d_parents, d_parents ? 4 * parents_ints : 0, true},
        {"d_dist", d_dist, d_dist ? 4 * dist_floats : 0, true},
        {"d_status", d_status, 4 * (int64_t)n, true},
        {"d_work", d_work, work_bytes_have, true},
    };
    const int align[] = {1, 4, 8, 4, 4, 4, 4, 4, 4, 16};
    if (check_buffers(who, bufs, align, (int)(sizeof(bufs) / sizeof(bufs[0]))) != 0) return -1;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const HostBlock block = {problems, sizeof(simq_grid_path_large_problem) * (size_t)n};
    SIMQ_CHECK_HIP(upload_descriptors(d_problems, &block, 1, nullptr, s));
    grid_paths_kernel<InHbm><<<n, kLanes, 0, s>>>(d_grids, d_closest, d_problems, d_paths, d_lengths, d_endpoints, d_parents, d_dist,
                                                  d_status, InHbm::Arg{static_cast<char*>(d_work), work_bytes_have});
    SIMQ_CHECK_LAUNCH();
    note_launch("grid_paths_large");
    return 0;
}
