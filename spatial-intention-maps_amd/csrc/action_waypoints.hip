// libsimq: from a robot's pixel pair to its waypoint pixels in one launch -- OccupancyMap.shortest_path between the two conversions
//   action_waypoints_kernel<InLds>  straight-line test, snap, GridGraph._spfa, the walk, approximate_polygon decided in integers, the
//                                   pruning                                                       envs.py:2483-2490, shortest_paths.pyx:69-154
//   action_waypoints_kernel<InHbm>  the same with the state, the path and the kept flags in a workspace in global memory: windows
//                                   over the LDS cap
//
// Both kernels are one template over where the state lies (InLds, InHbm), and both entry points one validation (check_problems,
// check_buffers), as in grid_waypoints.hip.  Below, "LDS" is the state's home: for InHbm read "the workspace".  Between the lanes of
// the one wavefront every __syncthreads() of the search and of the rule orders the stores before it ahead of the loads behind it in
// either memory, and nothing the kernel wrote is read through a const __restrict__ pointer.
// The search and the stages in front of it are grid_spfa.h's, shared with grid_paths_kernel (grid_waypoints.hip); the simplification,
// the pruning and the reversed output are waypoint_rule.h's, shared with grid_waypoints_kernel (grid_simplify.hip).  The rules are
// those of include/simq.h and the two headers say what is parallel.  What is this kernel's own:
//   * the three maps of a problem come from three bases (configuration space, thin map, closest cells), read where a BatchedMapper
//     keeps them; the window is the caller's, and the pass over the grid that refuses a free cell outside it stays;
//   * the dense path never leaves LDS.  When the queue has drained, the fp32 distances and the ring are dead: the walk writes the path
//     as 16-bit (row, column) pairs of the window (halo included, so a point is also the index of its flag byte) where the distances
//     lay -- a path has at most as many points as the window has free cells, 4 bytes each -- and the kept flags are a bit mask where
//     the ring lay (one bit a point against two bytes a free cell).  The rule compares differences of coordinates only, so
//     window coordinates decide as grid coordinates do; they are below 2^15 by the cap on the window;
//   * the pruning's lines join two points of one path, which lie in the window, so they read the flag bytes: bit 2 is set where the
//     cell of the configuration space is 1 (bit 0, free, is != 0: the search and the line test differ on a cell of 2 .. 255);
//   * an upstream word that is not 0 ends the problem before anything of it is read.
#include "batch_abi.h"
#include "grid_spfa.h"
#include "waypoint_rule.h"
#include "../../include/simq.h"

#include <algorithm>
#include <vector>

namespace simq {

namespace {

using namespace grid_spfa;

static_assert(SIMQ_GRID_WAYPOINTS_MAX_PATH >= SIMQ_GRID_PATH_MAX_BOX_CELLS, "a path has at most as many points as its window has cells");
static_assert(SIMQ_GRID_PATH_MAX_BOX_CELLS / 3 < (1 << 15), "window coordinates fit 16 bits and keep the rule's products in range");
constexpr int kMaxLargeSide = 32765;               // a side of a window in a workspace: with the halo at most 32 767, coordinates < 2^15

struct Extents {
    int64_t cspace_bytes, thin_bytes, closest_ints, way_pairs;
    int n_upstream;
};

// kCapped: the window must fit LDS (simq_action_waypoint_problem); otherwise its sides stay under 2^15 with the halo
// (simq_action_waypoint_large_problem)
template <bool kCapped, typename Problem>
__device__ __forceinline__ bool descriptor_ok(const Problem& p, const uint8_t* thin, const int32_t* closest, const Extents& x) {
    if (p.rows < 1 || p.cols < 1 || (int64_t)p.rows * p.cols >= SIMQ_GRID_MAX_CELLS) return false;
    const int64_t cells = (int64_t)p.rows * p.cols;
    if (p.src_i < 0 || p.src_i >= p.rows || p.src_j < 0 || p.src_j >= p.cols) return false;
    if (p.tgt_i < 0 || p.tgt_i >= p.rows || p.tgt_j < 0 || p.tgt_j >= p.cols) return false;
    if (p.cspace_offset < 0 || p.cspace_offset > x.cspace_bytes - cells) return false;
    if (p.thin_offset < -1 || (p.thin_offset >= 0 && (!thin || p.thin_offset > x.thin_bytes - cells))) return false;
    if (p.closest_offset < -1 || (p.closest_offset >= 0 && (!closest || p.closest_offset > x.closest_ints - 2 * cells))) return false;
    if (p.way_capacity < 1 || p.way_offset < 0 || p.way_offset > x.way_pairs - p.way_capacity) return false;
    if (p.box_rows < 0 || p.box_cols < 0 || p.box_i0 < 0 || p.box_j0 < 0 || p.box_i0 > p.rows - p.box_rows ||
        p.box_j0 > p.cols - p.box_cols)
        return false;
    if (kCapped && (int64_t)(p.box_rows + 2) * (p.box_cols + 2) > SIMQ_GRID_PATH_MAX_BOX_CELLS) return false;
    if (!kCapped && (p.box_rows > kMaxLargeSide || p.box_cols > kMaxLargeSide)) return false;
    return p.upstream >= -1 && p.upstream < x.n_upstream;
}

// Where the state, and after the search the path and the kept flags, lie: the descriptor, the kernel's last argument, the rule that
// argument adds to the descriptor's, the memory (grid_waypoints.hip's pair, over this file's descriptors).
struct InLds {
    using Problem = simq_action_waypoint_problem;
    using State = Lds;
    using Arg = unsigned;                               // the dynamic LDS of the launch, bytes
    static constexpr bool kCapped = true;
    static __device__ __forceinline__ bool room(const Problem& p, Arg have) { return lds_bytes(p.box_rows, p.box_cols) <= (int64_t)have; }
    static __device__ __forceinline__ char* memory(const Problem&, Arg) {
        extern __shared__ __attribute__((aligned(16))) char smem[];
        return smem;
    }
};
struct InHbm {
    using Problem = simq_action_waypoint_large_problem;
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

template <typename Where>
__global__ void __launch_bounds__(kLanes) action_waypoints_kernel(const uint8_t* __restrict__ cspace, const uint8_t* __restrict__ thins,
                                                                  const int32_t* __restrict__ closest,
                                                                  const typename Where::Problem* __restrict__ probs,
                                                                  int2* __restrict__ ways, int32_t* __restrict__ counts,
                                                                  int32_t* __restrict__ endpoints, const int32_t* __restrict__ upstream,
                                                                  int32_t* __restrict__ status, Extents ext, typename Where::Arg where) {
    const typename Where::Problem p = probs[blockIdx.x];
    const int lane = threadIdx.x;
    if (!descriptor_ok<Where::kCapped>(p, thins, closest, ext) || !Where::room(p, where) || (p.upstream >= 0 && !upstream)) {
        if (lane == 0) status[blockIdx.x] = 2;          // (the host validated already: nothing is read or written)
        return;
    }
    if (p.upstream >= 0) {
        const int word = upstream[p.upstream];
        if (word != 0) {                                // e.g. a configuration space without a free cell: its closest cells are undefined
            if (lane == 0) {
                status[blockIdx.x] = word;
                counts[blockIdx.x] = 0;
            }
            return;
        }
    }
    const int R = p.rows, C = p.cols, n_cells = R * C;
    const uint8_t* g = cspace + p.cspace_offset;
    int si = p.src_i, sj = p.src_j, ti = p.tgt_i, tj = p.tgt_j;

    // ---- OccupancyMap.shortest_path's straight-line test, on the pixels as given (envs.py:2483-2485)
    if (p.thin_offset >= 0) {
        const uint8_t* thin = thins + p.thin_offset;
        if (!line_hits([&](int r, int c) { return thin[r * C + c] != 1; }, si, sj, ti, tj, lane)) {
            if (lane == 0) {
                status[blockIdx.x] = 1;
                counts[blockIdx.x] = 0;
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
    if (!free_cells_inside(g, n_cells, C, box, lane)) {
        if (lane == 0) status[blockIdx.x] = 2;
        return;
    }

    // ---- the search over the window + halo, its state where Where says; the flag bytes keep kOne for the pruning
    char* const smem = Where::memory(p, where);
    const typename Where::State lds(smem, box);
    const float inf = 2.f * (float)n_cells;              // self.inf = 2 * max_num_verts (exact: < 2^24)
    const bool tgt_in = box.holds(ti, tj);
    const int s_l = box.holds(si, sj) ? lds.index(box, si, sj) : -1;
    const int vertices = init_window<true>(lds, g, C, box, s_l, inf, lane);
    const bool searched = s_l >= 0 && (lds.flg[s_l] & kFree) != 0;   // edges leave a free cell only: a blocked source relaxes nothing
    int st = searched ? search<true>(lds, s_l, vertices + 1, lane) : 0;
    if (st != 0) {
        if (lane == 0) status[blockIdx.x] = st;
        return;
    }
    int2* way = ways + p.way_offset;
    int32_t* e = endpoints + 4 * (int64_t)blockIdx.x;

    // ---- a path of the target alone (an unreachable or blocked target, a blocked source, target == source, either outside the window)
    if (!searched || !tgt_in) {
        if (lane == 0) {
            way[0] = make_int2(ti, tj);
            counts[blockIdx.x] = 1;
            e[0] = si; e[1] = sj; e[2] = ti; e[3] = tj;
            status[blockIdx.x] = 0;
        }
        return;
    }

    // ---- the walk from the target (shortest_paths.pyx:126-137): window coordinates where the distances lay
    ushort2* path = reinterpret_cast<ushort2*>(smem);
    uint32_t* keep = reinterpret_cast<uint32_t*>(lds.ring);
    const int W = lds.W, N = lds.N;
    int n = 0;
    if (lane == 0) {
        int i = ti - box.i0 + 1, j = tj - box.j0 + 1;
        int v = i * W + j;
        path[0] = make_ushort2((unsigned short)i, (unsigned short)j);
        n = 1;
        while (v != s_l && n < N) {
            const int pk = lds.par[v];
            if (pk == kNoParent) break;
            i -= dir_di(pk);
            j -= dir_dj(pk);
            v -= dir_di(pk) * W + dir_dj(pk);
            path[n] = make_ushort2((unsigned short)i, (unsigned short)j);
            ++n;
        }
        if (v != s_l && n >= N) n = -1;                 // (a walk longer than the window has cells: the parents hold a cycle)
    }
    n = __shfl(n, 0, kLanes);
    if (n < 0) {
        if (lane == 0) status[blockIdx.x] = 4;
        return;
    }

    // ---- simplify (tolerance 1), prune, and the kept points last first as pixels of the grid (waypoint_rule.h)
    const uint8_t* flg = lds.flg;
    const int oi = box.i0 - 1, oj = box.j0 - 1;
    int total = 0;
    st = waypoint_rule::waypoints(
        keep, n, 1ull, p.way_capacity, [&](int k) { const ushort2 q = path[k]; return make_int2((int)q.x, (int)q.y); },
        [&](int r, int c) { return (flg[r * W + c] & kOne) == 0u; }, [&](int at, int2 q) { way[at] = make_int2(q.x + oi, q.y + oj); },
        lane, &total);
    if (lane == 0) {
        if (st == 0) {
            counts[blockIdx.x] = total;
            e[0] = si; e[1] = sj; e[2] = ti; e[3] = tj;
        }
        status[blockIdx.x] = st != 0 ? st : (total > p.way_capacity ? 3 : 0);
    }
}

// Every rule of the call and of its descriptor array that both entry points share (`who` names the entry point in the refusal), in
// the order the refusals come; `each(i, p)` holds the entry point's own rule for the window of problem i and returns 0 or -1 with
// the error set.
template <typename Problem, typename Each>
int check_problems(const char* who, const Problem* problems, int n, int64_t cspace_bytes, const uint8_t* d_thin, int64_t thin_bytes,
                   const int32_t* d_closest, int64_t closest_ints, int64_t way_pairs, const int32_t* d_upstream, int n_upstream, Each each) {
    SIMQ_REQUIRE(n >= 1 && n <= (1 << 24), "%s: n = %d (1 .. 2^24 problems)", who, n);
    SIMQ_REQUIRE(cspace_bytes >= 1 && way_pairs >= 1 && way_pairs <= ((int64_t)1 << 40) && thin_bytes >= 0 && closest_ints >= 0,
                 "%s: extents of %lld bytes of d_cspace, %lld of d_thin, %lld ints of d_closest, %lld pairs of d_ways "
                 "(d_cspace and d_ways >= 1, pairs <= 2^40, none negative)", who, (long long)cspace_bytes, (long long)thin_bytes,
                 (long long)closest_ints, (long long)way_pairs);
    SIMQ_REQUIRE(n_upstream >= 0 && (n_upstream == 0) == (d_upstream == nullptr),
                 "%s: d_upstream and n_upstream = %d (NULL with 0, or n_upstream >= 1 words)", who, n_upstream);
    std::vector<Span> way_spans;
    way_spans.reserve(n);
    for (int i = 0; i < n; ++i) {
        const Problem& p = problems[i];
        SIMQ_REQUIRE(p.rows >= 1 && p.cols >= 1 && (int64_t)p.rows * p.cols < SIMQ_GRID_MAX_CELLS,
                     "%s: problem %d is %d x %d (rows, cols >= 1, rows * cols < 2^22)", who, i, p.rows, p.cols);
        SIMQ_REQUIRE(p.src_i >= 0 && p.src_i < p.rows && p.src_j >= 0 && p.src_j < p.cols,
                     "%s: problem %d: source (%d, %d) outside its %d x %d grid", who, i, p.src_i, p.src_j, p.rows, p.cols);
        SIMQ_REQUIRE(p.tgt_i >= 0 && p.tgt_i < p.rows && p.tgt_j >= 0 && p.tgt_j < p.cols,
                     "%s: problem %d: target (%d, %d) outside its %d x %d grid", who, i, p.tgt_i, p.tgt_j, p.rows, p.cols);
        const int64_t cells = (int64_t)p.rows * p.cols;
        SIMQ_REQUIRE(fits(p.cspace_offset, cells, cspace_bytes), "%s: problem %d: cspace_offset: bytes [%lld, %lld) outside the %lld of d_cspace",
                     who, i, (long long)p.cspace_offset, (long long)(p.cspace_offset + cells), (long long)cspace_bytes);
        SIMQ_REQUIRE(p.thin_offset == -1 || (d_thin && fits(p.thin_offset, cells, thin_bytes)),
                     "%s: problem %d: thin_offset: bytes [%lld, %lld) outside the %lld of d_thin (-1: no straight-line test)", who, i,
                     (long long)p.thin_offset, (long long)(p.thin_offset + cells), (long long)(d_thin ? thin_bytes : 0));
        SIMQ_REQUIRE(p.closest_offset == -1 || (d_closest && fits(p.closest_offset, 2 * cells, closest_ints)),
                     "%s: problem %d: closest_offset: ints [%lld, %lld) outside the %lld of d_closest (-1: no snap)", who, i,
                     (long long)p.closest_offset, (long long)(p.closest_offset + 2 * cells), (long long)(d_closest ? closest_ints : 0));
        SIMQ_REQUIRE(p.box_rows >= 0 && p.box_cols >= 0 && p.box_i0 >= 0 && p.box_j0 >= 0 && p.box_i0 <= p.rows - p.box_rows &&
                         p.box_j0 <= p.cols - p.box_cols,
                     "%s: problem %d: window rows [%d, %d + %d), columns [%d, %d + %d) outside its %d x %d grid", who, i, p.box_i0, p.box_i0,
                     p.box_rows, p.box_j0, p.box_j0, p.box_cols, p.rows, p.cols);
        if (each(i, p) != 0) return -1;
        SIMQ_REQUIRE(p.way_capacity >= 1, "%s: problem %d: way_capacity = %d (>= 1 pair)", who, i, p.way_capacity);
        SIMQ_REQUIRE(fits(p.way_offset, p.way_capacity, way_pairs), "%s: problem %d: way_offset: pairs [%lld, %lld) outside the %lld of d_ways",
                     who, i, (long long)p.way_offset, (long long)(p.way_offset + p.way_capacity), (long long)way_pairs);
        SIMQ_REQUIRE(p.upstream >= -1 && p.upstream < n_upstream, "%s: problem %d: upstream = %d (-1, or a word of the %d of d_upstream)", who, i,
                     p.upstream, n_upstream);
        way_spans.push_back({(uint64_t)p.way_offset, (uint64_t)(p.way_offset + p.way_capacity), i});
    }
    const size_t o = first_overlap(way_spans);
    SIMQ_REQUIRE(o == 0, "%s: problems %d and %d overlap in d_ways at pair %lld", who, way_spans[o - 1].problem, way_spans[o].problem,
                 (long long)way_spans[o].lo);
    return 0;
}

// alignment of every buffer, then every buffer the launch writes against every other buffer of the call
int check_buffers(const char* who, const Buffer* bufs, const int* align, int nb) {
    for (int a = 0; a < nb; ++a) SIMQ_REQUIRE((uintptr_t)bufs[a].p % align[a] == 0, "%s: %s is not %d-byte aligned", who, bufs[a].name, align[a]);
    int a = 0, b = 0;
    SIMQ_REQUIRE(!first_conflict(bufs, nb, &a, &b), "%s: %s and %s overlap", who, bufs[a].name, bufs[b].name);
    return 0;
}

}  // namespace

}  // namespace simq

using namespace simq;

extern "C" int simq_action_waypoints(const uint8_t* d_cspace, int64_t cspace_bytes, const uint8_t* d_thin, int64_t thin_bytes,
                                     const int32_t* d_closest, int64_t closest_ints, const simq_action_waypoint_problem* problems, int n,
                                     simq_action_waypoint_problem* d_problems, int32_t* d_ways, int64_t way_pairs, int32_t* d_counts,
                                     int32_t* d_endpoints, const int32_t* d_upstream, int n_upstream, int32_t* d_status, void* stream) {
    static const char who[] = "action_waypoints";
    SIMQ_REQUIRE(d_cspace && problems && d_problems && d_ways && d_counts && d_endpoints && d_status, "%s: NULL pointer", who);
    int64_t lds = 0;
    const auto under_the_cap = [&](int i, const simq_action_waypoint_problem& p) {
        SIMQ_REQUIRE((int64_t)(p.box_rows + 2) * (p.box_cols + 2) <= SIMQ_GRID_PATH_MAX_BOX_CELLS,
                     "%s: problem %d: window of %d x %d cells plus its halo is %lld cells, over SIMQ_GRID_PATH_MAX_BOX_CELLS = %d "
                     "(the search state lives in LDS)", who, i, p.box_rows, p.box_cols, (long long)(p.box_rows + 2) * (p.box_cols + 2),
                     SIMQ_GRID_PATH_MAX_BOX_CELLS);
        lds = std::max(lds, lds_bytes(p.box_rows, p.box_cols));
        return 0;
    };
    if (check_problems(who, problems, n, cspace_bytes, d_thin, thin_bytes, d_closest, closest_ints, way_pairs, d_upstream, n_upstream,
                       under_the_cap) != 0)
        return -1;
    const Buffer bufs[] = {
        {"d_cspace", d_cspace, cspace_bytes, false},
        {"d_thin", d_thin, d_thin ? thin_bytes : 0, false},
        {"d_closest", d_closest, d_closest ? 4 * closest_ints : 0, false},
        {"d_upstream", d_upstream, 4 * (int64_t)n_upstream, false},
        {"d_problems", d_problems, (int64_t)sizeof(simq_action_waypoint_problem) * n, true},
        {"d_ways", d_ways, 8 * way_pairs, true},
        {"d_counts", d_counts, 4 * (int64_t)n, true},
        {"d_endpoints", d_endpoints, 16 * (int64_t)n, true},
        {"d_status", d_status, 4 * (int64_t)n, true},
    };
    const int align[] = {1, 1, 4, 4, 8, 8, 4, 4, 4};
    if (check_buffers(who, bufs, align, (int)(sizeof(bufs) / sizeof(bufs[0]))) != 0) return -1;
    lds = (lds + 15) & ~(int64_t)15;
    SIMQ_REQUIRE(lds <= kLdsBudget, "%s: %lld bytes of LDS over the %d of a compute unit", who, (long long)lds, kLdsBudget);

    hipStream_t s = static_cast<hipStream_t>(stream);
    SIMQ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(action_waypoints_kernel<InLds>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kLdsBudget));
    const HostBlock block = {problems, sizeof(simq_action_waypoint_problem) * (size_t)n};
    SIMQ_CHECK_HIP(upload_descriptors(d_problems, &block, 1, nullptr, s));
    const Extents ext = {cspace_bytes, d_thin ? thin_bytes : 0, d_closest ? closest_ints : 0, way_pairs, n_upstream};
    action_waypoints_kernel<InLds><<<n, kLanes, (size_t)lds, s>>>(d_cspace, d_thin, d_closest, d_problems, reinterpret_cast<int2*>(d_ways),
                                                                  d_counts, d_endpoints, d_upstream, d_status, ext, (unsigned)lds);
    SIMQ_CHECK_LAUNCH();
    note_launch("action_waypoints");
    return 0;
}

extern "C" int64_t simq_action_waypoints_large_work_bytes(int32_t box_rows, int32_t box_cols) {
    if (box_rows < 0 || box_cols < 0 || box_rows > kMaxLargeSide || box_cols > kMaxLargeSide ||
        (int64_t)box_rows * box_cols >= SIMQ_GRID_MAX_CELLS)
        return -1;
    return work_bytes(box_rows, box_cols);
}

extern "C" int simq_action_waypoints_large(const uint8_t* d_cspace, int64_t cspace_bytes, const uint8_t* d_thin, int64_t thin_bytes,
                                           const int32_t* d_closest, int64_t closest_ints,
                                           const simq_action_waypoint_large_problem* problems, int n,
                                           simq_action_waypoint_large_problem* d_problems, int32_t* d_ways, int64_t way_pairs,
                                           int32_t* d_counts, int32_t* d_endpoints, const int32_t* d_upstream, int n_upstream,
                                           int32_t* d_status, void* d_work, int64_t work_bytes_have, void* stream) {
    static const char who[] = "action_waypoints_large";
    SIMQ_REQUIRE(d_cspace && problems && d_problems && d_ways && d_counts && d_endpoints && d_status && d_work, "%s: NULL pointer", who);
    SIMQ_REQUIRE(work_bytes_have >= 0 && work_bytes_have < (1LL << 40), "%s: work_bytes = %lld (in [0, 2^40))", who,
                 (long long)work_bytes_have);
    std::vector<Span> work_spans;
    const auto inside_the_workspace = [&](int i, const simq_action_waypoint_large_problem& p) {
        SIMQ_REQUIRE(p.box_rows <= kMaxLargeSide && p.box_cols <= kMaxLargeSide,
                     "%s: problem %d: window of %d x %d cells (each side at most %d: with the halo below 2^15)", who, i, p.box_rows, p.box_cols,
                     kMaxLargeSide);
        const int64_t need = work_bytes(p.box_rows, p.box_cols);
        SIMQ_REQUIRE(p.work_offset % 16 == 0 && fits(p.work_offset, need, work_bytes_have),
                     "%s: problem %d: work_offset: bytes [%lld, %lld) outside the %lld of d_work, or not at a multiple of 16", who, i,
                     (long long)p.work_offset, (long long)(p.work_offset + need), (long long)work_bytes_have);
        work_spans.push_back({(uint64_t)p.work_offset, (uint64_t)(p.work_offset + need), i});
        return 0;
    };
    if (check_problems(who, problems, n, cspace_bytes, d_thin, thin_bytes, d_closest, closest_ints, way_pairs, d_upstream, n_upstream,
                       inside_the_workspace) != 0)
        return -1;
    const size_t o = first_overlap(work_spans);
    SIMQ_REQUIRE(o == 0, "%s: problems %d and %d overlap in d_work at byte %lld", who, work_spans[o - 1].problem, work_spans[o].problem,
                 (long long)work_spans[o].lo);
    const Buffer bufs[] = {
        {"d_cspace", d_cspace, cspace_bytes, false},
        {"d_thin", d_thin, d_thin ? thin_bytes : 0, false},
        {"d_closest", d_closest, d_closest ? 4 * closest_ints : 0, false},
        {"d_upstream", d_upstream, 4 * (int64_t)n_upstream, false},
        {"d_problems", d_problems, (int64_t)sizeof(simq_action_waypoint_large_problem) * n, true},
        {"d_ways", d_ways, 8 * way_pairs, true},
        {"d_counts", d_counts, 4 * (int64_t)n, true},
        {"d_endpoints", d_endpoints, 16 * (int64_t)n, true},
        {"d_status", d_status, 4 * (int64_t)n, true},
        {"d_work", d_work, work_bytes_have, true},
    };
    const int align[] = {1, 1, 4, 4, 8, 8, 4, 4, 4, 16};
    if (check_buffers(who, bufs, align, (int)(sizeof(bufs) / sizeof(bufs[0]))) != 0) return -1;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const HostBlock block = {problems, sizeof(simq_action_waypoint_large_problem) * (size_t)n};
    SIMQ_CHECK_HIP(upload_descriptors(d_problems, &block, 1, nullptr, s));
    const Extents ext = {cspace_bytes, d_thin ? thin_bytes : 0, d_closest ? closest_ints : 0, way_pairs, n_upstream};
    action_waypoints_kernel<InHbm><<<n, kLanes, 0, s>>>(d_cspace, d_thin, d_closest, d_problems, reinterpret_cast<int2*>(d_ways), d_counts,
                                                        d_endpoints, d_upstream, d_status, ext,
                                                        InHbm::Arg{static_cast<char*>(d_work), work_bytes_have});
    SIMQ_CHECK_LAUNCH();
    note_launch("action_waypoints_large");
    return 0;
}
