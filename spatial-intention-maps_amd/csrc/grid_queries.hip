// libsimq: batched shortest-path distance queries on 8-connected grids -- the point form of grid_paths.hip
//   grid_queries_kernel      OccupancyMap.shortest_path_distance without its division: the snap of source and targets through
//                            closest_cspace_indices, GridGraph._spfa's distances, the lookup at each target
//                            (envs.py:2506-2511 -> shortest_paths.pyx:150-158; the partial rewards of envs.py:1082-1087, 1210-1215, 1331-1335)
//
// One problem = one grid, one source pixel and Q >= 0 target pixels; one wavefront per problem.  The wave snaps the source, runs
// the relaxation of grid_relax.h to its fixed point in the problem's working image (the arithmetic and the stopping rule of
// grid_paths.hip: one fp32 add per update, a whole pass without improvement), then its lanes stride over the targets: snap, load the
// label, store it (-1 where the label is still inf).  A receptacle-sourced search therefore serves every cube of its map, and the
// distances of a whole step come back in one packed array.  No atomics, no second launch.
//
// Visibility.  The labels the epilogue loads were stored by other lanes of the same wave.  The relaxation has that hazard already -- a
// pass re-reads, through load_row, the rows the previous pass stored -- and closes it with __threadfence_block() after every column
// block (and after the initialisation); the epilogue relies on the same fences and adds one after the optional -1 fill.  The working
// image is never `__restrict__`, so the compiler keeps loads and stores to it in program order across the fences.
#include "batch_abi.h"
#include "grid_relax.h"
#include "grid_spfa.h"
#include "../../include/simq.h"

#include <vector>

namespace simq {

namespace {

using namespace grid_relax;
using grid_spfa::snap;

__global__ void __launch_bounds__(kLanes) grid_queries_kernel(const uint8_t* __restrict__ grids, const int32_t* __restrict__ closest,
                                                              const simq_grid_query_problem* __restrict__ probs,
                                                              const int32_t* __restrict__ targets, float* work, int images,
                                                              float* __restrict__ out, int32_t* __restrict__ status, int64_t grids_bytes,
                                                              int64_t closest_ints, int64_t work_floats, int64_t n_targets_total) {
    const simq_grid_query_problem p = probs[blockIdx.x];
    const int lane = threadIdx.x;
    const int R = p.rows, C = p.cols;
    if (R < 1 || C < 1 || (int64_t)R * C >= SIMQ_GRID_MAX_CELLS || p.src_i < 0 || p.src_i >= R || p.src_j < 0 || p.src_j >= C ||
        p.grid_offset < 0 || p.grid_offset > grids_bytes - (int64_t)R * C || p.work_offset < 0 ||
        p.work_offset > work_floats - (int64_t)R * C || p.n_targets < 0 || p.target_offset < 0 ||
        p.target_offset > n_targets_total - p.n_targets || p.closest_offset < -1 ||
        (p.closest_offset >= 0 && (!closest || p.closest_offset > closest_ints - 2 * (int64_t)R * C))) {
        if (lane == 0) status[blockIdx.x] = 2;          // (the host validated already: nothing is read or written)
        return;
    }
    const int n = R * C;
    const uint8_t* g = grids + p.grid_offset;
    const int32_t* cl = p.closest_offset >= 0 ? closest + p.closest_offset : nullptr;
    float* d = work + p.work_offset;
    const float inf = 2.f * (float)n;                    // self.inf = 2 * max_num_verts (exact: < 2^24)

    // ---- OccupancyMap._closest_valid_cspace_indices on the source (envs.py:2509, 2522-2523)
    int si = p.src_i, sj = p.src_j;
    if (cl && !snap(cl, R, C, si, sj)) {
        if (lane == 0) status[blockIdx.x] = 2;
        return;
    }

    // ---- GridGraph._spfa's distances (shortest_paths.pyx:69-114)
    const Box box = init_labels(g, d, R, C, si * C + sj, inf, lane);
    float dmax;                                          // (the distance images' epilogue needs it; nothing here does)
    const bool capped = relax_passes(g, d, box, n, inf, lane, &dmax);

    // ---- the image as simq_grid_distance_images leaves it without its epilogue: -1 where unreachable
    if (images) {
        for (int i = lane; i < n; i += kLanes)
            if (d[i] == inf) d[i] = -1.f;
        __threadfence_block();                           // the lookups below read cells other lanes have just filled
    }

    // ---- the queries: snap each target (envs.py:2510), read its label (shortest_paths.pyx:150-158)
    const int32_t* tg = targets + 2 * p.target_offset;
    float* o = out + p.target_offset;
    bool bad = false;
    for (int q = lane; q < p.n_targets; q += kLanes) {
        int ti = tg[2 * q], tj = tg[2 * q + 1];
        if (ti < 0 || ti >= R || tj < 0 || tj >= C || (cl && !snap(cl, R, C, ti, tj))) {
            bad = true;
            continue;
        }
        const float x = d[ti * C + tj];
        o[q] = x == inf ? -1.f : x;
    }
    bad = __any(bad);
    if (lane == 0) status[blockIdx.x] = bad ? 2 : (capped ? 1 : 0);
}

}  // namespace

}  // namespace simq

using namespace simq;

extern "C" int simq_grid_distance_queries(const uint8_t* d_grids, int64_t grids_bytes, const int32_t* d_closest, int64_t closest_ints,
                                          const simq_grid_query_problem* problems, int n, const int32_t* targets, int64_t n_targets_total,
                                          void* d_descriptors, float* d_work, int64_t work_floats, int images, float* d_out,
                                          int64_t out_floats, int32_t* d_status, void* stream) {
    SIMQ_REQUIRE(d_grids && problems && d_descriptors && d_work && d_status, "grid_distance_queries: NULL pointer");
    SIMQ_REQUIRE(n >= 1 && n <= (1 << 24), "grid_distance_queries: n = %d (1 .. 2^24 problems)", n);
    SIMQ_REQUIRE(n_targets_total >= 0 && n_targets_total <= (1LL << 32), "grid_distance_queries: n_targets_total = %lld (0 .. 2^32)",
                 (long long)n_targets_total);
    SIMQ_REQUIRE(n_targets_total == 0 || (targets && d_out), "grid_distance_queries: NULL targets or d_out with %lld targets",
                 (long long)n_targets_total);
    SIMQ_REQUIRE(images == 0 || images == 1, "grid_distance_queries: images = %d (0: the working images are scratch, 1: outputs)", images);
    SIMQ_REQUIRE(grids_bytes >= 0 && closest_ints >= 0 && work_floats >= 0 && out_floats >= 0 && grids_bytes < (1LL << 40) &&
                     closest_ints < (1LL << 40) && work_floats < (1LL << 40) && out_floats < (1LL << 40),
                 "grid_distance_queries: buffer sizes %lld, %lld, %lld, %lld (each in [0, 2^40))", (long long)grids_bytes,
                 (long long)closest_ints, (long long)work_floats, (long long)out_floats);
    SIMQ_REQUIRE(out_floats >= n_targets_total, "grid_distance_queries: d_out holds %lld floats, the targets need %lld", (long long)out_floats,
                 (long long)n_targets_total);
    SIMQ_REQUIRE(((uintptr_t)d_descriptors & 7) == 0 && ((uintptr_t)d_closest & 3) == 0 && ((uintptr_t)d_work & 3) == 0 &&
                     ((uintptr_t)d_out & 3) == 0 && ((uintptr_t)d_status & 3) == 0,
                 "grid_distance_queries: d_descriptors must be 8-byte, d_closest, d_work, d_out and d_status 4-byte aligned");
    std::vector<Span> work_spans, out_spans;
    work_spans.reserve(n);
    out_spans.reserve(n);
    for (int i = 0; i < n; ++i) {
        const simq_grid_query_problem& p = problems[i];
        SIMQ_REQUIRE(p.rows >= 1 && p.cols >= 1 && (int64_t)p.rows * p.cols < SIMQ_GRID_MAX_CELLS,
                     "grid_distance_queries: problem %d is %d x %d (rows, cols >= 1, rows * cols < 2^22)", i, p.rows, p.cols);
        SIMQ_REQUIRE(p.src_i >= 0 && p.src_i < p.rows && p.src_j >= 0 && p.src_j < p.cols,
                     "grid_distance_queries: problem %d: source (%d, %d) outside its %d x %d grid", i, p.src_i, p.src_j, p.rows, p.cols);
        const int64_t cells = (int64_t)p.rows * p.cols;
        SIMQ_REQUIRE(fits(p.grid_offset, cells, grids_bytes),
                     "grid_distance_queries: problem %d: grid bytes [%lld, %lld) outside the %lld of d_grids", i, (long long)p.grid_offset,
                     (long long)(p.grid_offset + cells), (long long)grids_bytes);
        SIMQ_REQUIRE(p.closest_offset == -1 || (d_closest && fits(p.closest_offset, 2 * cells, closest_ints)),
                     "grid_distance_queries: problem %d: closest ints [%lld, %lld) outside the %lld of d_closest (-1: no snap)", i,
                     (long long)p.closest_offset, (long long)(p.closest_offset + 2 * cells), (long long)(d_closest ? closest_ints : 0));
        SIMQ_REQUIRE(fits(p.work_offset, cells, work_floats),
                     "grid_distance_queries: problem %d: working image floats [%lld, %lld) outside the %lld of d_work", i,
                     (long long)p.work_offset, (long long)(p.work_offset + cells), (long long)work_floats);
        SIMQ_REQUIRE(p.n_targets >= 0 && fits(p.target_offset, p.n_targets, n_targets_total),
                     "grid_distance_queries: problem %d: targets [%lld, %lld) outside the %lld of the call", i, (long long)p.target_offset,
                     (long long)(p.target_offset + p.n_targets), (long long)n_targets_total);
        for (int64_t q = p.target_offset; q < p.target_offset + p.n_targets; ++q) {
            const int ti = targets[2 * q], tj = targets[2 * q + 1];
            SIMQ_REQUIRE(ti >= 0 && ti < p.rows && tj >= 0 && tj < p.cols,
                         "grid_distance_queries: problem %d: target %lld (%d, %d) outside its %d x %d grid", i, (long long)(q - p.target_offset),
                         ti, tj, p.rows, p.cols);
        }
        work_spans.push_back({(uint64_t)p.work_offset, (uint64_t)(p.work_offset + cells), i});
        if (p.n_targets > 0) out_spans.push_back({(uint64_t)p.target_offset, (uint64_t)(p.target_offset + p.n_targets), i});
    }
    size_t clash = first_overlap(work_spans);
    SIMQ_REQUIRE(clash == 0, "grid_distance_queries: problems %d and %d share working image floats from %lld on", work_spans[clash - 1].problem,
                 work_spans[clash].problem, (long long)work_spans[clash].lo);
    clash = first_overlap(out_spans);
    SIMQ_REQUIRE(clash == 0, "grid_distance_queries: problems %d and %d share d_out (and target) entries from %lld on",
                 out_spans[clash - 1].problem, out_spans[clash].problem, (long long)out_spans[clash].lo);

    // every buffer the launch writes against every other buffer of the call (an absent or empty buffer takes no part)
    const int64_t prob_bytes = (int64_t)sizeof(simq_grid_query_problem) * n;
    const Buffer all[] = {{"d_work", d_work, 4 * work_floats, true},
                          {"d_out", d_out, d_out ? 4 * out_floats : 0, true},
                          {"d_status", d_status, 4LL * n, true},
                          {"d_descriptors", d_descriptors, prob_bytes + 8 * n_targets_total, true},
                          {"d_grids", d_grids, grids_bytes, false},
                          {"d_closest", d_closest, d_closest ? 4 * closest_ints : 0, false}};
    Buffer bufs[6];
    int nb = 0;
    for (const Buffer& b : all)
        if (b.p && b.bytes > 0) bufs[nb++] = b;
    int a = 0, b = 0;
    SIMQ_REQUIRE(!first_conflict(bufs, nb, &a, &b), "grid_distance_queries: %s overlaps %s", bufs[a].name, bufs[b].name);

    hipStream_t s = static_cast<hipStream_t>(stream);
    const HostBlock blocks[2] = {{problems, (size_t)prob_bytes}, {targets, (size_t)(8 * n_targets_total)}};
    const char* at[2] = {nullptr, nullptr};
    SIMQ_CHECK_HIP(upload_descriptors(d_descriptors, blocks, n_targets_total > 0 ? 2 : 1, at, s));
    grid_queries_kernel<<<n, kLanes, 0, s>>>(d_grids, d_closest, reinterpret_cast<const simq_grid_query_problem*>(at[0]),
                                             reinterpret_cast<const int32_t*>(at[1]), d_work, images, d_out, d_status, grids_bytes,
                                             d_closest ? closest_ints : 0, work_floats, n_targets_total);
    SIMQ_CHECK_LAUNCH();
    note_launch("grid_queries");
    return 0;
}
