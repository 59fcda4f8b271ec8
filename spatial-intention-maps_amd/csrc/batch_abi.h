// What the C entry points of the batched map operators share (grid_paths, grid_queries, grid_waypoints, action_waypoints, local_maps, intention_maps,
// occupancy_maps, observation_maps, visualization): the checks that keep a bad descriptor from becoming a fault, the descriptor upload, and the
// NaN-keeping reduction of two of the kernels.  Nothing here knows an operator.  The helpers report -- a bool, an index, a pair -- and
// the entry point words the refusal: every SIMQ_REQUIRE and its text stay with the operator.
#pragma once
#include "common.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace simq {

// ---- host: ranges ------------------------------------------------------------------------------------------------------------------

// [a, a + na) and [b, b + nb) (bytes) share a byte
inline bool overlaps(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

// `count` elements from `offset` on lie inside a buffer of `capacity` elements.  Usable on the device too, but the kernels' own
// descriptor checks (which guard a launch whose descriptors were changed behind the host's back) keep the expression spelled out: the
// compiler chains six calls of this differently (3 to 9 more instructions per workgroup, and the observation kernel measured 1-2 %
// slower), and this header changes no kernel's code
__host__ __device__ inline bool fits(int64_t offset, int64_t count, int64_t capacity) {
    return offset >= 0 && offset <= capacity - count;
}

// [lo, hi) of one problem's output: element offsets into one buffer, or addresses
struct Span {
    uint64_t lo, hi;
    int problem;
};

inline bool span_before(const Span& a, const Span& b) { return a.lo < b.lo; }

// sorts `spans` by lo and returns the index i >= 1 of the first span that begins inside its predecessor (spans[i - 1] and spans[i]
// overlap), 0 when all are disjoint.  Spans are never empty, so two that begin together overlap, and which i comes first and its lo
// do not depend on how the sort orders equal keys.
inline size_t first_overlap(std::vector<Span>& spans) {
    std::sort(spans.begin(), spans.end(), span_before);
    for (size_t i = 1; i < spans.size(); ++i)
        if (spans[i].lo < spans[i - 1].hi) return i;
    return 0;
}

// one buffer of a call, for the check of every buffer the launch writes against every other buffer of the call
struct Buffer {
    const char* name;
    const void* p;
    int64_t bytes;
    bool written;
};

// the first pair a < b (in table order) that overlaps with at least one of the two written; false when there is none
inline bool first_conflict(const Buffer* bufs, int n, int* a_out, int* b_out) {
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b)
            if ((bufs[a].written || bufs[b].written) && overlaps(bufs[a].p, bufs[a].bytes, bufs[b].p, bufs[b].bytes)) {
                *a_out = a;
                *b_out = b;
                return true;
            }
    return false;
}

// ---- host: slot tables -------------------------------------------------------------------------------------------------------------
// A call that writes item p to pool + slots[p] * item_bytes (simq_replay_scatter, simq_local_state_images_slots) checks its host table
// with these two: nothing else of the pool is the call's business, so buffers the launch reads may lie in the pool's other slots.

// `sorted` receives the n slots in ascending order.  0: every slot lies in [0, pool_slots) and none is named twice; 1: *which lies
// outside the pool; 2: *which is named twice.
inline int check_slots(const int64_t* slots, int n, int64_t pool_slots, std::vector<int64_t>& sorted, int64_t* which) {
    for (int p = 0; p < n; ++p)
        if (slots[p] < 0 || slots[p] >= pool_slots) {
            *which = slots[p];
            return 1;
        }
    sorted.assign(slots, slots + n);
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 1; i < sorted.size(); ++i)
        if (sorted[i] == sorted[i - 1]) {
            *which = sorted[i];
            return 2;
        }
    return 0;
}

// a slot of `sorted` (ascending, each in [0, pool_slots)) whose bytes [pool + slot * item_bytes, + item_bytes) share a byte with
// [p, p + bytes); -1 when there is none
inline int64_t written_slot_in(const std::vector<int64_t>& sorted, const void* pool, int64_t item_bytes, int64_t pool_slots, const void* p,
                               int64_t bytes) {
    if (bytes <= 0 || !overlaps(pool, pool_slots * item_bytes, p, bytes)) return -1;
    const uintptr_t base = (uintptr_t)pool, lo = (uintptr_t)p, hi = lo + (uintptr_t)bytes - 1;        // (hi: the last byte)
    const int64_t first = lo <= base ? 0 : (int64_t)((lo - base) / (uintptr_t)item_bytes);
    const int64_t last = std::min<int64_t>(pool_slots - 1, (int64_t)((hi - base) / (uintptr_t)item_bytes));
    const auto it = std::lower_bound(sorted.begin(), sorted.end(), first);
    return it != sorted.end() && *it <= last ? *it : -1;
}

// ---- host: the descriptor upload ---------------------------------------------------------------------------------------------------

struct HostBlock {
    const void* src;
    size_t bytes;
};

// Packs `n` host blocks end to end into d_dst with one hipMemcpyAsync on `s`; at[k] (at: NULL, or n entries) is where block k lies on
// the device.  Several blocks go through one staging vector, one block is copied from where it is.
// The source is pageable memory that dies on return (the staging vector) or may (the caller's array): the runtime finishes a pageable
// host-to-device copy (staged behind the stream's earlier work) before hipMemcpyAsync returns, which is what makes this safe -- and what
// makes the call block the host until `s` has drained.
inline hipError_t upload_descriptors(void* d_dst, const HostBlock* blocks, int n, const char** at, hipStream_t s) {
    if (n == 1) {
        if (at) at[0] = static_cast<const char*>(d_dst);
        return hipMemcpyAsync(d_dst, blocks[0].src, blocks[0].bytes, hipMemcpyHostToDevice, s);
    }
    size_t total = 0;
    for (int k = 0; k < n; ++k) total += blocks[k].bytes;
    std::vector<char> host(total);
    size_t off = 0;
    for (int k = 0; k < n; ++k) {
        if (at) at[k] = static_cast<const char*>(d_dst) + off;
        if (blocks[k].bytes) std::memcpy(host.data() + off, blocks[k].src, blocks[k].bytes);
        off += blocks[k].bytes;
    }
    return hipMemcpyAsync(d_dst, host.data(), total, hipMemcpyHostToDevice, s);
}

// ---- device: reductions that keep a NaN --------------------------------------------------------------------------------------------

// minimum / maximum that keep a NaN, as ndarray.min() / max() do (fminf / fmaxf would drop it): a map or an output holding a NaN gives
// an all-NaN image, as in the reference.  Which of +0 / -0 is the minimum of a set holding both is not fixed here (nor by numpy's
// vectorised min).
__device__ __forceinline__ float min_nan(float a, float b) {
    return a != a ? a : (b != b ? b : (b < a ? b : a));
}
__device__ __forceinline__ float max_nan(float a, float b) {
    return a != a ? a : (b != b ? b : (b > a ? b : a));
}

// The block reduction in its two halves: every lane's value over its wavefront (shuffles) ...
template <typename Op>
__device__ __forceinline__ float wave_reduce(float v, Op op) {
    for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
// ... and, once lane 0 of every wave has stored its result in LDS and the block has synchronised, those `waves` values in order
template <typename Op>
__device__ __forceinline__ float reduce_waves(const float* part, int waves, Op op) {
    float w = part[0];
    for (int k = 1; k < waves; ++k) w = op(w, part[k]);
    return w;
}

}  // namespace simq
