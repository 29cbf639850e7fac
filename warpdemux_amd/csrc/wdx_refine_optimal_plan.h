// The scratch plan of the optimal change-points (WDX_OPT_REFINE_OPTIMAL_CPTS; wdx_refine_optimal.hip): how long a tail a
// workgroup's slot holds, what a slot costs and how many workgroups a launch gets -- the one statement of the rule (plain
// host C++17: no HIP, nothing of the context, so the system compiler builds it alone: tests/host/optimal_plan_check.cpp).
//
// A grid of `slots` workgroups strides over the reads; each owns `slot_bytes` of the context's scratch buffer: the path table
// of the read in flight (16-bit entries, B rows of cap + 1) and, only when the launch was sized for tails beyond kOptLdsCap
// samples, its prefix sums and two rows of the value table (four arrays of cap + 1 doubles).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/wdx.h"

namespace wdx {

constexpr int kOptLdsCap = 2047;                    // tails whose prefix sums and value rows live in LDS
constexpr size_t kOptScratchMax = (size_t)256 << 20;   // upper bound of the scratch buffer
constexpr int64_t kOptMaxSlots = 2048;
struct OptimalPlan {
    int64_t cap;         // longest tail a slot holds
    size_t slot_bytes;
    int64_t slots;
    size_t bytes;        // slots * slot_bytes <= kOptScratchMax
};

// bytes of one workgroup's slot for tails of up to `cap` samples and B change-points
inline size_t optimal_slot_bytes(int64_t cap, int B) {
    size_t b = ((size_t)B * (size_t)(cap + 1) * 2 + 15) & ~(size_t)15;
    if (cap > kOptLdsCap) b += (size_t)4 * (size_t)(cap + 1) * 8;
    return (b + 255) & ~(size_t)255;
}
inline int64_t optimal_tail_cap(int64_t max_len) {
    // (the exact kernel's LDS carve-up rounds max_len up to a multiple of 64 samples: so does this bound)
    return std::min<int64_t>((std::max<int64_t>(max_len, 64) + 63) / 64 * 64, WDX_MAX_ADAPTER_SAMPLES);
}

inline OptimalPlan plan_refine_optimal(int64_t n_reads, int64_t max_len, int B, int64_t max_slots = 0) {
    OptimalPlan pl{};
    pl.cap = optimal_tail_cap(max_len);
    pl.slot_bytes = optimal_slot_bytes(pl.cap, B < 1 ? 1 : B);
    int64_t slots = (int64_t)(kOptScratchMax / pl.slot_bytes);   // (the largest slot, B = 253 at 16 384 samples, is 8.4 MiB)
    slots = std::min<int64_t>(slots, kOptMaxSlots);
    if (max_slots > 0) slots = std::min(slots, max_slots);
    slots = std::min(slots, n_reads);
    pl.slots = std::max<int64_t>(slots, 1);
    pl.bytes = (size_t)pl.slots * pl.slot_bytes;
    return pl;
}

}  // namespace wdx
