// Stand-alone sweep of warpdemux_amd/csrc/wdx_refine_optimal_plan.h -- the slot plan of the optimal change-points
// (WDX_OPT_REFINE_OPTIMAL_CPTS) -- built by tests/test_optimal_plan_host.py with the system compiler and the address /
// undefined-behaviour sanitizers.  n_reads in {1, 2, 9, 199, 200, 2048, 2049, 10^6}, max_len in {1, 63, 64, 65, 2047, 2048,
// 2049, 11 264, 16 383, 16 384}, B in {1, 25, 60, 253}, max_slots in {0, 1, 2}.  stdout: one line per case, "n_reads max_len B
// max_slots cap slot_bytes slots bytes".  The program itself checks what must hold of every plan: a slot holds the path table
// (and, beyond the LDS cap, four arrays of doubles behind it at a 16-byte boundary), slots are whole multiples of 256 bytes,
// there is at least one and the buffer stays within its bound.
#include "wdx_refine_optimal_plan.h"

#include <stdio.h>

int main() {
    const int64_t reads[] = {1, 2, 9, 199, 200, 2048, 2049, 1000000};
    const int64_t lens[] = {1, 63, 64, 65, 2047, 2048, 2049, 11264, 16383, 16384};
    const int bs[] = {1, 25, 60, 253};
    long long cases = 0;
    for (int64_t n_reads : reads)
        for (int64_t max_len : lens)
            for (int B : bs)
                for (int64_t max_slots = 0; max_slots <= 2; ++max_slots) {
                    const wdx::OptimalPlan P = wdx::plan_refine_optimal(n_reads, max_len, B, max_slots);
                    if (P.cap < max_len || P.cap % 64 || P.cap > WDX_MAX_ADAPTER_SAMPLES) return 1;
                    const size_t path = ((size_t)B * (size_t)(P.cap + 1) * 2 + 15) & ~(size_t)15;
                    const size_t rows = P.cap > wdx::kOptLdsCap ? (size_t)4 * (size_t)(P.cap + 1) * 8 : 0;
                    if (P.slot_bytes < path + rows || P.slot_bytes % 256 || P.slot_bytes != wdx::optimal_slot_bytes(P.cap, B)) return 2;
                    if (P.slots < 1 || P.slots > wdx::kOptMaxSlots || P.slots > n_reads) return 3;
                    if (max_slots > 0 && P.slots > max_slots) return 4;
                    if (P.bytes != (size_t)P.slots * P.slot_bytes || P.bytes > wdx::kOptScratchMax) return 5;
                    printf("%lld %lld %d %lld %lld %llu %lld %llu\n", (long long)n_reads, (long long)max_len, B, (long long)max_slots,
                           (long long)P.cap, (unsigned long long)P.slot_bytes, (long long)P.slots, (unsigned long long)P.bytes);
                    ++cases;
                }
    fprintf(stderr, "%lld cases\n", cases);
    return 0;
}
