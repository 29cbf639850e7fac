"""The slot plan of the optimal change-points (warpdemux_amd/csrc/wdx_refine_optimal_plan.h), restated: a grid of `slots`
workgroups strides over the reads of a refining call, each with `slot_bytes` of a scratch buffer of at most 256 MiB.  The
tests that need a workgroup to finish a second read size their batches by it."""
LDS_CAP = 2047            # kOptLdsCap: tails whose prefix sums and value rows live in LDS
SCRATCH_MAX = 256 << 20   # kOptScratchMax
MAX_SLOTS = 2048          # kOptMaxSlots
MAX_TAIL = 16384          # WDX_MAX_ADAPTER_SAMPLES


def tail_cap(max_len):
    """the longest tail a slot holds: max_len rounded up to a multiple of 64 samples, within 64 .. 16 384"""
    return min((max(int(max_len), 64) + 63) // 64 * 64, MAX_TAIL)


def slot_bytes(cap, B):
    """the path table, 16-bit entries, B rows of cap + 1, to a 16-byte boundary; beyond the LDS cap four arrays of cap + 1
    doubles; the whole to a multiple of 256 bytes"""
    b = (B * (cap + 1) * 2 + 15) // 16 * 16
    if cap > LDS_CAP:
        b += 4 * (cap + 1) * 8
    return (b + 255) // 256 * 256


def optimal_plan(n_reads, max_len, B, max_slots=0):
    """-> dict(cap, slot_bytes, slots, bytes)"""
    cap = tail_cap(max_len)
    sb = slot_bytes(cap, max(int(B), 1))
    slots = min(SCRATCH_MAX // sb, MAX_SLOTS)
    if max_slots > 0:
        slots = min(slots, max_slots)
    slots = max(min(slots, int(n_reads)), 1)
    return dict(cap=cap, slot_bytes=sb, slots=slots, bytes=slots * sb)
