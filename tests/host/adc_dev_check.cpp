// The slicing arithmetic of the int16 device shards (warpdemux_amd/csrc/wdx_adc_dev.h) and the window the device kernel
// stages for a read, with the system compiler and no GPU: tests/test_adc_dev_host.py builds this under the address and
// undefined-behaviour sanitizers.  stdin: records of nine little-endian int64; stdout: six int64 per record.
//   kind 0 (plan)    n_reads max_len slice_option          -> pitch slice_reads n_slices last_reads staging_bytes budget
//   kind 1 (window)  a_start a_end packed capacity row_len row_win padding max_len  (dead = bit 1 of `packed`)
//                                                          -> first row valid win a_start' a_end'
// The program itself asserts what must hold whatever the expected numbers are: the staging block inside the budget and large
// enough for every slice, the slices covering the reads exactly, the staged row inside its pitch and inside the read, and
// adc_dev_window equal to adapter_window called with the alignment and the cut the header states.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "wdx_adc_dev.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "case %lld: %s\n", (long long)(i), #c);          \
            return 1;                                                         \
        }                                                                     \
    } while (0)

int main() {
    std::vector<int64_t> in;
    int64_t v;
    while (fread(&v, 8, 1, stdin) == 1) in.push_back(v);
    if (in.size() % 9) return 2;
    const int64_t n_cases = (int64_t)in.size() / 9;
    std::vector<int64_t> out((size_t)n_cases * 6);
    for (int64_t i = 0; i < n_cases; ++i) {
        const int64_t *c = &in[(size_t)i * 9];
        int64_t *o = &out[(size_t)i * 6];
        if (c[0] == 0) {
            const int64_t n = c[1], max_len = c[2], opt = c[3];
            const wdx::AdcDevPlan P = wdx::adc_dev_plan(n, max_len, opt);
            CHECK(P.pitch == wdx::adc_dev_pitch(max_len) && P.pitch % 8 == 0 && P.pitch >= max_len + 8);
            CHECK(P.slice_reads >= 1);
            CHECK(P.staging_bytes <= wdx::kAdcDevStagingBudget);
            CHECK(P.slice_reads * wdx::adc_dev_read_bytes(P.pitch) <= wdx::kAdcDevStagingBudget);
            if (n > 0) {
                CHECK(P.n_slices >= 1 && P.last_reads >= 1 && P.last_reads <= P.slice_reads);
                CHECK((P.n_slices - 1) * P.slice_reads + P.last_reads == n);
                CHECK(P.staging_bytes == (n < P.slice_reads ? n : P.slice_reads) * (P.pitch * 4 + 12));
            } else {
                CHECK(P.n_slices == 0 && P.last_reads == 0 && P.staging_bytes == 0);
            }
            if (opt > 0) CHECK(P.slice_reads <= opt);
            o[0] = P.pitch, o[1] = P.slice_reads, o[2] = P.n_slices, o[3] = P.last_reads, o[4] = P.staging_bytes;
            o[5] = wdx::kAdcDevStagingBudget;
        } else {
            const int32_t a_start = (int32_t)c[1], a_end = (int32_t)c[2];
            const bool packed = c[3] & 1, dead = c[3] & 2;
            const int64_t capacity = c[4], row_len = c[5], row_win = c[6], padding = c[7], max_len = c[8];
            const wdx::AdcDevRow R = wdx::adc_dev_row(packed, capacity, row_len, row_win);
            CHECK(R.row_len >= 0 && R.row_len <= (capacity > 0 ? capacity : 0) && R.limit >= 0);
            CHECK(packed ? R.limit >= R.row_len : R.limit == (capacity > 0 ? capacity : 0));
            const wdx::Window w = wdx::adc_dev_window(a_start, a_end, R, dead, padding, max_len);
            const wdx::WindowOpts opts{padding, 8, max_len + 1};
            const wdx::Window ref = wdx::adapter_window(a_start, a_end, R.limit, dead, opts, R.row_len);
            CHECK(w.first == ref.first && w.row == ref.row && w.valid == ref.valid && w.win == ref.win &&
                  w.a_start == ref.a_start && w.a_end == ref.a_end);
            // what the kernel relies on: whole groups of 8 inside the pitch, 16-byte loads inside the read
            CHECK(w.first % 8 == 0 && w.first >= 0 && w.valid >= 0 && w.valid <= w.row);
            CHECK((w.row + 7) / 8 * 8 <= wdx::adc_dev_pitch(max_len));
            CHECK(w.first + w.valid <= R.row_len || w.valid == 0);
            CHECK(w.win <= max_len + 1);
            if (dead) CHECK(w.row == 0 && w.a_start == a_start && w.a_end == a_end);
            o[0] = w.first, o[1] = w.row, o[2] = w.valid, o[3] = w.win, o[4] = w.a_start, o[5] = w.a_end;
        }
    }
    fwrite(out.data(), 8, out.size(), stdout);
    fprintf(stderr, "%lld cases\n", (long long)n_cases);
    return 0;
}
