// Stand-alone check of warpdemux_amd/csrc/wdx_window.h (tests/test_window_host.py builds it with the system compiler and the
// address / undefined-behaviour sanitizers).  stdin: the cases as binary records of eight int64 (a million lines of text
// cost more than the check itself),
//   a_start a_end limit padding align max_win row_len dead        (limit < 0: no row limit; row_len < 0: no valid count)
// stdout: first row valid win a_start' a_end' of every case, six int64 each.  Every case is also held against what the
// comments of the staging loops claim: nothing outside the row is addressed, the start is aligned, and the kernels' own rule
// on the packed row with the shifted bounds selects exactly the samples it selects on the original row.
#include "wdx_window.h"

#include <stdio.h>

#include <algorithm>

#define CHECK(cond)                                                                                          \
    if (!(cond)) {                                                                                           \
        fprintf(stderr, "case %lld (%lld %lld %lld %lld %lld %lld %lld %lld): %s\n", n_cases, as, ae, limit, \
                pad, align, max_win, row_len, dead, #cond);                                                  \
        return 1;                                                                                            \
    }

int main() {
    long long in[8], n_cases = 0;
    static_assert(sizeof(long long) == 8, "the cases are int64");
    while (fread(in, 8, 8, stdin) == 8) {
        const long long as = in[0], ae = in[1], limit = in[2], pad = in[3], align = in[4], max_win = in[5], row_len = in[6], dead = in[7];
        const wdx::WindowOpts o{pad, align, max_win};
        const int64_t lim = limit < 0 ? wdx::kNoRowLimit : limit;
        const wdx::Window w = wdx::adapter_window((int32_t)as, (int32_t)ae, lim, dead != 0, o, row_len);
        const long long res[6] = {w.first, w.row, w.valid, w.win, w.a_start, w.a_end};
        fwrite(res, 8, 6, stdout);
        // nothing outside the row is addressed
        CHECK(w.first >= 0 && w.first <= lim);
        CHECK(w.valid >= 0 && w.first + w.valid <= lim);
        CHECK(w.first % align == 0);
        CHECK(w.valid <= w.row);
        // the kernels' rule (extract_adapter) on the original row ...
        const int64_t start = std::max<int64_t>(as - pad, 0);
        int64_t n = std::max<int64_t>(std::min<int64_t>(ae + pad, lim) - start, 0);
        if (max_win > 0) n = std::min<int64_t>(n, max_win);   // (a capped window keeps its first max_win samples)
        if (dead) n = 0;
        // ... and on the packed row, whose length the kernels are given as `row`
        const int64_t p_start = std::max<int64_t>((int64_t)w.a_start - pad, 0);
        const int64_t p_n = std::max<int64_t>(std::min<int64_t>((int64_t)w.a_end + pad, w.row) - p_start, 0);
        CHECK(p_n == n && w.win == n);
        CHECK(n == 0 || w.first + p_start == start);
        if (n == 0) CHECK(w.row == 0 && w.valid == 0);
        // a packed sample is copied exactly when it is one of the read's own (the rest is the NaN tail)
        for (int64_t j = 0; j < w.row; ++j) CHECK((j < w.valid) == (row_len < 0 || w.first + j < row_len));
        ++n_cases;
    }
    // the accumulators, on a sequence small enough to state by hand
    wdx::WindowBatch wb(16);
    wdx::PackedOffset pos(4);
    const wdx::WindowOpts o{1, 4, 0};
    const wdx::Window a = wdx::adapter_window(6, 9, 16, false, o), b = wdx::adapter_window(2, 3, 16, false, o),
                      c = wdx::adapter_window(20, 30, 16, false, o), d = wdx::adapter_window(0, 16, 16, true, o);
    for (const wdx::Window &w : {a, b, c, d}) wb.add(w);
    const bool acc_ok = wb.max_len == 5 && wb.col0 == 0 && wb.col1 == 10 && wb.win_total == 6 + 4 && pos.take(a.row) == 0 &&
                        pos.take(b.row) == 8 && pos.take(c.row) == 12 && pos.take(d.row) == 12 && pos.next == 12;
    if (!acc_ok) {
        fprintf(stderr, "accumulators: max_len %lld cols [%lld, %lld) total %lld next %lld\n", (long long)wb.max_len,
                (long long)wb.col0, (long long)wb.col1, (long long)wb.win_total, (long long)pos.next);
        return 1;
    }
    fprintf(stderr, "%lld cases\n", n_cases);
    return 0;
}
