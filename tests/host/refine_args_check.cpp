// Stand-alone check of warpdemux_amd/csrc/wdx_refine_args.h (tests/test_refine_args_host.py builds it with the system compiler
// and the address / undefined-behaviour sanitizers).  stdin: the cases as binary records of seven int64,
//   p_null rp_given query_null n_query barcode_keep_events checks barcode_num_events
// stdout: code, K of *pv (-777 when the call was refused: *pv must then be as it was), which message (0 none, 1 "<who>: bad
// arguments", 2 empty query, 3 barcode_num_events must be >= 1) of every case, three int64 each.  An accepted case is also
// held against the rest of the contract: every other field of *p arrives in *pv, and *p is not written.
#include "wdx_refine_args.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

static char g_msg[256];

namespace wdx {
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
}
}  // namespace wdx

#define CHECK(cond)                                                                  \
    if (!(cond)) {                                                                   \
        fprintf(stderr, "case %lld: %s (message \"%s\")\n", n_cases, #cond, g_msg); \
        return 1;                                                                    \
    }

int main() {
    long long in[7], n_cases = 0;
    static_assert(sizeof(long long) == 8, "the cases are int64");
    const double query[3] = {0.5, -0.5, 0.25};
    while (fread(in, 8, 7, stdin) == 7) {
        wdx_seg_params p;
        memset(&p, 0x5a, sizeof(p));   // every field recognisable
        p.barcode_num_events = (int32_t)in[6];
        wdx_refine_params rp;
        memset(&rp, 0, sizeof(rp));
        rp.query = in[2] ? nullptr : query;
        rp.n_query = (int32_t)in[3];
        rp.barcode_keep_events = (int32_t)in[4];
        const wdx_seg_params p0 = p;
        wdx_seg_params pv;
        memset(&pv, 0x33, sizeof(pv));
        const wdx_seg_params pv0 = pv;
        g_msg[0] = 0;
        const int code = wdx::refine_seg_params("who", in[0] ? nullptr : &p, in[1] ? &rp : nullptr, &pv, (unsigned)in[5]);
        const long long which = !g_msg[0] ? 0 : !strcmp(g_msg, "who: bad arguments") ? 1 : !strcmp(g_msg, "consensus refinement: empty query") ? 2
                              : !strcmp(g_msg, "barcode_num_events must be >= 1") ? 3 : -1;
        CHECK(which >= 0);
        CHECK(code == WDX_SUCCESS || code == WDX_ERR_INVALID);
        CHECK((code == WDX_SUCCESS) == (which == 0));
        CHECK(!memcmp(&p, &p0, sizeof(p)));   // (wdx_seg_params has no padding: ten 4-byte fields and a double)
        if (code == WDX_SUCCESS) {
            wdx_seg_params want = p0;
            if (in[1]) want.barcode_num_events = (int32_t)in[4];
            CHECK(!memcmp(&pv, &want, sizeof(pv)));
        } else {
            CHECK(!memcmp(&pv, &pv0, sizeof(pv)));
        }
        const long long res[3] = {code, code == WDX_SUCCESS ? pv.barcode_num_events : -777, which};
        fwrite(res, 8, 3, stdout);
        ++n_cases;
    }
    fprintf(stderr, "%lld cases\n", n_cases);
    return 0;
}
