// Stand-alone driver of warpdemux_amd/csrc/wdx_fp_plan.h -- which kernels a fingerprint call launches, in which order, over
// which grids -- built by tests/test_fp_plan_host.py with the system compiler and the address / undefined-behaviour sanitizers.
//   fp_plan_check <profiles/r08a_launch_sequence.txt>
// REPLAY.  Every section of the recorded route table is rebuilt as a call (configuration x reads x the one option, or
// wdx_fingerprint_profile_dev's fast_path / stop_phase), planned, expanded through fp_slices, and compared launch by launch:
// kernel with its template arguments, grid in work-items, workgroup size.  The two refinement wave kernels are compared by
// position and name only (their grids belong to wdx_refine_*.hip; the tail step is taken as the wave form, which is what the
// recorded triple runs); the trace's static-LDS column is a property of the kernel, not a decision, and is not read.  Prints
// "<sections> sections <launches> launches".
// Where a section's name leaves a parameter open, the value taken is (CONFIGS below):
//   longest window 8192 where the name has no maxNNNN; barcode_num_events 25 everywhere; the caller gave the buffer of
//   fingerprint_big_bytes (the recorded 12288- and 16384-sample sections end in fingerprint_big_kernel) and none for the long form
//   W6                     E 110, d 3        W10_exact_only_even   E 110, d 5       W13_exact_only_odd_max12288   E 110, d 6
//   W40_no_fast_kernel     E 110, d 6        sig_norm_mean         E 110, d 6, W 12, WDX_NORM_MEAN
//   refine_E120_d9_W18     a query of 40 points, barcode_num_events[0] = 25, hand-over records given
//   profile_dev            E 110, d 6, W 12; fast_path 0: no workspace; fast_path 2: stop_phase -2 (as wdx_api.hip passes it)
// SWEEP.  running_stat_width 0 .. kMaxW x min_obs_per_base 0 .. 20 x the three normalisations x num_events {1, 25, 110, 126,
// 127, kMaxEvents} x max_len at and either side of every capacity boundary x n_reads {1, 1023, 1024, 2047, 2048, 40 000,
// 2^21 +- 1, 10^7, 2^31 - 1} x (no switch, every switch alone) x every PlanFlags combination an entry point produces: the
// product's every 1801st point (a prime that divides no dimension: every value of every dimension is met), about 10^6 plans.
// Checked of each: check() below, the exit status names the invariant.  Then every refusal once, code and message.  Prints,
// not asserts, the workgroups per CU of every distinct (family, capF, capP, nbt) by the 1 280-byte LDS granule rule.
#include "wdx_fp_plan.h"

#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <tuple>
#include <vector>

using namespace wdx;

static const char *tf(bool b) { return b ? "true" : "false"; }
static std::string kernel_name(const FpKernelKey &k) {
    char b[160];
    switch (k.family) {
        case kFamFastMain: snprintf(b, sizeof b, "wdx::fingerprint_fast_kernel<%d, %s, %d, %d, %s, %s>", k.npt, tf(k.prof), k.fw, k.nbt, tf(k.ext), tf(k.split)); break;
        case kFamList1: snprintf(b, sizeof b, "wdx::fingerprint_fast_list1_kernel<%d, %d, %d, %s>", k.npt, k.fw, k.nbt, tf(k.split)); break;
        case kFamListStride: snprintf(b, sizeof b, "wdx::fingerprint_fast_list_kernel<%d, %d, %d>", k.npt, k.fw, k.nbt); break;
        case kFamStream: snprintf(b, sizeof b, "wdx::fingerprint_fast_stream_kernel<%d, %d>", k.fw, k.nbt); break;
        case kFamSplitTail: snprintf(b, sizeof b, "wdx::fingerprint_split_tail_kernel<%d, %d>", k.fw, k.nbt); break;
        case kFamClip: snprintf(b, sizeof b, "wdx::clip_bounds_kernel<%d>", k.npl); break;
        case kFamClipList: snprintf(b, sizeof b, "wdx::clip_bounds_list_kernel<%d>", k.npl); break;
        case kFamClipBlock: snprintf(b, sizeof b, "wdx::clip_bounds_block_kernel"); break;
        case kFamRoute: snprintf(b, sizeof b, "wdx::route_long_windows_kernel"); break;
        case kFamExactChunks: snprintf(b, sizeof b, "wdx::fingerprint_kernel<%d, %s>", k.block, tf(k.prof)); break;
        case kFamExactList: snprintf(b, sizeof b, "wdx::fingerprint_list_kernel<%d>", k.block); break;
        case kFamBig: snprintf(b, sizeof b, "wdx::fingerprint_big_kernel<%d>", k.block); break;
        case kFamLong: snprintf(b, sizeof b, "wdx::fingerprint_long_kernel<%d>", k.block); break;
        default: snprintf(b, sizeof b, "?"); break;
    }
    return b;
}
static const char *const kMatchWave = "wdx::(anonymous namespace)::fingerprint_refine_match_wave_kernel";
static const char *const kTailWave = "wdx::(anonymous namespace)::fingerprint_refine_tail_wave_kernel";

struct Launch {
    std::string name;
    long long grid, wg;   // grid in work-items; -1: compared by name only
};
// the launches of a plan, in order
static std::vector<Launch> expand(const FpPlan &pl, int64_t max_launch_slice) {
    std::vector<Launch> out;
    for (int i = 0; i < pl.n_steps; ++i) {
        const FpStep &s = pl.steps[i];
        const FpSlices S = fp_slices(s.extent, s.rule, s.slice_limit, max_launch_slice);
        const FpStep *tail = s.split_tile ? &pl.steps[i + 1] : nullptr;
        for (int64_t j = 0; j < S.count; ++j) {
            if (s.key.family == kFamRefineTail || s.key.family == kFamRefineOptimal) {
                out.push_back({kMatchWave, -1, -1});
                if (s.key.family == kFamRefineTail) out.push_back({kTailWave, -1, -1});
                continue;
            }
            out.push_back({kernel_name(s.key), (long long)(S.n(j) * s.wg), s.wg});
            if (tail) out.push_back({kernel_name(tail->key), (long long)((S.n(j) + tail->per_wg - 1) / tail->per_wg * tail->wg), tail->wg});
        }
        if (s.key.family == kFamRefineOptimal) out.push_back({"wdx::fingerprint_refine_optimal_kernel", -1, -1});
        if (tail) ++i;
    }
    return out;
}

// ---- replay -----------------------------------------------------------------------------------------------------------
struct Config {
    const char *name;
    int E, d, W, max_len, norm;
    bool refine;
};
static const Config CONFIGS[15] = {
    {"E110_d6_W12_max4096", 110, 6, 12, 4096, WDX_NORM_NONE, false},   {"E110_d6_W12_max5120", 110, 6, 12, 5120, WDX_NORM_NONE, false},
    {"E110_d6_W12_max6144", 110, 6, 12, 6144, WDX_NORM_NONE, false},   {"E110_d6_W12_max8192", 110, 6, 12, 8192, WDX_NORM_NONE, false},
    {"E110_d6_W12_max12288", 110, 6, 12, 12288, WDX_NORM_NONE, false}, {"E110_d6_W12_max16384", 110, 6, 12, 16384, WDX_NORM_NONE, false},
    {"E120_d9_W18", 120, 9, 18, 8192, WDX_NORM_NONE, false},           {"E110_d15_W30", 110, 15, 30, 8192, WDX_NORM_NONE, false},
    {"W6", 110, 3, 6, 8192, WDX_NORM_NONE, false},                     {"E110_d12_W12_combo7", 110, 12, 12, 8192, WDX_NORM_NONE, false},
    {"W10_exact_only_even", 110, 5, 10, 8192, WDX_NORM_NONE, false},   {"W13_exact_only_odd_max12288", 110, 6, 13, 12288, WDX_NORM_NONE, false},
    {"W40_no_fast_kernel", 110, 6, 40, 8192, WDX_NORM_NONE, false},    {"sig_norm_mean", 110, 6, 12, 8192, WDX_NORM_MEAN, false},
    {"refine_E120_d9_W18", 120, 9, 18, 8192, WDX_NORM_NONE, true},
};
static wdx_seg_params seg_params(int E, int d, int W, int norm) {
    wdx_seg_params p;
    memset(&p, 0, sizeof p);
    p.num_events = E, p.min_obs_per_base = d, p.running_stat_width = W, p.sig_norm = norm, p.barcode_num_events = 25;
    return p;
}
static bool set_option(FpSwitches &sw, const std::string &opt) {
    if (opt.empty()) return true;
    if (opt == "NO_SPLIT_TAIL") sw.no_split = true;
    else if (opt == "FAST_EXACT_SCORES") sw.fast_exact_scores = true;
    else if (opt == "NO_PEAK_FILTER") sw.no_peak_filter = true;
    else if (opt == "EXACT_PATH") sw.exact_path = true;
    else if (opt == "NO_CLIP_REUSE") sw.no_clip_reuse = true;
    else if (opt == "NO_WAVE_CLIP_LONG") sw.no_wave_clip_long = true;
    else if (opt.rfind("FAST_MAIN_CAP=", 0) == 0) sw.fast_main_cap = atoi(opt.c_str() + 14);
    else if (opt.rfind("MAX_LAUNCH_SLICE=", 0) == 0) sw.max_launch_slice = atoll(opt.c_str() + 17);
    else return false;
    return true;
}
// "== <configuration> n=<N> [OPTION]" or "== profile_dev fast_path=F stop_phase=S n=<N>" -> the launches the plan makes of it
static bool plan_section(const std::string &head, std::vector<Launch> &out) {
    std::vector<std::string> w;
    for (size_t a = 0; a < head.size();) {
        const size_t b = head.find(' ', a);
        w.push_back(head.substr(a, b == std::string::npos ? b : b - a));
        a = b == std::string::npos ? head.size() : b + 1;
    }
    if (w.size() < 2) return false;
    FpSwitches sw;
    PlanFlags f{true, false, 0, true, false, false, false};
    wdx_seg_params p;
    int64_t n = 0, max_len = 8192;
    if (w[0] == "profile_dev") {
        if (w.size() != 4 || w[1].rfind("fast_path=", 0) || w[2].rfind("stop_phase=", 0) || w[3].rfind("n=", 0)) return false;
        const int fast_path = atoi(w[1].c_str() + 10), stop_phase = atoi(w[2].c_str() + 11);
        n = atoll(w[3].c_str() + 2);
        p = seg_params(110, 6, 12, WDX_NORM_NONE);
        f = PlanFlags{fast_path != 0, true, fast_path == 2 ? -2 : stop_phase, false, false, false, false};
    } else {
        const Config *c = nullptr;
        for (const Config &k : CONFIGS)
            if (w[0] == k.name) c = &k;
        if (!c || w[1].rfind("n=", 0) || w.size() > 3) return false;
        n = atoll(w[1].c_str() + 2);
        if (!set_option(sw, w.size() == 3 ? w[2] : std::string())) return false;
        p = seg_params(c->E, c->d, c->W, c->norm);
        max_len = c->max_len;
        f.refine = f.refine_ws = c->refine;
    }
    const FpRefineView view{true, 40, 25, 0, 0};
    if (check_fingerprint_call(n, p, f.refine ? &view : nullptr, f, sw).code) return false;
    const FpPlan pl = plan_fingerprint(p, max_len, n, sw, f);
    if (pl.refused.code) return false;
    out = expand(pl, sw.max_launch_slice);
    return true;
}
static int replay(const char *path) {
    FILE *fp = fopen(path, "r");
    if (!fp) {
        fprintf(stderr, "cannot open %s\n", path);
        return 100;
    }
    char line[512];
    std::vector<Launch> want;
    std::string head;
    size_t at = 0;
    long long sections = 0, launches = 0;
    int bad = 0;
    auto close_section = [&]() {
        if (!head.empty() && !bad && at != want.size()) {
            fprintf(stderr, "section '%s': the trace has %zu launches, the plan %zu\n", head.c_str(), at, want.size());
            bad = 101;
        }
    };
    while (!bad && fgets(line, sizeof line, fp)) {
        std::string s(line);
        while (!s.empty() && (s.back() == '\n' || s.back() == '\r' || s.back() == ' ')) s.pop_back();
        if (s.empty() || s[0] == '#') continue;
        if (s.rfind("== ", 0) == 0) {
            close_section();
            head = s.substr(3), at = 0, ++sections;
            if (!bad && !plan_section(head, want)) {
                fprintf(stderr, "section '%s': not a call this program can rebuild\n", head.c_str());
                bad = 102;
            }
            continue;
        }
        // "<kernel>   grid G   wg W   lds L"
        const size_t g = s.find(" grid ");
        long long grid = 0, wg = 0;
        if (head.empty() || g == std::string::npos || sscanf(s.c_str() + g, " grid %lld wg %lld", &grid, &wg) != 2) {
            fprintf(stderr, "unreadable line: %s\n", s.c_str());
            bad = 103;
            break;
        }
        std::string name = s.substr(0, g);
        while (!name.empty() && name.back() == ' ') name.pop_back();
        ++launches;
        if (at >= want.size() || want[at].name != name || (want[at].grid >= 0 && (want[at].grid != grid || want[at].wg != wg))) {
            fprintf(stderr, "section '%s', launch %zu: the trace has %s grid %lld wg %lld, the plan %s grid %lld wg %lld\n", head.c_str(), at,
                    name.c_str(), grid, wg, at < want.size() ? want[at].name.c_str() : "(nothing)", at < want.size() ? want[at].grid : 0,
                    at < want.size() ? want[at].wg : 0);
            bad = 104;
        }
        ++at;
    }
    close_section();
    fclose(fp);
    printf("%lld sections %lld launches\n", sections, launches);
    return bad;
}

// ---- sweep ------------------------------------------------------------------------------------------------------------
struct Case {
    wdx_seg_params p;
    int64_t max_len, n_reads;
    FpSwitches sw;
    PlanFlags f;
};
static bool is_fast(FpFamily f) { return f == kFamFastMain || f == kFamList1 || f == kFamListStride || f == kFamStream || f == kFamSplitTail; }
static std::set<std::tuple<int, int, int, int, size_t>> g_shapes;   // (family, capF, capP, nbt, lds) of the steps with dynamic LDS

// what must hold of every plan; 0 or the number of the invariant that does not
static int check(const Case &c, const FpPlan &pl) {
    if (pl.refused.code) return 1;   // (the sweep's calls are inside the accepted domain: nothing reaches the plan's two refusals)
    if (pl.n_steps < 1 || pl.n_steps >= kFpMaxSteps) return 2;
    const bool ablation = c.f.prof && c.f.stop_phase > 0 && pl.path == FpPlan::kChain;
    int last_fast = -1, slow_at = -1, stride_on_big1 = 0, retry_on_big1 = 0;
    for (int i = 0; i < pl.n_steps; ++i) {
        const FpStep &s = pl.steps[i];
        if (!fp_key_exists(s.key)) return 3;
        if (s.lds > kLdsMax) return 4;
        if (s.wg < 64 || s.wg > 1024 || s.wg % 64 || s.extent < 1 || s.per_wg < 1) return 5;
        const FpSlices S = fp_slices(s.extent, s.rule, s.slice_limit, c.sw.max_launch_slice);
        // (slice j is base(j) = j * slice .. of n(j) <= slice workgroups: the first is the largest, the last ends at the extent)
        if (S.count < 1 || S.slice < 1 || S.n(0) * s.wg >= (1ll << 32) || S.n(0) != (S.count == 1 ? s.extent : S.slice)) return 6;
        if (S.n(S.count - 1) < 1 || S.base(S.count - 1) + S.n(S.count - 1) != s.extent) return 7;
        if (is_fast(s.key.family)) {
            last_fast = i;
            // peak lists: the ownership rounds' reach; the non-EXT striding kernel's in-kernel medians put their histogram of
            // kHB + 64 words where the peak list will be (score 8 + position 2 + state 1 bytes per entry)
            if (s.capP < 1 || s.capP > (s.key.family == kFamStream ? kCapPMaxStream : kCapPMax)) return 8;
            if (s.key.family == kFamListStride && (size_t)(s.capP + 8 * s.key.nbt) * 11 < (size_t)(kHB + 64) * 4) return 9;
            if (s.key.family != kFamSplitTail) {
                const size_t lds = s.key.family == kFamStream ? fast_stream_lds_bytes(s.capP, s.key.nbt) : fast_lds_bytes(s.capF, s.capP, s.key.nbt);
                if (s.lds != lds || (s.key.family != kFamStream && s.capF != s.key.npt * kFastBlock)) return 10;
            }
        }
        if (s.lds) g_shapes.insert({(int)s.key.family, s.capF, s.capP, s.key.nbt, s.lds});
        // a tile is followed by its tail over the same slices
        if (s.split_tile) {
            if (i + 1 >= pl.n_steps) return 11;
            const FpStep &t = pl.steps[i + 1];
            if (t.key.family != kFamSplitTail || t.key.fw != s.key.fw || t.key.nbt != s.key.nbt || !s.key.split) return 12;
            if (t.rule != s.rule || t.slice_limit != s.slice_limit || t.extent != (s.extent + t.per_wg - 1) / t.per_wg) return 13;
            if (t.in != s.in || t.over != s.over || t.retry != s.retry || t.capP != s.capP || t.clip != s.clip) return 14;
            if (s.rule != kFullSlices || fp_slice_limit(s.slice_limit, c.sw.max_launch_slice) > kSplitSlice) return 15;   // (the slice's lists fit the workspace)
        } else if (s.key.family == kFamSplitTail && (i == 0 || !pl.steps[i - 1].split_tile)) {
            return 16;
        }
        if (s.key.split && !s.split_tile) return 17;
        // lists: what a step hands over to or retries on is taken by a later step, and was not taken before
        for (int l : {s.over, s.retry}) {
            if (l == kNoList) continue;
            if (l < kCntSlow || l > kCntBack) return 18;
            bool later = false;
            for (int j = 0; j < pl.n_steps; ++j) {
                if (pl.steps[j].in != l || j == i || (s.split_tile && j == i + 1) || (j + 1 == i && pl.steps[j].split_tile)) continue;
                if (j < i) return 19;
                later = true;
            }
            if (!later && !ablation) return 20;
        }
        if (s.in == kCntBig1 && s.key.family == kFamListStride) ++stride_on_big1;
        if (s.retry == kCntBig1) ++retry_on_big1;
        if (s.in == kCntSlow && s.key.family == kFamExactList && slow_at < 0) slow_at = i;
        if (s.key.family == kFamExactList || s.key.family == kFamBig || s.key.family == kFamLong || s.key.family == kFamExactChunks) {
            if (s.wg != s.key.block) return 21;
        }
    }
    // (big1 is the 8192-sample list, or -- the documented reuse -- the streaming kernel's retry list: never both)
    if (stride_on_big1 && retry_on_big1) return 22;
    if (pl.path == FpPlan::kChain) {
        // the slow list is taken by the exact kernel behind every fast kernel
        if (ablation ? slow_at >= 0 : (slow_at < 0 || slow_at < last_fast)) return 23;
        if (last_fast < 0) return 24;
    } else {
        if (last_fast >= 0 || slow_at >= 0) return 25;
        int chunks = 0;
        for (int i = 0; i < pl.n_steps; ++i) chunks += pl.steps[i].key.family == kFamExactChunks;
        if (chunks != 1) return 26;
    }
    if (pl.with_long && !pl.with_huge) return 27;
    return 0;
}

static int sweep() {
    static const int EV[] = {1, 25, 110, 126, 127, kMaxEvents};
    static const int NORM[] = {WDX_NORM_NONE, WDX_NORM_MEAN, WDX_NORM_MEDIAN};
    static const int64_t BOUND[] = {64, 512, 4096, 5120, 6144, 8192, 11200, 12288, 13312, 16384, 65536};
    static const int64_t NREADS[] = {1, 1023, 1024, 2047, 2048, 40000, (1ll << 21) - 1, (1ll << 21) + 1, 10000000, 0x7fffffffLL};
    // no switch, and every switch alone
    std::vector<FpSwitches> SW(16);
    SW[1].exact_path = true, SW[2].fast_peak_cap = 640, SW[3].fast_main_cap = 5120, SW[4].fast_main_cap = 6144, SW[5].fast_chain_min = 1024;
    SW[6].fast_chain_min = 1 << 22, SW[7].fast_exact_scores = true, SW[8].no_clip_reuse = true, SW[9].no_wave_clip_long = true;
    SW[10].no_peak_filter = true, SW[11].no_split = true, SW[12].max_launch_slice = 7000, SW[13].long_windows = true;
    SW[14].long_refine_windows = true, SW[15].refine_optimal = true;
    // the entry points: a plain or refining call with a workspace (with / without the buffers of the big and long forms, with /
    // without the hand-over records), and wdx_fingerprint_profile_dev's fast_path 0 / 1 / 2 x stop_phase 0 / 1
    std::vector<PlanFlags> FL;
    for (int refine = 0; refine < 3; ++refine)
        for (int buf = 0; buf < 3; ++buf) FL.push_back(PlanFlags{true, false, 0, buf >= 1, buf == 2, refine > 0, refine == 2});
    for (int sp = 0; sp < 2; ++sp) FL.push_back(PlanFlags{false, true, sp, false, false, false, false});
    for (int sp = 0; sp < 2; ++sp) FL.push_back(PlanFlags{true, true, sp, false, false, false, false});
    FL.push_back(PlanFlags{true, true, -2, false, false, false, false});
    const int64_t dims[8] = {kMaxW + 1, 21, 3, 6, 33, 10, (int64_t)SW.size(), (int64_t)FL.size()};
    int64_t total = 1;
    for (int64_t d : dims) {
        if (d % 1801 == 0) return 40;
        total *= d;
    }
    long long points = 0, by_path[3] = {0, 0, 0};
    const FpRefineView view{true, 40, 25, 0, 0};
    for (int64_t at = 0; at < total; at += 1801) {
        int64_t ix[8], r = at;
        for (int k = 0; k < 8; ++k) ix[k] = r % dims[k], r /= dims[k];
        Case c;
        c.p = seg_params(EV[ix[3]], (int)ix[1], (int)ix[0], NORM[ix[2]]);
        c.max_len = BOUND[ix[4] / 3] + ix[4] % 3 - 1;
        c.n_reads = NREADS[ix[5]];
        c.sw = SW[ix[6]];
        c.f = FL[ix[7]];
        if (c.p.barcode_num_events > c.p.num_events + 1) c.p.barcode_num_events = 1;
        const FpCheck ok = check_fingerprint_call(c.n_reads, c.p, c.f.refine ? &view : nullptr, c.f, c.sw);
        if (ok.code) {   // (inside the accepted domain only the refining calls' own limits refuse)
            if (ok.why < kFpRefineQuery || ok.why > kFpOptimalNorm) return 41;
            continue;
        }
        const FpPlan pl = plan_fingerprint(c.p, c.max_len, c.n_reads, c.sw, c.f);
        if (const int rc = check(c, pl)) {
            fprintf(stderr, "invariant %d: W %d d %d norm %d E %d max_len %lld n %lld switch %lld flags %lld\n", rc, c.p.running_stat_width,
                    c.p.min_obs_per_base, c.p.sig_norm, c.p.num_events, (long long)c.max_len, (long long)c.n_reads, (long long)ix[6], (long long)ix[7]);
            return rc;
        }
        ++points, ++by_path[pl.path];
    }
    printf("%lld points: %lld chain, %lld exact, %lld diagnostic exact\n", points, by_path[FpPlan::kChain], by_path[FpPlan::kExact],
           by_path[FpPlan::kProfExact]);
    return 0;
}

// ---- refusals: each once, code and message ------------------------------------------------------------------------------
static int refusals() {
    bool seen[kFpRefusals] = {};
    int n = 0, bad = 0;
    auto expect = [&](const FpCheck &r, FpRefusal why, int code, const char *msg) {
        if (r.why != why || r.code != code || strcmp(r.msg, msg) || seen[why]) {
            fprintf(stderr, "refusal %d: got %d / %d / '%s'\n", (int)why, (int)r.why, r.code, r.msg);
            bad = 60 + (int)why;
        }
        seen[why] = true, ++n;
    };
    const PlanFlags plain{true, false, 0, true, false, false, false}, refine{true, false, 0, true, false, true, true};
    const FpSwitches none;
    FpSwitches optimal, optimal_long;
    optimal.refine_optimal = optimal_long.refine_optimal = optimal_long.long_refine_windows = true;
    const FpRefineView view{true, 40, 25, 0, 0};
    auto call = [&](int64_t n_reads, wdx_seg_params p, const FpRefineView *rf, PlanFlags f, const FpSwitches &sw) {
        return check_fingerprint_call(n_reads, p, rf, f, sw);
    };
    wdx_seg_params p = seg_params(110, 6, 12, WDX_NORM_NONE), q;
    if (call(0x7fffffffLL, p, nullptr, plain, none).code || call(1, p, &view, refine, optimal).code) return 59;
    expect(call(0x80000000LL, p, nullptr, plain, none), kFpTooManyReads, WDX_ERR_INVALID, "at most 2^31-1 reads per call");
    q = p, q.num_events = kMaxEvents + 1;
    expect(call(1, q, nullptr, plain, none), kFpNumEvents, WDX_ERR_UNSUPPORTED, "num_events must be in [1, 253]");
    q = p, q.num_events = 0;
    if (call(1, q, nullptr, plain, none).code != WDX_ERR_INVALID) bad = 58;   // (the same refusal, below the range: another code)
    q = p, q.barcode_num_events = kSegCap + 1;
    expect(call(1, q, nullptr, plain, none), kFpBarcodeEvents, WDX_ERR_INVALID, "barcode_num_events must be in [1, 254]");
    q = p, q.running_stat_width = kMaxW + 1;
    expect(call(1, q, nullptr, plain, none), kFpWidth, WDX_ERR_UNSUPPORTED, "running_stat_width must be in [0, 64]");
    q = p, q.padding = -1;
    expect(call(1, q, nullptr, plain, none), kFpPadding, WDX_ERR_INVALID, "padding must be >= 0");
    FpRefineView v = view;
    v.nq = kRefineMaxQuery + 1;
    expect(call(1, p, &v, refine, none), kFpRefineQuery, WDX_ERR_UNSUPPORTED,
           "consensus refinement: the query must have 1..96 points and num_events + 1 <= 128");
    v = view, v.E2 = 0;
    expect(call(1, p, &v, refine, none), kFpRefineEvents, WDX_ERR_INVALID, "consensus refinement: barcode_num_events[0] must be in [1, 253], psi >= 0");
    expect(call(1, p, &view, refine, optimal_long), kFpOptimalWithLong, WDX_ERR_UNSUPPORTED,
           "WDX_OPT_REFINE_OPTIMAL_CPTS and WDX_OPT_LONG_REFINE_WINDOWS do not go together");
    q = p, q.min_obs_per_base = 0;
    expect(call(1, q, &view, refine, optimal), kFpOptimalMinObs, WDX_ERR_UNSUPPORTED, "optimal change-points: min_obs_per_base must be >= 1");
    q = p, q.sig_norm = WDX_NORM_MEAN;
    expect(call(1, q, &view, refine, optimal), kFpOptimalNorm, WDX_ERR_UNSUPPORTED, "optimal change-points: sig_extract.normalization must be \"none\"");
    // the plan's own two: no call inside the accepted domain reaches them (the sweep says so), so they are made directly --
    // the carve-up of a 16 384-sample window, a main kernel of a width that has none
    char want[160];
    snprintf(want, sizeof want, "fingerprint LDS carve-up (%zu B) exceeds 160 KiB", fp_lds_bytes(16384));
    expect(check_fp_lds(fp_lds_bytes(16384)), kFpLds, WDX_ERR_INVALID, want);
    if (check_fp_lds(fp_lds_bytes(kExactLdsCap)).code) bad = 57;
    FpKernelKey k;
    k.family = kFamFastMain, k.npt = kNptLarge, k.fw = 40, k.nbt = 2;
    expect(check_fp_main_kernel(k), kFpNoFastKernels, WDX_ERR_INVALID, "no fast kernels for running_stat_width 40");
    // ... and a plan that outgrows its fixed array of steps is refused, not truncated
    FpPlan over;
    for (int i = 0; i <= kFpMaxSteps; ++i) {
        if (over.refused.code && i <= kFpMaxSteps - 1) bad = 55;
        over.add(kFamRoute);
    }
    if (over.n_steps != kFpMaxSteps) bad = 54;
    snprintf(want, sizeof want, "fingerprint plan: more than %d steps", kFpMaxSteps);
    expect(over.refused, kFpTooManySteps, WDX_ERR_INVALID, want);
    for (int w = 1; w < kFpRefusals; ++w)
        if (!seen[w]) bad = 56;
    printf("%d refusals\n", n);
    return bad;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: fp_plan_check <launch sequence file>\n");
        return 99;
    }
    if (int rc = replay(argv[1])) return rc;
    if (int rc = sweep()) return rc;
    if (int rc = refusals()) return rc;
    // An observation, not a check: LDS is allocated in granules of 1 280 bytes, 128 per CU -- workgroups per CU by that rule
    static const char *const FAM[] = {"main", "list1", "striding", "stream", "split_tail", "clip", "clip_list", "clip_block", "route", "exact",
                                      "exact_list", "big", "long"};
    for (const auto &t : g_shapes) {
        const size_t lds = std::get<4>(t), granules = (lds + 1279) / 1280;
        printf("granules %-10s capF %5d capP %4d nbt %d  lds %6zu B = %3zu granules -> %zu workgroups per CU\n", FAM[std::get<0>(t)],
               std::get<1>(t), std::get<2>(t), std::get<3>(t), lds, granules, 128 / granules);
    }
    return 0;
}
