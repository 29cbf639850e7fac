// Leave-one-out nearest neighbours of a labelled set for gfx950 (include/wdx.h: wdx_self_nearest_device states the rule;
// wdx_loo_plan.h what a call does with its sizes).
//
// Tile route: the self matrix's tile walk (wdx_dtw_self.hip) with the rule's reduction in the place of the two
// images.  The rows are gathered in their own order (wdx_dtw_tile.h: tile_gather_kernel<true>), loo_init_kernel adds the labels
// to the member flags and sets every key to "no candidate"; one WAVE takes one 64 x 64 tile (I, J), J >= I.  Lane a owns row
// 64 I + a.  Each half of 32 columns goes through the hand[column * 65 + row] block in LDS, where lane a walks row a over the
// columns (the row side) and lane c walks column c over the rows of chunk I (the column side: the rows of chunk J).  Both sides
// are merged into the (rows_padded, 2) keys with a 64-bit atomic minimum: a key is (float32 bits << 32) | candidate row, so the
// minimum over the tiles is the rule's choice whatever order they finish in.  A diagonal tile takes each pair from lane
// min(a, b) and skips a == b.  loo_finish_kernel unpacks the keys.
// General route: blocks of padded rows through dtw_plan / run_dtw_plan into a float32 block, then loo_rows_kernel: one wave per
// row applies the rule to its row of the block and writes nn / best itself.
#include "wdx_ctx.h"
#include "wdx_dtw_tile.h"
#include "wdx_loo_plan.h"

#include <math.h>

namespace wdx {

typedef unsigned long long LooKey;

__device__ __forceinline__ LooKey loo_key_of(const float f, const int64_t row) {
    return ((LooKey)__float_as_uint(f) << 32) | (LooKey)(uint32_t)row;
}
// candidate (f, row) of label `lab` into the running keys of a row of label `mine`
__device__ __forceinline__ void loo_take(LooKey &own, LooKey &other, const float f, const int64_t row, const int32_t lab, const int32_t mine) {
    const LooKey k = loo_key_of(f, row);
    if (lab == mine) own = k < own ? k : own;
    else other = k < other ? k : other;
}
__device__ __forceinline__ void loo_merge(LooKey *__restrict__ keys, const int64_t row, const LooKey own, const LooKey other) {
    if (own != kLooNoKey) atomicMin(keys + 2 * row, own);
    if (other != kLooNoKey) atomicMin(keys + 2 * row + 1, other);
}

// ---- behind the gather: labels into the member flags, every key "no candidate" ------------------------------------------------
// label[p]: the label of padded row p when it is a member (its flag from the gather and a label >= 0), else -1
__global__ __launch_bounds__(256) void loo_init_kernel(const int32_t *__restrict__ d_label, int64_t n, int64_t rows,
                                                       uint8_t *__restrict__ member, int32_t *__restrict__ label, LooKey *__restrict__ keys) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= rows) return;
    const int32_t lab = p < n ? (d_label ? d_label[p] : 0) : -1;
    const bool mem = member[p] != 0 && lab >= 0;
    member[p] = mem ? 1 : 0;
    label[p] = mem ? lab : -1;
    keys[2 * p] = kLooNoKey, keys[2 * p + 1] = kLooNoKey;
}

struct LooTileArgs {
    const double *dense;     // (rows_padded, L): a lane's own row
    const double *padded;    // (rows_padded, Lpad): the uniform operand, series at +halo
    int64_t Lpad;
    int halo;
    const int32_t *label;    // [rows_padded]: -1 for a non-member
    int64_t chunks;
    LooKey *keys;            // (rows_padded, 2)
    int L, w;
    double p2;
    int unfused;             // Knobs::dtw_unfused
};

// SHORT: the unrolled 25-point / window-15 shape (W, EXACT_W ignored); DIAG: tile (I, I), the whole 64 x 64 hand-over in LDS.
// (held to the three waves per SIMD the band kernels run at, like self_tile_kernel)
template <int W, bool EXACT_W, bool SHORT, bool DIAG>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((SHORT || W == 15) ? 3 : 0))) void loo_tile_kernel(
    const LooTileArgs G) {
    constexpr int COLS = DIAG ? 64 : 32;
    constexpr int LS = 25, WS = 15;
    __shared__ float hand[COLS * 65];   // hand[column * 65 + row]
    __shared__ int32_t rlab[64];        // label of row 64 I + r (-1: no member)
    __shared__ int32_t clab[64];        // label of row 64 J + c
    const int lane = threadIdx.x;
    int32_t I, J;
    if (DIAG) I = J = (int32_t)blockIdx.x;
    else medoid_upper_tile(G.chunks, (int64_t)blockIdx.x, &I, &J);
    I = __builtin_amdgcn_readfirstlane(I), J = __builtin_amdgcn_readfirstlane(J);
    const int64_t rowI = kMedoidChunk * (int64_t)I, rowJ = kMedoidChunk * (int64_t)J;
    const int32_t mine = G.label[rowI + lane];
    const bool rowmem = mine >= 0;
    const unsigned long long rowmask = __ballot(rowmem);
    rlab[lane] = mine;
    if (!DIAG) clab[lane] = G.label[rowJ + lane];
    const int L = SHORT ? LS : G.L;
    const double *__restrict__ xp = G.dense + (rowI + lane) * (int64_t)L;
    const double delta = dtw_delta(L);
    double xs[SHORT ? LS : 1];
    if (SHORT) {
#pragma unroll
        for (int i = 0; i < LS; ++i) xs[i] = xp[i];
    }
    // f(row of this lane, padded row `col`): the float32 distance (anything when `use` is false)
    auto pair = [&](const int64_t col, const bool use) -> float {
        if constexpr (SHORT) {
            const double *__restrict__ y = G.padded + col * G.Lpad + G.halo;
            return (float)dtw_short_pair<LS, WS>(xs, y, G.p2, !use, delta, G.unfused);
        } else {
            const double *__restrict__ y = G.padded + col * G.Lpad + (G.halo - (W - 1));
            return medoid_band_pair<W, EXACT_W>(xp, y, L, G.w, G.p2, use, delta, G.unfused);
        }
    };
    medoid_wave_sync();
    // The pair loops are self_tile_kernel's: every f goes through the hand-over block and nothing of the reduction is live across
    // a pair (the running keys would cost the band kernels the registers they do not have).  The rule is applied from LDS.
    if constexpr (DIAG) {
        #pragma nounroll
        for (int b = 0; b < 64; ++b) {
            if (!((rowmask >> b) & 1ull)) continue;   // (uniform: the column is no member)
            const float f = pair(rowI + b, rowmem && lane < b);
            if (lane < b) hand[b * 65 + lane] = f;    // pair (lane, b), lane < b: taken once, a == b never
        }
        medoid_wave_sync();
        // row 64 I + lane against the candidates j != lane of the chunk: pair (lane, j) from lane min(lane, j)
        LooKey own = kLooNoKey, other = kLooNoKey;
        if (rowmem) {
            #pragma unroll 4
            for (int j = 0; j < 64; ++j) {
                const int32_t jl = rlab[j];
                if (jl >= 0 && j != lane) loo_take(own, other, j > lane ? hand[j * 65 + lane] : hand[lane * 65 + j], rowI + j, jl, mine);
            }
            loo_merge(G.keys, rowI + lane, own, other);
        }
    } else {
        // The keys of the tile wait in LDS as 32-bit halves, so that every address of the reduction is the lane's word offset plus
        // a constant -- nothing of it is worth a register across the pair loops -- and are merged once, behind the second half.
        __shared__ uint32_t stash[8 * 64];   // [own lo, own hi, other lo, other hi] of row 64 I + lane, then of row 64 J + lane
        auto get = [&](const int k, const int i) -> LooKey { return ((LooKey)stash[(k + 1) * 64 + i] << 32) | stash[k * 64 + i]; };
        auto put = [&](const int k, const int i, const LooKey v) { stash[k * 64 + i] = (uint32_t)v, stash[(k + 1) * 64 + i] = (uint32_t)(v >> 32); };
        const unsigned long long colmask = __ballot(clab[lane] >= 0);   // the members of chunk J
        #pragma nounroll
        for (int h = 0; h < 2; ++h) {
            #pragma nounroll
            for (int bl = 0; bl < 32; ++bl) {
                if (!((colmask >> (32 * h + bl)) & 1ull)) continue;   // (uniform)
                hand[bl * 65 + lane] = pair(rowJ + 32 * h + bl, rowmem);
            }
            medoid_wave_sync();
            // the row side: row 64 I + lane over the 32 columns of this half
            const int32_t rmine = rlab[lane];
            if (rmine >= 0) {
                LooKey own = kLooNoKey, other = kLooNoKey;
                if (h == 1) own = get(0, lane), other = get(2, lane);
                #pragma unroll 4
                for (int bl = 0; bl < 32; ++bl) {
                    const int32_t cl = clab[32 * h + bl];
                    if (cl >= 0) loo_take(own, other, hand[bl * 65 + lane], rowJ + 32 * h + bl, cl, rmine);
                }
                put(0, lane, own), put(2, lane, other);
            }
            // the column side: lane c < 32 takes row 64 J + 32 h + c over the rows of chunk I
            const int32_t cmine = lane < 32 ? clab[32 * h + lane] : -1;
            if (cmine >= 0) {
                LooKey cown = kLooNoKey, cother = kLooNoKey;
                #pragma unroll 4
                for (int r = 0; r < 64; ++r) {
                    const int32_t rl = rlab[r];
                    if (rl >= 0) loo_take(cown, cother, hand[lane * 65 + r], rowI + r, rl, cmine);
                }
                put(4, 32 * h + lane, cown), put(6, 32 * h + lane, cother);
            }
            medoid_wave_sync();
        }
        if (rowmem) loo_merge(G.keys, rowI + lane, get(0, lane), get(2, lane));
        if (clab[lane] >= 0) loo_merge(G.keys, rowJ + lane, get(4, lane), get(6, lane));
    }
}

using LooTileKernel = void (*)(const LooTileArgs);
static LooTileKernel loo_tile_kernel_of(MedoidKernel k, bool diag) {
    switch (k) {
    case MedoidKernel::kShort: return diag ? loo_tile_kernel<15, true, true, true> : loo_tile_kernel<15, true, true, false>;
    case MedoidKernel::kBand8: return diag ? loo_tile_kernel<8, false, false, true> : loo_tile_kernel<8, false, false, false>;
    case MedoidKernel::kBand15: return diag ? loo_tile_kernel<15, true, false, true> : loo_tile_kernel<15, true, false, false>;
    case MedoidKernel::kBand16: return diag ? loo_tile_kernel<16, false, false, true> : loo_tile_kernel<16, false, false, false>;
    default: return diag ? loo_tile_kernel<32, false, false, true> : loo_tile_kernel<32, false, false, false>;
    }
}

// ---- the outputs of one row from its two keys ---------------------------------------------------------------------------------
__device__ __forceinline__ void loo_write(int32_t *__restrict__ nn, float *__restrict__ best, const int64_t a, const bool mem,
                                          const LooKey own, const LooKey other) {
    const LooKey k[2] = {own, other};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const bool none = !mem || k[s] == kLooNoKey;
        nn[2 * a + s] = none ? -1 : (int32_t)(uint32_t)(k[s] & 0xffffffffull);
        best[2 * a + s] = !mem ? __builtin_nanf("") : (none ? __builtin_inff() : __uint_as_float((uint32_t)(k[s] >> 32)));
    }
}

// tile route: one thread per caller's row
__global__ __launch_bounds__(256) void loo_finish_kernel(const int32_t *__restrict__ label, const LooKey *__restrict__ keys, int64_t n,
                                                         int32_t *__restrict__ nn, float *__restrict__ best) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    loo_write(nn, best, a, label[a] >= 0, keys[2 * a], keys[2 * a + 1]);
}

// general route: one wave per row of the block M (rows, ld) = padded rows [r0, r0 + rows) against every padded row
__global__ __launch_bounds__(256) void loo_rows_kernel(const float *__restrict__ M, int64_t r0, int64_t rows, int64_t ld,
                                                       const int32_t *__restrict__ label, int64_t n, int32_t *__restrict__ nn,
                                                       float *__restrict__ best) {
    const int64_t rl = (int64_t)blockIdx.x * 4 + threadIdx.x / 64, a = r0 + rl;
    const int lane = threadIdx.x & 63;
    if (rl >= rows || a >= n) return;   // (uniform over the wave)
    const int32_t mine = label[a];
    LooKey own = kLooNoKey, other = kLooNoKey;
    if (mine >= 0) {
        const float *__restrict__ m = M + rl * ld;
        for (int64_t b = lane; b < n; b += 64) {
            const int32_t lb = label[b];
            if (lb >= 0 && b != a) loo_take(own, other, m[b], b, lb, mine);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const LooKey po = __shfl_xor(own, off), pt = __shfl_xor(other, off);
        own = po < own ? po : own, other = pt < other ? pt : other;
    }
    if (lane == 0) loo_write(nn, best, a, mine >= 0, own, other);
}

// One block of padded rows through the DTW dispatch: rows [B.r0, B.r0 + B.rows) against all padded rows, into the block
static int loo_matrix_block(wdx_ctx *ctx, const LooPlan &LP, const LooBlock &B, int32_t window, double penalty, const double *dense,
                            const double *padded, float *M, hipStream_t s) {
    const int64_t cols = LP.rows_padded;
    const DtwPlan P = dtw_plan(B.rows, cols, LP.L, window, false, DtwEntry::kMatrix, ctx->knobs.dtw_switches());
    if (P.info.family == WDX_DTW_NONE || P.prep == DtwPrep::kPaddedReads) {   // (rows is a multiple of 64: the lanes are the rows)
        set_error("self nearest: no DTW dispatch for a %lld x %lld block", (long long)B.rows, (long long)cols);
        return WDX_ERR_UNSUPPORTED;
    }
    int rc;
    if (P.scratch_bytes && (rc = ctx->scratch.ensure((size_t)P.scratch_bytes))) return rc;
    if (P.copy_bytes && (rc = ctx->tmp1.ensure((size_t)P.copy_bytes))) return rc;
    if (P.flag_bytes && (rc = ctx->tmp2.ensure((size_t)P.flag_bytes))) return rc;
    const double *A = dense + B.r0 * LP.L;
    DtwOperands op{A, 1, B.rows, nullptr, padded, LP.Lpad, kDtwHalo, cols, nullptr, penalty, M, cols, 1,
                   nullptr, ctx->scratch.p, (int64_t)ctx->scratch.bytes, ctx->knobs.dtw_unfused, s};
    if (P.prep == DtwPrep::kReadMinor) {
        if ((rc = launch_transpose(A, B.rows, LP.L, (double *)ctx->tmp1.p, P.ld, (uint8_t *)ctx->tmp2.p, s))) return rc;
        op.A = (const double *)ctx->tmp1.p, op.ldA = P.ld, op.a_nan = (const uint8_t *)ctx->tmp2.p;
    }
    return run_dtw_plan(P, op, &ctx->dtw_last);
}

static LooPlan loo_plan_of(const wdx_ctx *ctx, int64_t n, int64_t L, int32_t window, bool have_out) {
    return loo_plan(n, L, window, have_out, ctx->knobs.self_nearest_general, ctx->knobs.no_short_dtw);
}

// the refusals of both forms, before anything is sized by the arguments
static int loo_refusals(const LooPlan &P, const void *X) {
    if (P.rc != WDX_SUCCESS) {
        set_error("%s", P.msg);
        return P.rc;
    }
    if (P.n > 0 && !X) {
        set_error("self nearest: the fingerprints are required (NULL given)");
        return WDX_ERR_INVALID;
    }
    return WDX_SUCCESS;
}

// With the context's mutex held.  Every pointer is device memory.
static int self_nearest_locked(wdx_ctx *ctx, const double *dX, int64_t n, int64_t L, const int32_t *d_label, const int32_t *d_status,
                               int32_t window, double penalty, int32_t *d_nn, float *d_best, hipStream_t s) {
    const LooPlan P = loo_plan_of(ctx, n, L, window, d_nn != nullptr && d_best != nullptr);
    int rc;
    if ((rc = loo_refusals(P, dX))) return rc;
    if (n == 0) return WDX_SUCCESS;
    if ((rc = use_stream(ctx, s))) return rc;
    if ((rc = ctx->loo_ws.ensure((size_t)P.workspace_bytes))) return rc;
    uint8_t *const ws = (uint8_t *)ctx->loo_ws.p;
    uint8_t *member = ws + P.off_member;
    int32_t *label = (int32_t *)(ws + P.off_label);
    LooKey *keys = (LooKey *)(ws + P.off_keys);
    double *dense = (double *)(ws + P.off_dense), *padded = (double *)(ws + P.off_padded);
    float *block = (float *)(ws + P.off_block);
    const int w_eff = (int)dtw_effective_window(L, window);
    Timed t(ctx, WDX_K_SELF_NEAREST, s);
    hipLaunchKernelGGL(tile_gather_kernel<true>, dim3((unsigned)((P.rows_padded + 3) / 4)), dim3(256), 0, s, dX, d_status,
                       (const int32_t *)nullptr, n, P.rows_padded, (int)L, P.Lpad, kDtwHalo, dense, padded, member);
    hipLaunchKernelGGL(loo_init_kernel, dim3((unsigned)((P.rows_padded + 255) / 256)), dim3(256), 0, s, d_label, n, P.rows_padded, member,
                       label, keys);
    WDX_HIP_TRY(hipGetLastError());
    if (!P.general) {
        const LooTileArgs G{dense, padded, P.Lpad, kDtwHalo, label, P.chunks, keys, (int)L, w_eff, penalty * penalty, ctx->knobs.dtw_unfused};
        hipLaunchKernelGGL(loo_tile_kernel_of(P.kernel, true), dim3((unsigned)P.n_diag), dim3(64), 0, s, G);
        if (P.n_off) hipLaunchKernelGGL(loo_tile_kernel_of(P.kernel, false), dim3((unsigned)P.n_off), dim3(64), 0, s, G);
        hipLaunchKernelGGL(loo_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, label, keys, n, d_nn, d_best);
        WDX_HIP_TRY(hipGetLastError());
        return WDX_SUCCESS;
    }
    for (const LooBlock &B : P.blocks) {
        if ((rc = loo_matrix_block(ctx, P, B, window, penalty, dense, padded, block, s))) return rc;
        hipLaunchKernelGGL(loo_rows_kernel, dim3((unsigned)((B.rows + 3) / 4)), dim3(256), 0, s, block, B.r0, B.rows, P.rows_padded, label, n,
                           d_nn, d_best);
        WDX_HIP_TRY(hipGetLastError());
    }
    return WDX_SUCCESS;
}

}  // namespace wdx

using namespace wdx;

extern "C" {

int wdx_self_nearest_device(wdx_ctx *ctx, const double *dX, int64_t n, int64_t L, const int32_t *d_label, const int32_t *d_status,
                            int32_t window, double penalty, int32_t *d_nn, float *d_best, void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    return self_nearest_locked(ctx, dX, n, L, d_label, d_status, window, penalty, d_nn, d_best, (hipStream_t)stream);
}

int wdx_dtw_self_nearest(wdx_ctx *ctx, const double *X, int64_t n, int64_t L, const int32_t *label, const int32_t *status,
                         int32_t window, double penalty, int32_t *nn, float *best) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    if ((rc = loo_refusals(loo_plan_of(ctx, n, L, window, nn != nullptr && best != nullptr), X))) return rc;
    if (n == 0) return WDX_SUCCESS;
    hipStream_t s = ctx->stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const size_t xb = (size_t)(n * L) * sizeof(double), ib = (size_t)n * sizeof(int32_t);
    if ((rc = ctx->in0.ensure(xb))) return rc;
    if (status && (rc = ctx->in1.ensure(ib))) return rc;
    if (label && (rc = ctx->in2.ensure(ib))) return rc;
    if ((rc = ctx->out0.ensure(2 * ib))) return rc;
    if ((rc = ctx->out1.ensure(2 * (size_t)n * sizeof(float)))) return rc;
    StreamDrain drain(s);
    WDX_HIP_TRY(hipMemcpyAsync(ctx->in0.p, X, xb, hipMemcpyHostToDevice, s));
    if (status) WDX_HIP_TRY(hipMemcpyAsync(ctx->in1.p, status, ib, hipMemcpyHostToDevice, s));
    if (label) WDX_HIP_TRY(hipMemcpyAsync(ctx->in2.p, label, ib, hipMemcpyHostToDevice, s));
    if ((rc = self_nearest_locked(ctx, (const double *)ctx->in0.p, n, L, label ? (const int32_t *)ctx->in2.p : nullptr,
                                  status ? (const int32_t *)ctx->in1.p : nullptr, window, penalty, (int32_t *)ctx->out0.p, (float *)ctx->out1.p, s)))
        return rc;
    WDX_HIP_TRY(hipMemcpyAsync(nn, ctx->out0.p, 2 * ib, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipMemcpyAsync(best, ctx->out1.p, 2 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    return WDX_SUCCESS;
}

}  // extern "C"
