// The symmetric DTW self-distance matrix for gfx950 (include/wdx.h: wdx_self_matrix_device states the rule; wdx_self_plan.h what
// a call does with its sizes).
//
// Tile route (DESIGN.md "Self-distance matrix"): the medoid path's machinery with the distances kept.  The rows are gathered in
// their own order into the padded layout (wdx_dtw_tile.h: tile_gather_kernel<true>); one WAVE takes one 64 x 64 tile (I, J),
// J >= I.  Lane a owns row 64 I + a and walks the columns of chunk J, the column being the uniform operand on the scalar path.
// Each half of 32 columns goes through the hand[column * 65 + row] block in LDS, and from there both images of the tile are
// written with contiguous lanes: the mirror rows 64 J + column, columns 64 I + lane (256 B per instruction), and the upper rows
// two at a time (2 x 128 B per instruction).  Each unordered pair is computed once; a diagonal tile takes the whole tile in LDS
// and each pair from lane min(a, b).  Non-members give the quiet NaN; rows and columns >= n are not written.
// General route: row blocks through dtw_plan / run_dtw_plan straight into the matrix, then a mask kernel for the non-members.
#include "wdx_ctx.h"
#include "wdx_dtw_tile.h"
#include "wdx_self_plan.h"

#include <math.h>

namespace wdx {

struct SelfTileArgs {
    const double *dense;     // (rows_padded, L): a lane's own row
    const double *padded;    // (rows_padded, Lpad): the uniform operand, series at +halo
    int64_t Lpad;
    int halo;
    const uint8_t *member;   // [rows_padded]
    int64_t chunks;
    float *out;              // (n, ld)
    int64_t ld, n;
    int L, w;
    double p2;
    int unfused;             // Knobs::dtw_unfused
};

// SHORT: the unrolled 25-point / window-15 shape (W, EXACT_W ignored); DIAG: tile (I, I), the whole 64 x 64 hand-over in LDS.
// (held to the three waves per SIMD the band kernels run at, like medoid_tile_kernel)
template <int W, bool EXACT_W, bool SHORT, bool DIAG>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((SHORT || W == 15) ? 3 : 0))) void self_tile_kernel(
    const SelfTileArgs G) {
    constexpr int COLS = DIAG ? 64 : 32;
    constexpr int LS = 25, WS = 15;
    __shared__ float hand[COLS * 65];   // hand[column * 65 + row]: the pair loop writes it contiguous over the lanes
    const int lane = threadIdx.x;
    int32_t I, J;
    if (DIAG) I = J = (int32_t)blockIdx.x;
    else medoid_upper_tile(G.chunks, (int64_t)blockIdx.x, &I, &J);
    // (the tile is the wave's: said outright, so that everything derived from it stays on the scalar path)
    I = __builtin_amdgcn_readfirstlane(I), J = __builtin_amdgcn_readfirstlane(J);
    const int64_t rowI = kMedoidChunk * (int64_t)I, rowJ = kMedoidChunk * (int64_t)J;
    const int64_t n = G.n, ld = G.ld;
    const bool rowmem = G.member[rowI + lane] != 0;
    const unsigned long long rowmask = __ballot(rowmem);
    const int L = SHORT ? LS : G.L;
    const double *__restrict__ xp = G.dense + (rowI + lane) * (int64_t)L;
    float *__restrict__ out = G.out;
    const double delta = dtw_delta(L);
    const float qnan = __builtin_nanf("");   // 0x7fc00000
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
    if constexpr (DIAG) {
        #pragma nounroll
        for (int b = 0; b < 64; ++b) {
            float f = qnan;
            if ((rowmask >> b) & 1ull) {   // (uniform branch: the column is a member)
                f = pair(rowI + b, rowmem && lane <= b);
                f = rowmem ? f : qnan;
            }
            if (lane <= b) hand[b * 65 + lane] = f;   // pair (lane, b), lane <= b: taken once
        }
        medoid_wave_sync();
        // row 64 I + r, columns 64 I + lane: pair (r, lane) from lane min(r, lane)
        const bool colin = rowI + lane < n;
        #pragma unroll 4
        for (int r = 0; r < 64; ++r) {
            if (rowI + r >= n) break;   // (uniform)
            const float f = lane >= r ? hand[lane * 65 + r] : hand[r * 65 + lane];
            if (colin) out[(rowI + r) * ld + rowI + lane] = f;
        }
    } else {
        const unsigned long long colmask = __ballot(G.member[rowJ + lane] != 0);   // the members of chunk J
        #pragma nounroll
        for (int h = 0; h < 2; ++h) {
            #pragma nounroll
            for (int bl = 0; bl < 32; ++bl) {
                const int64_t col = rowJ + 32 * h + bl;
                float f = qnan;
                if ((colmask >> (32 * h + bl)) & 1ull) {   // (uniform)
                    f = pair(col, rowmem);
                    f = rowmem ? f : qnan;
                }
                hand[bl * 65 + lane] = f;
            }
            medoid_wave_sync();
            // (every row of chunk I is a row of the matrix: I < J and chunk J exists; only chunk J may reach beyond n)
            // the mirror image: row 64 J + 32 h + bl, columns 64 I + lane -- 256 B per instruction
            #pragma unroll 4
            for (int bl = 0; bl < 32; ++bl) {
                const int64_t r = rowJ + 32 * h + bl;
                if (r >= n) break;   // (uniform)
                out[r * ld + rowI + lane] = hand[bl * 65 + lane];
            }
            // the upper image: rows 64 I + 2 k and 64 I + 2 k + 1, columns 64 J + 32 h + (lane & 31) -- two rows of 128 B
            const int c = lane & 31, up = lane >> 5;
            const int64_t cc = rowJ + 32 * h + c;
            const bool colin = cc < n;
            #pragma unroll 4
            for (int k = 0; k < 32; ++k) {
                const int a = 2 * k + up;
                const float f = hand[c * 65 + a];
                if (colin) out[(rowI + a) * ld + cc] = f;
            }
            medoid_wave_sync();
        }
    }
}

using SelfTileKernel = void (*)(const SelfTileArgs);
static SelfTileKernel self_tile_kernel_of(MedoidKernel k, bool diag) {
    switch (k) {
    case MedoidKernel::kShort: return diag ? self_tile_kernel<15, true, true, true> : self_tile_kernel<15, true, true, false>;
    case MedoidKernel::kBand8: return diag ? self_tile_kernel<8, false, false, true> : self_tile_kernel<8, false, false, false>;
    case MedoidKernel::kBand15: return diag ? self_tile_kernel<15, true, false, true> : self_tile_kernel<15, true, false, false>;
    case MedoidKernel::kBand16: return diag ? self_tile_kernel<16, false, false, true> : self_tile_kernel<16, false, false, false>;
    default: return diag ? self_tile_kernel<32, false, false, true> : self_tile_kernel<32, false, false, false>;
    }
}

// ---- general route: the quiet NaN wherever a row or a column is no member -----------------------------------------------------
// grid (n, ceil(n / 256)): block (a, cb) takes columns 256 cb .. of row a
__global__ __launch_bounds__(256) void self_mask_kernel(const uint8_t *__restrict__ member, int64_t n, int64_t ld,
                                                        float *__restrict__ out) {
    const int64_t a = blockIdx.x, b = (int64_t)blockIdx.y * 256 + threadIdx.x;
    if (b >= n) return;
    if (!member[a] || !member[b]) out[a * ld + b] = __builtin_nanf("");
}

// One row block through the DTW dispatch: rows [r0, r0 + rows) against all n rows, straight into the matrix
static int self_matrix_block(wdx_ctx *ctx, const SelfPlan &SP, const SelfBlock &B, int32_t window, double penalty, const double *dense,
                             const double *padded, float *d_out, hipStream_t s) {
    DtwSwitches sw = ctx->knobs.dtw_switches();
    sw.no_wavefront = true;   // (the wavefront kernel writes a dense (rows, n) block: it knows no leading dimension)
    const DtwPlan P = dtw_plan(B.rows, SP.n, SP.L, window, false, DtwEntry::kMatrix, sw);
    if (P.info.family == WDX_DTW_NONE || P.prep == DtwPrep::kPaddedReads) {   // (a block has 64 rows or all of them: its rows are the lanes)
        set_error("self matrix: no DTW dispatch for a %lld x %lld block", (long long)B.rows, (long long)SP.n);
        return WDX_ERR_UNSUPPORTED;
    }
    int rc;
    if (P.scratch_bytes && (rc = ctx->scratch.ensure((size_t)P.scratch_bytes))) return rc;
    if (P.copy_bytes && (rc = ctx->tmp1.ensure((size_t)P.copy_bytes))) return rc;
    if (P.flag_bytes && (rc = ctx->tmp2.ensure((size_t)P.flag_bytes))) return rc;
    const double *A = dense + B.r0 * SP.L;
    DtwOperands op{A, 1, B.rows, nullptr, padded, SP.Lpad, kDtwHalo, SP.n, nullptr, penalty, d_out + B.r0 * SP.ld, SP.ld, 1,
                   nullptr, ctx->scratch.p, (int64_t)ctx->scratch.bytes, ctx->knobs.dtw_unfused, s};
    if (P.prep == DtwPrep::kReadMinor) {
        if ((rc = launch_transpose(A, B.rows, SP.L, (double *)ctx->tmp1.p, P.ld, (uint8_t *)ctx->tmp2.p, s))) return rc;
        op.A = (const double *)ctx->tmp1.p, op.ldA = P.ld, op.a_nan = (const uint8_t *)ctx->tmp2.p;
    }
    return run_dtw_plan(P, op, &ctx->dtw_last);
}

static SelfPlan self_plan_of(const wdx_ctx *ctx, int64_t n, int64_t L, int64_t ld, int32_t window, bool have_out) {
    return self_plan(n, L, ld, window, have_out, ctx->knobs.self_matrix_general, ctx->knobs.no_short_dtw);
}

// With the context's mutex held.  Every pointer is device memory.
static int self_matrix_locked(wdx_ctx *ctx, const double *dX, int64_t n, int64_t L, const int32_t *d_status, int32_t window,
                              double penalty, float *d_out, int64_t ld, hipStream_t s) {
    const SelfPlan P = self_plan_of(ctx, n, L, ld, window, d_out != nullptr);
    if (P.rc != WDX_SUCCESS) {
        set_error("%s", P.msg);
        return P.rc;
    }
    if (n > 0 && !dX) {
        set_error("self matrix: the fingerprints are required (NULL given)");
        return WDX_ERR_INVALID;
    }
    if (n == 0) return WDX_SUCCESS;
    int rc;
    if ((rc = use_stream(ctx, s))) return rc;
    if ((rc = ctx->self_ws.ensure((size_t)P.workspace_bytes))) return rc;
    uint8_t *const ws = (uint8_t *)ctx->self_ws.p;
    uint8_t *member = ws + P.off_member;
    double *dense = (double *)(ws + P.off_dense), *padded = (double *)(ws + P.off_padded);
    const int w_eff = (int)dtw_effective_window(L, window);
    Timed t(ctx, WDX_K_DTW, s);
    hipLaunchKernelGGL(tile_gather_kernel<true>, dim3((unsigned)((P.rows_padded + 3) / 4)), dim3(256), 0, s, dX, d_status,
                       (const int32_t *)nullptr, n, P.rows_padded, (int)L, P.Lpad, kDtwHalo, dense, padded, member);
    WDX_HIP_TRY(hipGetLastError());
    if (!P.general) {
        const SelfTileArgs G{dense, padded, P.Lpad, kDtwHalo, member, P.chunks, d_out, ld, n, (int)L, w_eff, penalty * penalty,
                             ctx->knobs.dtw_unfused};
        hipLaunchKernelGGL(self_tile_kernel_of(P.kernel, true), dim3((unsigned)P.n_diag), dim3(64), 0, s, G);
        if (P.n_off) hipLaunchKernelGGL(self_tile_kernel_of(P.kernel, false), dim3((unsigned)P.n_off), dim3(64), 0, s, G);
        WDX_HIP_TRY(hipGetLastError());
        return WDX_SUCCESS;
    }
    for (const SelfBlock &B : P.blocks)
        if ((rc = self_matrix_block(ctx, P, B, window, penalty, dense, padded, d_out, s))) return rc;
    hipLaunchKernelGGL(self_mask_kernel, dim3((unsigned)n, (unsigned)((n + 255) / 256)), dim3(256), 0, s, member, n, ld, d_out);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

}  // namespace wdx

using namespace wdx;

extern "C" {

int wdx_self_matrix_device(wdx_ctx *ctx, const double *dX, int64_t n, int64_t L, const int32_t *d_status, int32_t window,
                           double penalty, float *d_out, int64_t ld, void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    return self_matrix_locked(ctx, dX, n, L, d_status, window, penalty, d_out, ld, (hipStream_t)stream);
}

int wdx_dtw_self_matrix(wdx_ctx *ctx, const double *X, int64_t n, int64_t L, const int32_t *status, int32_t window, double penalty,
                        float *out, int64_t ld) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    {   // the refusals before anything is sized by the arguments
        const SelfPlan P = self_plan_of(ctx, n, L, ld, window, out != nullptr);
        if (P.rc == WDX_SUCCESS && n > 0 && !X) {
            set_error("self matrix: the fingerprints are required (NULL given)");
            return WDX_ERR_INVALID;
        }
        if (P.rc != WDX_SUCCESS) {
            set_error("%s", P.msg);
            return P.rc;
        }
    }
    if (n == 0) return WDX_SUCCESS;
    hipStream_t s = ctx->stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const size_t xb = (size_t)(n * L) * sizeof(double);
    if ((rc = ctx->in0.ensure(xb))) return rc;
    if (status && (rc = ctx->in1.ensure((size_t)n * sizeof(int32_t)))) return rc;
    // the matrix lives for this call only: a context never keeps 16 GiB
    struct Matrix {
        float *p = nullptr;
        ~Matrix() {
            if (p) (void)hipFree(p);
        }
    } M;
    WDX_HIP_TRY(hipMalloc((void **)&M.p, (size_t)n * (size_t)n * sizeof(float)));
    {
        StreamDrain drain(s);   // (declared behind M: the stream is drained before the matrix is freed)
        WDX_HIP_TRY(hipMemcpyAsync(ctx->in0.p, X, xb, hipMemcpyHostToDevice, s));
        if (status) WDX_HIP_TRY(hipMemcpyAsync(ctx->in1.p, status, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if ((rc = self_matrix_locked(ctx, (const double *)ctx->in0.p, n, L, status ? (const int32_t *)ctx->in1.p : nullptr, window, penalty,
                                     M.p, n, s)))
            return rc;
        WDX_HIP_TRY(hipMemcpy2DAsync(out, (size_t)ld * sizeof(float), M.p, (size_t)n * sizeof(float), (size_t)n * sizeof(float), (size_t)n,
                                     hipMemcpyDeviceToHost, s));
        WDX_HIP_TRY(hipStreamSynchronize(s));
        drain.done();
    }
    return WDX_SUCCESS;
}

}  // extern "C"
