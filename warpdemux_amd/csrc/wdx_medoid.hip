// Per-label DTW medoids for gfx950 (include/wdx.h: wdx_medoids_device states the rule; wdx_medoid_plan.h what a call does with
// its host labels).
//
// Tile route (DESIGN.md "Medoids"): the label's rows are gathered into a padded layout (every label starts on a multiple of 64
// rows); one WAVE takes one 64 x 64 tile (I, J), J >= I, of the label's chunk x chunk matrix.  Lane a owns row 64 I + a and walks
// the columns of chunk J with the lane-per-pair machinery of wdx_dtw.hip (wdx_dtw_cells.h: the register band, the fused pass and
// the settle pass; the column is the uniform operand and arrives through scalar loads of its padded row).  The lane adds each
// float32 distance to its row's chunk sum S_J in a register -- sequential in rising column order by construction -- and hands it
// through LDS to the column's owner, which adds the 64 values of its column in rising ROW order (S_I of the rows of chunk J): a
// tree over the lanes would give other bits.  Each unordered pair is computed once; each (chunk, row) partial sum is written
// once, without atomics.  The hand-over runs in halves of 32 columns (32 x 65 float32 = 8.1 KiB of LDS per wave; a whole tile
// would be 16.3 KiB and twelve waves of that do not fit a CU); the few diagonal tiles take the whole tile in LDS and a kernel of
// their own.
// General route: the label's matrix block by block through dtw_plan / run_dtw_plan, then chunk sums of each row's own entries.
// Reduce: per label, the partial sums of a row in rising chunk order -> cost, the first minimum -> medoid, and the gathers.
#include "wdx_ctx.h"
#include "wdx_dtw_tile.h"
#include "wdx_medoid_plan.h"

#include <math.h>
#include <string.h>
#include <algorithm>

namespace wdx {

// (the pre-pass, tile_gather_kernel, and the pair on the register band live in wdx_dtw_tile.h: the self-matrix kernels share them)
__global__ __launch_bounds__(256) void medoid_fill_nan_kernel(double *__restrict__ cost, int64_t n) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) cost[r] = __builtin_nan("");
}

// ---- the tile kernels ---------------------------------------------------------------------------------------------------------
struct MedoidTileArgs {
    const double *dense;     // (rows_padded, L): a lane's own row
    const double *padded;    // (rows_padded, Lpad): the uniform operand, series at +halo
    int64_t Lpad;
    int halo;
    const uint8_t *member;   // [rows_padded]
    const MedoidLabel *labels;
    int32_t g0, g1;          // the labels of the pass
    int64_t tile0;           // number of the grid's first tile in its list (diagonal or strictly upper)
    double *partial;         // the pass's block
    int L, w;
    double p2;
    int unfused;             // Knobs::dtw_unfused
};

// SHORT: the unrolled 25-point / window-15 shape (W, EXACT_W ignored); DIAG: tile (I, I), the whole 64 x 64 hand-over in LDS.
// (held to the three waves per SIMD the band kernels run at, like their NEAREST twins)
template <int W, bool EXACT_W, bool SHORT, bool DIAG>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((SHORT || W == 15) ? 3 : 0))) void medoid_tile_kernel(
    const MedoidTileArgs G) {
    constexpr int COLS = DIAG ? 64 : 32;
    constexpr int LS = 25, WS = 15;
    __shared__ float hand[COLS * 65];   // hand[column * 65 + row]: writes contiguous over the lanes, reads conflict-free
    const int lane = threadIdx.x;
    const int64_t T = G.tile0 + blockIdx.x;
    const int32_t g = medoid_tile_label(G.labels, DIAG, G.g0, G.g1, T);
    const MedoidLabel Lb = G.labels[g];   // (uniform)
    int32_t I, J;
    if (DIAG) I = J = (int32_t)(T - Lb.diag0);
    else medoid_upper_tile(Lb.chunks, T - Lb.off0, &I, &J);
    // (the tile is the wave's: said outright, so that everything derived from it -- the columns' rows above all -- stays on the
    // scalar path; behind the bisections the compiler no longer sees it)
    I = __builtin_amdgcn_readfirstlane(I), J = __builtin_amdgcn_readfirstlane(J);
    const int64_t ld = kMedoidChunk * (int64_t)Lb.chunks;
    const int64_t rowI = Lb.row0 + kMedoidChunk * (int64_t)I, rowJ = Lb.row0 + kMedoidChunk * (int64_t)J;
    const bool rowmem = G.member[rowI + lane] != 0;
    const unsigned long long rowmask = __ballot(rowmem);
    const int L = SHORT ? LS : G.L;
    const double *__restrict__ xp = G.dense + (rowI + lane) * (int64_t)L;
    double *__restrict__ part = G.partial + Lb.part0;
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
    if constexpr (DIAG) {
        #pragma nounroll
        for (int b = 0; b < 64; ++b) {
            float f = 0.0f;
            if ((rowmask >> b) & 1ull) f = pair(rowI + b, rowmem && lane <= b);   // (uniform branch: the column is a member)
            if (lane <= b) hand[b * 65 + lane] = f;   // pair (lane, b), lane <= b: taken once
        }
        medoid_wave_sync();
        double s = 0.0;
        #pragma unroll 4
        for (int j = 0; j < 64; ++j)
            if ((rowmask >> j) & 1ull) s += (double)(j < lane ? hand[lane * 65 + j] : hand[j * 65 + lane]);
        part[(int64_t)I * ld + kMedoidChunk * (int64_t)I + lane] = s;
    } else {
        const unsigned long long colmask = __ballot(G.member[rowJ + lane] != 0);   // the members of chunk J
        double rowsum = 0.0;   // S_J of this lane's row
        double colsum = 0.0;   // S_I of the row whose column this lane owns (lane l: column 64 J + l)
        #pragma nounroll
        for (int h = 0; h < 2; ++h) {
            #pragma nounroll
            for (int bl = 0; bl < 32; ++bl) {
                const int64_t col = rowJ + 32 * h + bl;
                float f = 0.0f;
                if ((colmask >> (32 * h + bl)) & 1ull) {   // (uniform)
                    f = pair(col, rowmem);
                    rowsum += (double)f;
                }
                hand[bl * 65 + lane] = f;
            }
            medoid_wave_sync();
            if ((lane >> 5) == h) {   // lane l owns column 64 J + l: S_I of that row, over the member rows of chunk I in rising order
#pragma unroll 4
                for (int a = 0; a < 64; ++a)
                    if ((rowmask >> a) & 1ull) colsum += (double)hand[(lane & 31) * 65 + a];
            }
            medoid_wave_sync();
        }
        // (both stores behind the column loop: a global store inside it would make the rows of `padded` possibly overwritten in the
        // compiler's eyes, and the uniform operand would leave the scalar path -- vector loads and 65 to 87 spilled registers)
        part[(int64_t)I * ld + kMedoidChunk * (int64_t)J + lane] = colsum;
        part[(int64_t)J * ld + kMedoidChunk * (int64_t)I + lane] = rowsum;
    }
}

using MedoidTileKernel = void (*)(const MedoidTileArgs);
static MedoidTileKernel medoid_tile_kernel_of(MedoidKernel k, bool diag) {
    switch (k) {
    case MedoidKernel::kShort: return diag ? medoid_tile_kernel<15, true, true, true> : medoid_tile_kernel<15, true, true, false>;
    case MedoidKernel::kBand8: return diag ? medoid_tile_kernel<8, false, false, true> : medoid_tile_kernel<8, false, false, false>;
    case MedoidKernel::kBand15: return diag ? medoid_tile_kernel<15, true, false, true> : medoid_tile_kernel<15, true, false, false>;
    case MedoidKernel::kBand16: return diag ? medoid_tile_kernel<16, false, false, true> : medoid_tile_kernel<16, false, false, false>;
    default: return diag ? medoid_tile_kernel<32, false, false, true> : medoid_tile_kernel<32, false, false, false>;
    }
}

// ---- general route: chunk sums of a row's own matrix entries -----------------------------------------------------------------
// M (rows, ld) float32: rows r0 .. r0 + rows - 1 of the label against its ld = 64 x chunks padded rows.  One thread per (row,
// chunk): partial[chunk][r0 + row] = the float64 sum over the chunk's members in rising column order.
__global__ __launch_bounds__(256) void medoid_chunk_sum_kernel(const float *__restrict__ M, int64_t rows, int64_t ld, int chunks,
                                                               const uint8_t *__restrict__ member /* of the label */, int64_t r0,
                                                               double *__restrict__ part) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * chunks) return;
    const int64_t rl = idx % rows, c = idx / rows;
    const float *__restrict__ m = M + rl * ld + c * kMedoidChunk;
    const uint8_t *__restrict__ mem = member + c * kMedoidChunk;
    double s = 0.0;
    for (int j = 0; j < 64; ++j)
        if (mem[j]) s += (double)m[j];
    part[c * ld + r0 + rl] = s;
}

// ---- reduce: cost, first minimum, gathers ------------------------------------------------------------------------------------
struct MedoidReduceArgs {
    const MedoidLabel *labels;
    int32_t g0;
    const double *partial;
    const uint8_t *member;
    const int32_t *order;
    const double *X;
    int L;
    int64_t *medoid;
    double *medoid_cost;
    int64_t *count;
    double *cost;
    double *refs;
};
__global__ __launch_bounds__(256) void medoid_reduce_kernel(const MedoidReduceArgs R) {
    __shared__ double s_cost[256];
    __shared__ int s_idx[256], s_cnt[256];
    __shared__ int64_t s_src;
    const int tid = threadIdx.x;
    const int32_t g = R.g0 + blockIdx.x;
    const MedoidLabel Lb = R.labels[g];
    const int64_t ld = kMedoidChunk * (int64_t)Lb.chunks;
    const double *__restrict__ part = R.partial + Lb.part0;
    double best = 0.0;
    int bidx = -1, cnt = 0;
    for (int r = tid; r < Lb.size; r += 256) {
        const bool mem = R.member[Lb.row0 + r] != 0;
        double c = __builtin_nan("");
        if (mem) {
            c = 0.0;
            for (int k = 0; k < Lb.chunks; ++k) c += part[(int64_t)k * ld + r];   // the chunk sums in rising chunk order
            ++cnt;
            if (bidx < 0 || c < best) best = c, bidx = r;   // (a thread's rows rise: the first minimum among them)
        }
        if (R.cost) R.cost[R.order[Lb.row0 + r]] = c;
    }
    s_cost[tid] = best, s_idx[tid] = bidx, s_cnt[tid] = cnt;
    __syncthreads();
    if (tid == 0) {
        for (int t = 1; t < 256; ++t) {
            cnt += s_cnt[t];
            if (s_idx[t] < 0) continue;
            if (bidx < 0 || s_cost[t] < best || (s_cost[t] == best && s_idx[t] < bidx)) best = s_cost[t], bidx = s_idx[t];
        }
        const int64_t src = bidx < 0 ? -1 : (int64_t)R.order[Lb.row0 + bidx];
        s_src = src;
        R.medoid[g] = src;
        if (R.medoid_cost) R.medoid_cost[g] = bidx < 0 ? __builtin_nan("") : best;
        if (R.count) R.count[g] = cnt;
    }
    __syncthreads();
    if (R.refs) {
        const int64_t src = s_src;
        for (int i = tid; i < R.L; i += 256) R.refs[(int64_t)g * R.L + i] = src < 0 ? __builtin_nan("") : R.X[src * R.L + i];
    }
}

// ---- the call ------------------------------------------------------------------------------------------------------------------
void medoid_release_staged(wdx_ctx *ctx, bool all) {
    auto &v = ctx->medoid_staged;
    for (size_t i = 0; i < v.size();) {
        if (all) (void)hipEventSynchronize(v[i].copied);
        if (all || hipEventQuery(v[i].copied) == hipSuccess) {
            (void)hipEventDestroy(v[i].copied);
            (void)hipHostFree(v[i].host);
            v[i] = v.back();
            v.pop_back();
        } else {
            ++i;
        }
    }
}

// A page-locked block of `bytes` whose previous copy has run: one of the context's, or a new one (then the idle ones, all too
// small, are freed first).  The caller fills it, enqueues its copy and records `copied` behind it.
int medoid_stage_block(wdx_ctx *ctx, size_t bytes, MedoidStage **out) {
    for (MedoidStage &S : ctx->medoid_staged)
        if (S.bytes >= bytes && hipEventQuery(S.copied) == hipSuccess) {
            *out = &S;
            return WDX_SUCCESS;
        }
    medoid_release_staged(ctx, false);
    MedoidStage S;
    S.bytes = bytes + bytes / 4;   // (head-room: a slightly larger batch reuses it)
    WDX_HIP_TRY(hipHostMalloc(&S.host, S.bytes, hipHostMallocDefault));
    if (hipEventCreateWithFlags(&S.copied, hipEventDisableTiming) != hipSuccess) {
        (void)hipHostFree(S.host);
        set_error("medoids: hipEventCreateWithFlags failed");
        return WDX_ERR_HIP;
    }
    ctx->medoid_staged.push_back(S);
    *out = &ctx->medoid_staged.back();
    return WDX_SUCCESS;
}

// One block of the label's matrix through the DTW dispatch: padded rows [r0, r0 + rows) of label Lb against all its padded rows
static int medoid_matrix_block(wdx_ctx *ctx, const MedoidPlan &MP, const MedoidLabel &Lb, int64_t r0, int64_t rows, int32_t window,
                               double penalty, const double *dense, const double *padded, float *M, hipStream_t s) {
    const int64_t cols = kMedoidChunk * (int64_t)Lb.chunks;
    const DtwPlan P = dtw_plan(rows, cols, MP.L, window, false, DtwEntry::kMatrix, ctx->knobs.dtw_switches());
    if (P.info.family == WDX_DTW_NONE || P.prep == DtwPrep::kPaddedReads) {   // (rows is a multiple of 64: the lanes are the rows)
        set_error("medoids: no DTW dispatch for a %lld x %lld block", (long long)rows, (long long)cols);
        return WDX_ERR_UNSUPPORTED;
    }
    int rc;
    if (P.scratch_bytes && (rc = ctx->scratch.ensure((size_t)P.scratch_bytes))) return rc;
    if (P.copy_bytes && (rc = ctx->tmp1.ensure((size_t)P.copy_bytes))) return rc;
    if (P.flag_bytes && (rc = ctx->tmp2.ensure((size_t)P.flag_bytes))) return rc;
    const double *A = dense + (Lb.row0 + r0) * MP.L;
    DtwOperands op{A, 1, rows, nullptr, padded + Lb.row0 * MP.Lpad, MP.Lpad, kDtwHalo, cols, nullptr, penalty, M, cols, 1,
                   nullptr, ctx->scratch.p, (int64_t)ctx->scratch.bytes, ctx->knobs.dtw_unfused, s};
    if (P.prep == DtwPrep::kReadMinor) {
        if ((rc = launch_transpose(A, rows, MP.L, (double *)ctx->tmp1.p, P.ld, (uint8_t *)ctx->tmp2.p, s))) return rc;
        op.A = (const double *)ctx->tmp1.p, op.ldA = P.ld, op.a_nan = (const uint8_t *)ctx->tmp2.p;
    }
    return run_dtw_plan(P, op, &ctx->dtw_last);
}

// With the context's mutex held.  Every pointer but `label` is device memory.
static int medoids_locked(wdx_ctx *ctx, const double *dX, int64_t n, int64_t L, const int32_t *label, int64_t n_labels,
                          const int32_t *d_status, int32_t window, double penalty, int64_t *d_medoid, double *d_medoid_cost,
                          int64_t *d_count, double *d_cost, double *d_refs, hipStream_t s) {
    const MedoidKernel kern = L >= 1 ? medoid_kernel(L, window, ctx->knobs.medoid_general, ctx->knobs.no_short_dtw) : MedoidKernel::kGeneral;
    const bool general = kern == MedoidKernel::kGeneral;
    const MedoidPlan P = medoid_plan(label, n, n_labels, L, d_medoid != nullptr, general);
    if (P.rc != WDX_SUCCESS) {
        set_error("%s", P.msg);
        return P.rc;
    }
    if (n > 0 && !dX) {
        set_error("medoids: the fingerprints are required (NULL given)");
        return WDX_ERR_INVALID;
    }
    int rc;
    if ((rc = use_stream(ctx, s))) return rc;
    if ((rc = ctx->medoid_ws.ensure((size_t)P.workspace_bytes))) return rc;
    uint8_t *const ws = (uint8_t *)ctx->medoid_ws.p;
    // the tables, through a page-locked block (the call returns with the copy pending)
    {
        MedoidStage *S = nullptr;
        if ((rc = medoid_stage_block(ctx, (size_t)P.table_bytes, &S))) return rc;
        uint8_t *host = (uint8_t *)S->host;
        memset(host, 0, (size_t)P.table_bytes);
        if (P.rows_padded) memcpy(host + P.off_order, P.order.data(), (size_t)P.rows_padded * sizeof(int32_t));
        memcpy(host + P.off_labels, P.labels.data(), P.labels.size() * sizeof(MedoidLabel));
        const hipError_t e1 = hipMemcpyAsync(ws, host, (size_t)P.table_bytes, hipMemcpyHostToDevice, s);
        const hipError_t e2 = hipEventRecord(S->copied, s);
        WDX_HIP_TRY(e1);
        WDX_HIP_TRY(e2);
    }
    const int32_t *order = (const int32_t *)(ws + P.off_order);
    const MedoidLabel *labels = (const MedoidLabel *)(ws + P.off_labels);
    uint8_t *member = ws + P.off_member;
    double *dense = (double *)(ws + P.off_dense), *padded = (double *)(ws + P.off_padded), *partial = (double *)(ws + P.off_partial);
    float *matrix = (float *)(ws + P.off_matrix);
    const int w_eff = (int)dtw_effective_window(L, window);
    Timed t(ctx, WDX_K_MEDOID, s);
    if (P.rows_padded)
        hipLaunchKernelGGL(tile_gather_kernel<false>, dim3((unsigned)((P.rows_padded + 3) / 4)), dim3(256), 0, s, dX, d_status, order, n,
                           P.rows_padded, (int)L, P.Lpad, kDtwHalo, dense, padded, member);
    if (d_cost && n > 0) hipLaunchKernelGGL(medoid_fill_nan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_cost, n);
    WDX_HIP_TRY(hipGetLastError());
    for (const MedoidPass &Q : P.passes) {
        if (!general) {
            MedoidTileArgs G{dense, padded, P.Lpad, kDtwHalo, member, labels, Q.g0, Q.g1, 0, partial, (int)L, w_eff, penalty * penalty,
                             ctx->knobs.dtw_unfused};
            if (Q.diag1 > Q.diag0) {
                G.tile0 = Q.diag0;
                hipLaunchKernelGGL(medoid_tile_kernel_of(kern, true), dim3((unsigned)(Q.diag1 - Q.diag0)), dim3(64), 0, s, G);
            }
            if (Q.off1 > Q.off0) {
                G.tile0 = Q.off0;
                hipLaunchKernelGGL(medoid_tile_kernel_of(kern, false), dim3((unsigned)(Q.off1 - Q.off0)), dim3(64), 0, s, G);
            }
            WDX_HIP_TRY(hipGetLastError());
        } else {
            for (int32_t g = Q.g0; g < Q.g1; ++g) {
                const MedoidLabel &Lb = P.labels[(size_t)g];
                const int64_t cols = kMedoidChunk * (int64_t)Lb.chunks;
                for (int64_t r0 = 0; r0 < cols; r0 += P.block_rows) {
                    const int64_t rows = std::min(P.block_rows, cols - r0);
                    if ((rc = medoid_matrix_block(ctx, P, Lb, r0, rows, window, penalty, dense, padded, matrix, s))) return rc;
                    const int64_t threads = rows * Lb.chunks;
                    hipLaunchKernelGGL(medoid_chunk_sum_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, matrix, rows, cols,
                                       (int)Lb.chunks, member + Lb.row0, r0, partial + Lb.part0);
                    WDX_HIP_TRY(hipGetLastError());
                }
            }
        }
        const MedoidReduceArgs R{labels, Q.g0, partial, member, order, dX, (int)L, d_medoid, d_medoid_cost, d_count, d_cost, d_refs};
        hipLaunchKernelGGL(medoid_reduce_kernel, dim3((unsigned)(Q.g1 - Q.g0)), dim3(256), 0, s, R);
        WDX_HIP_TRY(hipGetLastError());
    }
    return WDX_SUCCESS;
}

}  // namespace wdx

using namespace wdx;

extern "C" {

int wdx_medoids_device(wdx_ctx *ctx, const double *dX, int64_t n, int64_t L, const int32_t *label, int64_t n_labels,
                       const int32_t *d_status, int32_t window, double penalty, int64_t *d_medoid, double *d_medoid_cost,
                       int64_t *d_count, double *d_cost, double *d_refs, void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    return medoids_locked(ctx, dX, n, L, label, n_labels, d_status, window, penalty, d_medoid, d_medoid_cost, d_count, d_cost, d_refs,
                          (hipStream_t)stream);
}

int wdx_dtw_medoids(wdx_ctx *ctx, const double *X, int64_t n, int64_t L, const int32_t *label, int64_t n_labels,
                    const int32_t *status, int32_t window, double penalty, int64_t *medoid, double *medoid_cost, int64_t *count,
                    double *cost, double *refs) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    {   // the refusals before anything is sized by the arguments
        const MedoidPlan P = medoid_plan(label, n, n_labels, L, medoid != nullptr, false);
        if (P.rc == WDX_SUCCESS && n > 0 && !X) {
            set_error("medoids: the fingerprints are required (NULL given)");
            return WDX_ERR_INVALID;
        }
        if (P.rc != WDX_SUCCESS) {
            set_error("%s", P.msg);
            return P.rc;
        }
    }
    hipStream_t s = ctx->stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const size_t G = (size_t)n_labels, xb = (size_t)(n * L) * sizeof(double), rb = G * (size_t)L * sizeof(double);
    if ((rc = ctx->in0.ensure(xb ? xb : 8))) return rc;
    if (status && (rc = ctx->in1.ensure(n ? (size_t)n * sizeof(int32_t) : 8))) return rc;
    if ((rc = ctx->out0.ensure(G * sizeof(int64_t)))) return rc;
    if (medoid_cost && (rc = ctx->out1.ensure(G * sizeof(double)))) return rc;
    if (count && (rc = ctx->out2.ensure(G * sizeof(int64_t)))) return rc;
    if (cost && (rc = ctx->out3.ensure(n ? (size_t)n * sizeof(double) : 8))) return rc;
    if (refs && (rc = ctx->tmp0.ensure(rb))) return rc;
    StreamDrain drain(s);
    if (n > 0) WDX_HIP_TRY(hipMemcpyAsync(ctx->in0.p, X, xb, hipMemcpyHostToDevice, s));
    if (status && n > 0) WDX_HIP_TRY(hipMemcpyAsync(ctx->in1.p, status, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if ((rc = medoids_locked(ctx, (const double *)ctx->in0.p, n, L, label, n_labels, status ? (const int32_t *)ctx->in1.p : nullptr, window,
                             penalty, (int64_t *)ctx->out0.p, medoid_cost ? (double *)ctx->out1.p : nullptr,
                             count ? (int64_t *)ctx->out2.p : nullptr, cost ? (double *)ctx->out3.p : nullptr,
                             refs ? (double *)ctx->tmp0.p : nullptr, s)))
        return rc;
    WDX_HIP_TRY(hipMemcpyAsync(medoid, ctx->out0.p, G * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (medoid_cost) WDX_HIP_TRY(hipMemcpyAsync(medoid_cost, ctx->out1.p, G * sizeof(double), hipMemcpyDeviceToHost, s));
    if (count) WDX_HIP_TRY(hipMemcpyAsync(count, ctx->out2.p, G * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (cost && n > 0) WDX_HIP_TRY(hipMemcpyAsync(cost, ctx->out3.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (refs) WDX_HIP_TRY(hipMemcpyAsync(refs, ctx->tmp0.p, rb, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    return WDX_SUCCESS;
}

}  // extern "C"
