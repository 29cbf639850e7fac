// One barycenter step for gfx950 (include/wdx.h: wdx_dba_step_device states the rule; wdx_dba_plan.h what a call does with its host
// labels).
//
// Pre-pass: the rows into the padded layout of the medoids (tile_gather_kernel, dense form only: every label starts on a multiple of 64 rows), the
// centres into rows with a zero halo and one "every sample finite" flag each.
// Align: one LANE per padded row, one wave per chunk of 64 rows -- so a wave belongs to one label and its centre is the uniform
// operand.  The lane runs the cost matrix on the reference's six operations (unfused cells only: a direction comes from a cell's exact
// predecessors), adds each cell's 2-bit direction to the row's words and stores them to the code block with the lanes contiguous;
// then the same lane walks its own words back from (L-1, L-1) and writes its runs, forms s_r[j] in rising i, and hands s_r[j],
// k_r[j] and its cost through LDS in slabs of 32 columns to the lanes that add them over the chunk's members in rising lane order.
//   dba_align_kernel<W, EXACT_W>   effective windows up to 32: the band in registers as dtw_row keeps it (8, 15 exact, 16, 32)
//   dba_align_general_kernel       any window: two rolling rows per lane in a global block, the lanes contiguous
// Reduce: one thread per (label, j) adds the chunk partials in rising chunk order and divides.
#include "wdx_ctx.h"
#include "wdx_dba_plan.h"
#include "wdx_dtw_tile.h"

#include <string.h>

namespace wdx {

enum : int { kDbaDiag = 0, kDbaUp = 1, kDbaLeft = 2 };

// the uniform operand: reads through this address space are invariant loads, which stay on the scalar path whatever the kernel stores
typedef const double __attribute__((address_space(4))) *dba_uniform_ptr;

struct DbaArgs {
    const double *dense;         // (rows_padded, L): a lane's own row
    const double *centres;       // (n_labels, Lpad): the uniform operand, series at +halo
    int64_t Lpad;
    int halo;
    const uint8_t *member;       // [rows_padded]
    const uint8_t *centre_ok;    // [n_labels]
    const int32_t *order;        // [rows_padded]
    const int32_t *chunk_label;  // [chunks]
    int64_t row0, pass_rows;     // first padded row of the launch; lanes the code block is laid out for
    uint64_t *codes;             // [(i * words + h) * pass_rows + lane]
    uint32_t *runs;              // [j * pass_rows + lane]: lo | hi << 16
    double *rolling;             // general route: [(b * (L + 1) + jj) * pass_rows + lane], b = 0, 1
    double *partial;
    int64_t chunks;              // of the call
    int L, w, words;
    double p2;
    double *cost;                // (n) or null
    int32_t *out_runs;           // (n, L, 2) or null
};

__device__ __forceinline__ int64_t dba_part_S(const DbaArgs &A, int64_t chunk, int j) { return chunk * A.L + j; }
__device__ __forceinline__ int64_t dba_part_K(const DbaArgs &A, int64_t chunk, int j) { return (A.chunks + chunk) * A.L + j; }
__device__ __forceinline__ int64_t dba_part_cost(const DbaArgs &A, int64_t chunk) { return 2 * A.chunks * A.L + chunk; }
__device__ __forceinline__ int64_t dba_part_members(const DbaArgs &A, int64_t chunk) { return 2 * A.chunks * A.L + A.chunks + chunk; }

__device__ __forceinline__ int dba_direction(double diag, double up, double left, double t) {
    return diag <= t ? kDbaDiag : (up <= left ? kDbaUp : kDbaLeft);
}

// ---- pre-pass ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void dba_centres_kernel(const double *__restrict__ C, int L, int64_t Lpad, int halo,
                                                         double *__restrict__ padded, uint8_t *__restrict__ ok) {
    const int64_t g = blockIdx.x;
    const int lane = threadIdx.x;
    bool bad = false;
    for (int64_t c = lane; c < Lpad; c += 64) {
        const int64_t s = c - halo;
        const bool in = s >= 0 && s < L;
        const double v = in ? C[g * L + s] : 0.0;
        padded[g * Lpad + c] = v;
        bad |= in && !(v - v == 0.0);   // NaN or an infinity
    }
    const unsigned long long any_bad = __ballot(bad);
    if (lane == 0) ok[g] = any_bad ? 0 : 1;
}

__global__ __launch_bounds__(256) void dba_fill_kernel(double *__restrict__ cost, int64_t n, int32_t *__restrict__ runs, int64_t n_runs) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cost && r < n) cost[r] = __builtin_nan("");
    if (runs && r < n_runs) runs[r] = -1;
}

// ---- what both align kernels do behind their cost matrix ---------------------------------------------------------------------
struct DbaLane {
    int lane;
    int64_t lrow, chunk;          // lane of the launch; chunk of the call
    int32_t g;
    bool mem;
    unsigned long long mask;      // the chunk's members
    const double *xp;
};

__device__ __forceinline__ DbaLane dba_lane(const DbaArgs &A) {
    DbaLane T;
    T.lane = threadIdx.x;
    T.lrow = (int64_t)blockIdx.x * kMedoidChunk + T.lane;
    T.chunk = A.row0 / kMedoidChunk + blockIdx.x;
    T.g = __builtin_amdgcn_readfirstlane(A.chunk_label[T.chunk]);
    T.mem = A.member[A.row0 + T.lrow] != 0 && A.centre_ok[T.g] != 0;
    T.mask = __ballot(T.mem);
    T.xp = A.dense + (A.row0 + T.lrow) * (int64_t)A.L;
    return T;
}

// a chunk without a member of a busy label: its partials are zeros (the block is reused from call to call)
__device__ __forceinline__ void dba_idle_chunk(const DbaArgs &A, const DbaLane &T) {
    for (int j = T.lane; j < A.L; j += 64) {
        A.partial[dba_part_S(A, T.chunk, j)] = 0.0;
        ((int64_t *)A.partial)[dba_part_K(A, T.chunk, j)] = 0;
    }
    if (T.lane == 0) {
        A.partial[dba_part_cost(A, T.chunk)] = 0.0;
        ((int64_t *)A.partial)[dba_part_members(A, T.chunk)] = 0;
    }
}

// the lane's path back from (L-1, L-1) by its own direction words: runs[j] = lo | hi << 16.  Whatever the words hold, i and j stay
// inside the matrix and every step lowers i + j.
__device__ __forceinline__ void dba_walk(const DbaArgs &A, const DbaLane &T) {
    const int L = A.L, w = A.w, words = A.words;
    int i = L - 1, j = L - 1, hi = L - 1;
    for (;;) {
        if (i == 0 && j == 0) {
            A.runs[T.lrow] = (uint32_t)hi << 16;
            break;
        }
        const int k = j - max(0, i - (w - 1));
        int code = kDbaDiag;
        if (k >= 0 && k < 32 * words) {
            const uint64_t word = A.codes[((int64_t)i * words + (k >> 5)) * A.pass_rows + T.lrow];
            code = (int)((word >> (2 * (k & 31))) & 3ull);
        }
        if (i == 0) code = kDbaLeft;
        else if (j == 0) code = kDbaUp;
        if (code == kDbaUp) {
            --i;
        } else {   // column j is complete: its lowest row is i
            A.runs[(int64_t)j * A.pass_rows + T.lrow] = (uint32_t)i | ((uint32_t)hi << 16);
            --j;
            if (code == kDbaDiag) --i;
            hi = i;
        }
    }
}

// s_r[j] in rising i, the hand-over through LDS in slabs of kDbaSlab columns, the chunk's partial sums, the lane's own outputs
__device__ __forceinline__ void dba_sums(const DbaArgs &A, const DbaLane &T, const double cost, double *hand_s, int32_t *hand_k) {
    const int L = A.L, lane = T.lane;
    const int64_t src = T.mem ? (int64_t)A.order[A.row0 + T.lrow] : -1;
    for (int j0 = 0; j0 < L; j0 += kDbaSlab) {
        const int ncol = min(kDbaSlab, L - j0);
        if (T.mem) {
            for (int jj = 0; jj < ncol; ++jj) {
                const uint32_t run = A.runs[(int64_t)(j0 + jj) * A.pass_rows + T.lrow];
                const int lo = (int)(run & 0xffffu), hi = (int)(run >> 16);
                double s = 0.0;
                for (int i = lo; i <= hi; ++i) s += T.xp[i];
                hand_s[jj * 65 + lane] = s;
                hand_k[jj * 65 + lane] = hi - lo + 1;
                if (A.out_runs) {
                    A.out_runs[(src * L + j0 + jj) * 2] = lo;
                    A.out_runs[(src * L + j0 + jj) * 2 + 1] = hi;
                }
            }
        }
        medoid_wave_sync();
        if (lane < ncol) {   // lane l owns column j0 + l: the chunk's members in rising lane order
            double S = 0.0;
            int64_t K = 0;
            for (int a = 0; a < 64; ++a)
                if ((T.mask >> a) & 1ull) {
                    S += hand_s[lane * 65 + a];
                    K += hand_k[lane * 65 + a];
                }
            A.partial[dba_part_S(A, T.chunk, j0 + lane)] = S;
            ((int64_t *)A.partial)[dba_part_K(A, T.chunk, j0 + lane)] = K;
        }
        medoid_wave_sync();
    }
    hand_s[lane] = cost;
    medoid_wave_sync();
    if (lane == 0) {
        double S = 0.0;
        for (int a = 0; a < 64; ++a)
            if ((T.mask >> a) & 1ull) S += hand_s[a];
        A.partial[dba_part_cost(A, T.chunk)] = S;
        ((int64_t *)A.partial)[dba_part_members(A, T.chunk)] = __popcll(T.mask);
    }
    if (T.mem && A.cost) A.cost[src] = cost;
}

// ---- the band route ----------------------------------------------------------------------------------------------------------
// The band cell c of row i is column j = i - (W - 1) + c, as in dtw_row; cells outside the window or the matrix are +inf.  EXACT_W
// (w == W): the window's limits are the band's own.  A row's direction bits are collected at 2 c and shifted down to the row's first
// cell inside the band before they are stored (wdx_dba_plan.h: words).
template <int W, bool EXACT_W>
__global__ __launch_bounds__(64) void dba_align_kernel(const DbaArgs A) {
    constexpr int B = 2 * W - 1;
    constexpr bool TWO = 2 * B > 64;
    __shared__ double hand_s[kDbaSlab * 65];
    __shared__ int32_t hand_k[kDbaSlab * 65];
    const DbaLane T = dba_lane(A);
    if (T.mask == 0ull) {   // (uniform)
        dba_idle_chunk(A, T);
        return;
    }
    const int L = A.L, w = EXACT_W ? W : A.w, words = A.words;
    const double p2 = A.p2;
    const dba_uniform_ptr y = (dba_uniform_ptr)(A.centres + (int64_t)T.g * A.Lpad + (A.halo - (W - 1)));
    double r[B];
#pragma unroll
    for (int c = 0; c < B; ++c) r[c] = WDX_INF;
    r[W - 1] = 0.0;
    #pragma nounroll
    for (int i = 0; i < L; ++i) {
        const double x = T.xp[i];
        const dba_uniform_ptr yi = y + i;
        const int jbase = i - (W - 1), jlo = max(0, i - (w - 1)), jhi = min(L - 1, i + (w - 1));
        uint64_t w0 = 0, w1 = 0;
        double left = WDX_INF;
#pragma unroll
        for (int c = 0; c < B; ++c) {
            const double d = x - yi[c];
            const double up = (c + 1 < B) ? r[c + 1 < B ? c + 1 : 0] : WDX_INF;
            const double diag = r[c];
            const double t = (c == 0 ? up : min_f64(up, left)) + p2;   // left of the first band cell is +inf
            double v = d * d + min_f64(t, diag);
            int code = dba_direction(diag, up, left, t);
            const int j = jbase + c;
            v = (j < jlo || j > jhi) ? WDX_INF : v;
            code = i == 0 ? (int)kDbaLeft : code;
            code = j == 0 ? (int)kDbaUp : code;
            if (2 * c < 64) w0 |= (uint64_t)code << ((2 * c) & 63);
            else w1 |= (uint64_t)code << ((2 * c) & 63);
            r[c] = v;
            left = v;
            // the centre in pieces of 8 cells: left alone, the scheduler gathers a whole row's loads (58 to 62 scalar registers at
            // W 15 / 16, beside the kernel's arguments more than the file holds) and every cell's difference in front of the chain
            if (c % 8 == 7) __builtin_amdgcn_sched_barrier(0);
        }
        const int sh = 2 * (jlo - jbase);   // 0 .. 2 (W - 1) < 64
        uint64_t s0 = w0 >> sh;
        if (TWO) {
            if (sh) s0 |= w1 << (64 - sh);
            w1 >>= sh;
        }
        A.codes[((int64_t)i * words) * A.pass_rows + T.lrow] = s0;
        if (TWO && words > 1) A.codes[((int64_t)i * words + 1) * A.pass_rows + T.lrow] = w1;
    }
    const double cost = r[W - 1];
    if (T.mem) dba_walk(A, T);
    dba_sums(A, T, cost, hand_s, hand_k);
}

// ---- the general route -------------------------------------------------------------------------------------------------------
// D[i][*] and D[i+1][*] per lane in the rolling block; the row in hand sets the entry left of its first cell and the one behind its last
// cell to +inf, which is all the next row reads outside this row's cells.
__global__ __launch_bounds__(64) void dba_align_general_kernel(const DbaArgs A) {
    __shared__ double hand_s[kDbaSlab * 65];
    __shared__ int32_t hand_k[kDbaSlab * 65];
    const DbaLane T = dba_lane(A);
    if (T.mask == 0ull) {   // (uniform)
        dba_idle_chunk(A, T);
        return;
    }
    const int L = A.L, w = A.w, words = A.words;
    const double p2 = A.p2;
    const dba_uniform_ptr y = (dba_uniform_ptr)(A.centres + (int64_t)T.g * A.Lpad + A.halo);
    const int64_t ld = A.pass_rows;
    double *prev = A.rolling + T.lrow, *cur = prev + (int64_t)(L + 1) * ld;
    for (int jj = 0; jj <= L; ++jj) prev[jj * ld] = jj == 0 ? 0.0 : WDX_INF;
    for (int i = 0; i < L; ++i) {
        const double x = T.xp[i];
        const int jlo = max(0, i - (w - 1)), jhi = min(L - 1, i + (w - 1));
        double left = WDX_INF, diag = prev[jlo * ld];
        cur[jlo * ld] = WDX_INF;
        uint64_t word = 0;
        for (int j = jlo; j <= jhi; ++j) {
            const double up = prev[(int64_t)(j + 1) * ld];
            const double d = x - y[j];
            const double t = min_f64(up, left) + p2;
            const double v = d * d + min_f64(t, diag);
            int code = dba_direction(diag, up, left, t);
            code = i == 0 ? (int)kDbaLeft : code;
            code = j == 0 ? (int)kDbaUp : code;
            const int k = j - jlo;
            word |= (uint64_t)code << (2 * (k & 31));
            if ((k & 31) == 31 || j == jhi) {
                A.codes[((int64_t)i * words + (k >> 5)) * ld + T.lrow] = word;
                word = 0;
            }
            cur[(int64_t)(j + 1) * ld] = v;
            diag = up;
            left = v;
        }
        if (jhi + 2 <= L) cur[(int64_t)(jhi + 2) * ld] = WDX_INF;
        double *const sw = prev;
        prev = cur, cur = sw;
    }
    const double cost = prev[(int64_t)L * ld];
    if (T.mem) dba_walk(A, T);
    dba_sums(A, T, cost, hand_s, hand_k);
}

using DbaAlignKernel = void (*)(const DbaArgs);
static DbaAlignKernel dba_align_kernel_of(DbaKernel k) {
    switch (k) {
    case DbaKernel::kBand8: return dba_align_kernel<8, false>;
    case DbaKernel::kBand15: return dba_align_kernel<15, true>;
    case DbaKernel::kBand16: return dba_align_kernel<16, false>;
    case DbaKernel::kBand32: return dba_align_kernel<32, false>;
    default: return dba_align_general_kernel;
    }
}

// ---- reduce: one thread per (label, j) ---------------------------------------------------------------------------------------
struct DbaReduceArgs {
    const MedoidLabel *labels;
    const double *partial;
    int64_t chunks, n_labels;
    int L;
    double *centres;
    int64_t *count;
    double *inertia;
};
__global__ __launch_bounds__(256) void dba_reduce_kernel(const DbaReduceArgs R) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R.n_labels * R.L) return;
    const int64_t g = idx / R.L;
    const int j = (int)(idx % R.L);
    const MedoidLabel Lb = R.labels[g];
    const int64_t c0 = Lb.row0 / kMedoidChunk;
    const int64_t *const ipart = (const int64_t *)R.partial;
    double T = 0.0, I = 0.0;
    int64_t K = 0, members = 0;
    for (int64_t c = c0; c < c0 + Lb.chunks; ++c) {   // rising chunk order
        T += R.partial[c * R.L + j];
        K += ipart[(R.chunks + c) * R.L + j];
        I += R.partial[2 * R.chunks * R.L + c];
        members += ipart[2 * R.chunks * R.L + R.chunks + c];
    }
    const bool idle = members == 0;   // (the members of a label whose centre is not finite were not counted)
    R.centres[idx] = idle ? __builtin_nan("") : T / (double)K;
    if (j == 0) {
        if (R.count) R.count[g] = members;
        if (R.inertia) R.inertia[g] = idle ? __builtin_nan("") : I;
    }
}

// ---- the call ------------------------------------------------------------------------------------------------------------------
// With the context's mutex held.  Every pointer but `label` is device memory.
static int dba_locked(wdx_ctx *ctx, const double *dX, int64_t n, int64_t L, const int32_t *label, int64_t n_labels,
                      const int32_t *d_status, const double *d_centres, int32_t window, double penalty, double *d_new, int64_t *d_count,
                      double *d_inertia, double *d_cost, int32_t *d_runs, hipStream_t s) {
    const DbaPlan P = dba_plan(label, n, n_labels, L, window, d_new != nullptr, d_centres != nullptr, ctx->knobs.dba_general);
    if (P.rc != WDX_SUCCESS) {
        set_error("%s", P.msg);
        return P.rc;
    }
    if (n > 0 && !dX) {
        set_error("dba: the fingerprints are required (NULL given)");
        return WDX_ERR_INVALID;
    }
    int rc;
    if ((rc = use_stream(ctx, s))) return rc;
    if ((rc = ctx->dba_ws.ensure((size_t)P.workspace_bytes))) return rc;
    uint8_t *const ws = (uint8_t *)ctx->dba_ws.p;
    {   // the tables, through a page-locked block (the call returns with the copy pending)
        MedoidStage *S = nullptr;
        if ((rc = medoid_stage_block(ctx, (size_t)P.table_bytes, &S))) return rc;
        uint8_t *host = (uint8_t *)S->host;
        memset(host, 0, (size_t)P.table_bytes);
        if (P.rows_padded) {
            memcpy(host + P.off_order, P.order.data(), (size_t)P.rows_padded * sizeof(int32_t));
            memcpy(host + P.off_chunk_label, P.chunk_label.data(), (size_t)P.chunks * sizeof(int32_t));
        }
        memcpy(host + P.off_labels, P.labels.data(), P.labels.size() * sizeof(MedoidLabel));
        const hipError_t e1 = hipMemcpyAsync(ws, host, (size_t)P.table_bytes, hipMemcpyHostToDevice, s);
        const hipError_t e2 = hipEventRecord(S->copied, s);
        WDX_HIP_TRY(e1);
        WDX_HIP_TRY(e2);
    }
    const int32_t *order = (const int32_t *)(ws + P.off_order);
    uint8_t *member = ws + P.off_member, *centre_ok = ws + P.off_centre_ok;
    double *dense = (double *)(ws + P.off_dense), *centres = (double *)(ws + P.off_centres);
    double *partial = (double *)(ws + P.off_partial);
    if (P.rows_padded)
        hipLaunchKernelGGL((tile_gather_kernel<false, false>), dim3((unsigned)((P.rows_padded + 3) / 4)), dim3(256), 0, s, dX, d_status, order, n,
                           P.rows_padded, (int)L, P.Lpad, kDtwHalo, dense, (double *)nullptr, member);
    hipLaunchKernelGGL(dba_centres_kernel, dim3((unsigned)n_labels), dim3(64), 0, s, d_centres, (int)L, P.Lpad, kDtwHalo, centres, centre_ok);
    const int64_t n_runs = d_runs ? n * L * 2 : 0, fill = std::max(d_cost ? n : 0, n_runs);
    if (fill > 0) hipLaunchKernelGGL(dba_fill_kernel, dim3((unsigned)((fill + 255) / 256)), dim3(256), 0, s, d_cost, n, d_runs, n_runs);
    WDX_HIP_TRY(hipGetLastError());
    DbaArgs A{dense, centres, P.Lpad, kDtwHalo, member, centre_ok, order, (const int32_t *)(ws + P.off_chunk_label), 0, P.pass_rows,
              (uint64_t *)(ws + P.off_codes), (uint32_t *)(ws + P.off_runs), (double *)(ws + P.off_rolling), partial, P.chunks, (int)L,
              (int)P.w, (int)P.words, penalty * penalty, d_cost, d_runs};
    for (const DbaPass &Q : P.passes) {
        A.row0 = Q.row0;
        hipLaunchKernelGGL(dba_align_kernel_of(P.kernel), dim3((unsigned)(Q.rows / kMedoidChunk)), dim3(64), 0, s, A);
        WDX_HIP_TRY(hipGetLastError());
    }
    const DbaReduceArgs R{(const MedoidLabel *)(ws + P.off_labels), partial, P.chunks, n_labels, (int)L, d_new, d_count, d_inertia};
    hipLaunchKernelGGL(dba_reduce_kernel, dim3((unsigned)((n_labels * L + 255) / 256)), dim3(256), 0, s, R);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

}  // namespace wdx

using namespace wdx;

extern "C" {

int wdx_dba_step_device(wdx_ctx *ctx, const double *dX, int64_t n, int64_t L, const int32_t *label, int64_t n_labels,
                        const int32_t *d_status, const double *d_centres, int32_t window, double penalty, double *d_new,
                        int64_t *d_count, double *d_inertia, double *d_cost, int32_t *d_runs, void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    return dba_locked(ctx, dX, n, L, label, n_labels, d_status, d_centres, window, penalty, d_new, d_count, d_inertia, d_cost, d_runs,
                      (hipStream_t)stream);
}

int wdx_dtw_dba_step(wdx_ctx *ctx, const double *X, int64_t n, int64_t L, const int32_t *label, int64_t n_labels,
                     const int32_t *status, const double *centres, int32_t window, double penalty, double *new_centres,
                     int64_t *count, double *inertia, double *cost, int32_t *runs) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    {   // the refusals before anything is sized by the arguments
        char msg[192] = {0};
        const int refused = dba_refusal(label, n, n_labels, L, new_centres != nullptr, centres != nullptr, msg);
        if (refused != WDX_SUCCESS) {
            set_error("%s", msg);
            return refused;
        }
        if (n > 0 && !X) {
            set_error("dba: the fingerprints are required (NULL given)");
            return WDX_ERR_INVALID;
        }
    }
    hipStream_t s = ctx->stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const size_t G = (size_t)n_labels, xb = (size_t)(n * L) * sizeof(double), cb = G * (size_t)L * sizeof(double);
    const size_t rb = (size_t)(n * L) * 2 * sizeof(int32_t);
    if ((rc = ctx->in0.ensure(xb ? xb : 8))) return rc;
    if (status && (rc = ctx->in1.ensure(n ? (size_t)n * sizeof(int32_t) : 8))) return rc;
    if ((rc = ctx->in2.ensure(cb))) return rc;
    if ((rc = ctx->out0.ensure(cb))) return rc;
    if (count && (rc = ctx->out1.ensure(G * sizeof(int64_t)))) return rc;
    if (inertia && (rc = ctx->out2.ensure(G * sizeof(double)))) return rc;
    if (cost && (rc = ctx->out3.ensure(n ? (size_t)n * sizeof(double) : 8))) return rc;
    if (runs && (rc = ctx->tmp0.ensure(rb ? rb : 8))) return rc;
    StreamDrain drain(s);
    if (n > 0) WDX_HIP_TRY(hipMemcpyAsync(ctx->in0.p, X, xb, hipMemcpyHostToDevice, s));
    if (status && n > 0) WDX_HIP_TRY(hipMemcpyAsync(ctx->in1.p, status, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    WDX_HIP_TRY(hipMemcpyAsync(ctx->in2.p, centres, cb, hipMemcpyHostToDevice, s));
    if ((rc = dba_locked(ctx, (const double *)ctx->in0.p, n, L, label, n_labels, status ? (const int32_t *)ctx->in1.p : nullptr,
                         (const double *)ctx->in2.p, window, penalty, (double *)ctx->out0.p, count ? (int64_t *)ctx->out1.p : nullptr,
                         inertia ? (double *)ctx->out2.p : nullptr, cost ? (double *)ctx->out3.p : nullptr,
                         runs ? (int32_t *)ctx->tmp0.p : nullptr, s)))
        return rc;
    WDX_HIP_TRY(hipMemcpyAsync(new_centres, ctx->out0.p, cb, hipMemcpyDeviceToHost, s));
    if (count) WDX_HIP_TRY(hipMemcpyAsync(count, ctx->out1.p, G * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (inertia) WDX_HIP_TRY(hipMemcpyAsync(inertia, ctx->out2.p, G * sizeof(double), hipMemcpyDeviceToHost, s));
    if (cost && n > 0) WDX_HIP_TRY(hipMemcpyAsync(cost, ctx->out3.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (runs && n > 0) WDX_HIP_TRY(hipMemcpyAsync(runs, ctx->tmp0.p, rb, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    return WDX_SUCCESS;
}

}  // extern "C"
