// Raw int16 ADC samples -> the calibrated float32 rows the fingerprint chain consumes (include/wdx.h: "raw int16 ADC
// minibatches").  THE CONTRACT, per read r with len_r samples adc, float32 offset_r and scale_r:
//     pa[i] = scale_r * ((float)adc[i] + offset_r)   i < len_r    float32 add, THEN float32 multiply: two roundings,
//                                                                 never one fused operation (__fadd_rn / __fmul_rn)
//     pa[i] = NaN                                    i >= len_r   the NaN tail of the reference's minibatch rows
// (file_proc.py:255-260) -- the decode WRITES it, so that nanmedian and the NaN hand-overs of the chain see the
// same samples as on a float32 minibatch.  NumPy statement: warpdemux_amd.sig_proc.calibrate_adc.
//
// Two pure streaming kernels, one workgroup per read, no LDS, no barrier; they differ in where the int16 samples are:
//   pack_windows_adc_kernel   a page-locked host minibatch read over the bus (49 GB/s, ~1.5 us away): only the adapter
//                             window of every read travels, four 16-byte loads (32 samples) in flight per thread
//   decode_adc_kernel         device memory (the 2-D / flat DMA copy of a pageable or caller-packed minibatch, or a
//                             caller's device buffer: wdx_calibrate_adc_dev)
// 16 bytes in = 8 samples = two 16-byte stores out; rows whose source or destination is not 16-byte aligned (a stride
// that is no multiple of 8) take the element loop, 16 two-byte loads in flight per thread.
//
// A third kernel is the device-to-device form of the window pack, for int16 shards that stay resident (wdx_adc_dev_in):
//   adc_dev_windows_kernel    one WAVE per read, four reads per workgroup: the wave evaluates the window rule itself
//                             (adapter_window, wdx_window.h -- the host loops' own text), decodes the window into the
//                             read's row of the staging block and writes the shifted bounds and the packed length
#include "wdx_common.h"

namespace wdx {

__device__ __forceinline__ float adc_to_pa(int x, float off, float sc) { return __fmul_rn(sc, __fadd_rn((float)x, off)); }

// float32 samples [0, n) of one row: the first nv from s, the rest NaN.  Nothing of s beyond s[nv) is read.
template <int IN_FLIGHT>
__device__ __forceinline__ void adc_decode_row(const int16_t *__restrict__ s, int nv, float off, float sc,
                                               float *__restrict__ d, int n) {
    const float nanv = __builtin_nanf("");
    if ((((uintptr_t)s | (uintptr_t)d) & 15) == 0) {
        const int g_all = n >> 3, g_full = nv >> 3;   // groups of 8 samples: to write, and wholly inside the read
        const int4 *__restrict__ s8 = reinterpret_cast<const int4 *>(s);
        float4 *__restrict__ d4 = reinterpret_cast<float4 *>(d);
        for (int g0 = threadIdx.x; g0 < g_all; g0 += 256 * IN_FLIGHT) {
            int4 v[IN_FLIGHT];
#pragma unroll
            for (int k = 0; k < IN_FLIGHT; ++k) {
                const int g = g0 + 256 * k;
                v[k] = g < g_full ? s8[g] : make_int4(0, 0, 0, 0);
            }
#pragma unroll
            for (int k = 0; k < IN_FLIGHT; ++k) {
                const int g = g0 + 256 * k;
                if (g >= g_all) continue;
                float f[8];
                if (g < g_full) {
                    const int w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        f[2 * j] = adc_to_pa((int)(short)(w[j] & 0xffff), off, sc);
                        f[2 * j + 1] = adc_to_pa(w[j] >> 16, off, sc);
                    }
                } else {   // the group the read ends in, and the NaN tail behind it
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int i = 8 * g + j;
                        f[j] = i < nv ? adc_to_pa(s[i], off, sc) : nanv;
                    }
                }
                d4[2 * g] = make_float4(f[0], f[1], f[2], f[3]);
                d4[2 * g + 1] = make_float4(f[4], f[5], f[6], f[7]);
            }
        }
        const int i = 8 * g_all + threadIdx.x;
        if (i < n) d[i] = i < nv ? adc_to_pa(s[i], off, sc) : nanv;
        return;
    }
    if (nv <= 0) {
        for (int i = threadIdx.x; i < n; i += 256) d[i] = nanv;
        return;
    }
    // (every load is issued, from an index clamped into the read, and selected afterwards: 16 loads in flight per thread,
    // no branch and no wait between them)
    const int last = nv - 1;
    for (int i0 = threadIdx.x; i0 < n; i0 += 256 * 16) {
        int v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = i0 + 256 * k;
            v[k] = (int)s[i < last ? i : last];
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = i0 + 256 * k;
            if (i < n) d[i] = i < nv ? adc_to_pa(v[k], off, sc) : nanv;
        }
    }
}

template <int IN_FLIGHT>
__device__ __forceinline__ void adc_rows_body(const AdcRows &A) {
    const int64_t r = blockIdx.x;
    const int n = A.n_out ? A.n_out[r] : (int)A.dst_stride;
    int nv = A.n_valid[r];
    nv = nv < 0 ? 0 : (nv > n ? n : nv);
    adc_decode_row<IN_FLIGHT>(A.src + (A.src_off ? A.src_off[r] : r * A.src_stride), nv, A.offset[r], A.scale[r],
                              A.dst + (A.dst_off ? A.dst_off[r] : r * A.dst_stride), n);
}

__global__ __launch_bounds__(256) void pack_windows_adc_kernel(const AdcRows A) { adc_rows_body<4>(A); }
__global__ __launch_bounds__(256) void decode_adc_kernel(const AdcRows A) { adc_rows_body<2>(A); }

// 16 bytes of int16 -> 8 calibrated samples
__device__ __forceinline__ void adc_group8(const int4 v, float off, float sc, float *f) {
    const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[2 * j] = adc_to_pa((int)(short)(w[j] & 0xffff), off, sc);
        f[2 * j + 1] = adc_to_pa(w[j] >> 16, off, sc);
    }
}

// Launch shape (guides: 16 bytes per lane is the widest global access; a streaming kernel wants many waves per SIMD and
// needs no LDS): a wave per read keeps the window rule wave-uniform and a 2 000 .. 6 000-sample window is 4 .. 12 groups of 8
// per lane, kGroups of them loaded before the first is converted.  Whole groups are stored -- the row's pitch is a multiple
// of 8 floats (wdx_adc_dev.h) -- so every store is 16 bytes wide and aligned; NaN fills the groups from `valid` on.
constexpr int kAdcDevReadsPerBlock = 4;
__global__ __launch_bounds__(64 * kAdcDevReadsPerBlock) void adc_dev_windows_kernel(const AdcDevWindows A) {
    constexpr int kGroups = 4;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kAdcDevReadsPerBlock + (threadIdx.x >> 6);
    if (i >= A.n) return;
    const int64_t r = A.r0 + i;
    const bool packed = A.row_off != nullptr;
    const int64_t base = packed ? A.row_off[r] : r * A.stride;
    const AdcDevRow R = adc_dev_row(packed, packed ? A.row_off[r + 1] - base : A.stride, A.row_len[r],
                                    packed && A.row_win ? (int64_t)A.row_win[r] : -1);
    const Window w = adc_dev_window(A.a_start[r], A.a_end[r], R, A.ok && !A.ok[r], A.padding, A.max_len);
    if (lane == 0) {
        A.a_start_out[i] = w.a_start;
        A.a_end_out[i] = w.a_end;
        A.row_len_out[i] = (int32_t)w.row;
    }
    if (w.row <= 0) return;   // a dead read, an empty or inverted window: nothing is staged, the bounds are unshifted
    const int16_t *__restrict__ s = A.adc + base + w.first;
    float4 *__restrict__ d4 = reinterpret_cast<float4 *>(A.dst + i * A.pitch);
    const float off = A.offset[r], sc = A.scale[r];
    const float nanv = __builtin_nanf("");
    const int nv = (int)w.valid, g_all = (int)((w.row + 7) >> 3);
    // groups wholly inside the read are one 16-byte load each -- when the window's first sample is 16-byte aligned (a
    // strided shard whose stride is no multiple of 8 is not: its groups take eight 2-byte loads)
    const int g_full = (((uintptr_t)s) & 15) == 0 ? nv >> 3 : 0;
    const int4 *__restrict__ s8 = reinterpret_cast<const int4 *>(s);
    for (int g0 = lane; g0 < g_all; g0 += 64 * kGroups) {
        int4 v[kGroups];
#pragma unroll
        for (int k = 0; k < kGroups; ++k) {
            const int g = g0 + 64 * k;
            v[k] = g < g_full ? s8[g] : make_int4(0, 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < kGroups; ++k) {
            const int g = g0 + 64 * k;
            if (g >= g_all) continue;
            float f[8];
            if (g < g_full) {
                adc_group8(v[k], off, sc, f);
            } else {   // unaligned groups, the group the read ends in, and the NaN tail behind it
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int e = 8 * g + j;
                    f[j] = e < nv ? adc_to_pa(s[e], off, sc) : nanv;
                }
            }
            d4[2 * g] = make_float4(f[0], f[1], f[2], f[3]);
            d4[2 * g + 1] = make_float4(f[4], f[5], f[6], f[7]);
        }
    }
}

int launch_adc_dev_windows(const AdcDevWindows &A, hipStream_t stream) {
    if (A.n <= 0) return WDX_SUCCESS;
    const int64_t blocks = (A.n + kAdcDevReadsPerBlock - 1) / kAdcDevReadsPerBlock;
    if (blocks > INT32_MAX) {
        set_error("int16 device shard: a slice of %lld reads is too large for one launch", (long long)A.n);
        return WDX_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(adc_dev_windows_kernel, dim3((unsigned)blocks), dim3(64 * kAdcDevReadsPerBlock), 0, stream, A);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

int launch_adc_rows(const AdcRows &A, int64_t n_reads, bool over_the_bus, hipStream_t stream) {
    if (n_reads == 0) return WDX_SUCCESS;
    if (over_the_bus)
        hipLaunchKernelGGL(pack_windows_adc_kernel, dim3((unsigned)n_reads), dim3(256), 0, stream, A);
    else
        hipLaunchKernelGGL(decode_adc_kernel, dim3((unsigned)n_reads), dim3(256), 0, stream, A);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

}  // namespace wdx
