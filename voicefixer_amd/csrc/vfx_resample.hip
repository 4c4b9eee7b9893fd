// vfx_resample.hip -- band-limited rate conversion of B rows on the device (vfx_resample_rows_f32), of a span of one row's
// outputs from a window of its inputs (vfx_resample_span_f32: the streaming session's converter), and the session's
// overlap cross-fade (vfx_xfade_f32).
//
// The reference resamples every input to 44.1 kHz inside librosa.load (voicefixer/base.py:47-49, soxr "HQ").  The host
// path does that in the decode workers (csrc_host/vfx_resample.c); this kernel evaluates the SAME sum for whole batches
// on the device, so a folder job's workers only decode, and results can leave at another rate:
//
//     y[r][m] = sum_i bank[p][i] * x[r][lo + i],   pos = c + m*down,  kmax = pos / up,  p = pos mod up,  lo = kmax - J + 1
//     m < ny_r = ceil(n_r * up / down);  samples outside [0, n_r) count as zero
//
// bank[p][i] = g[p + (J - 1 - i) * up] (g = up * h, L taps, c = (L - 1) / 2, J = ceil(L / up); taps past L are zero): the
// reversed per-phase layout of vfx_resample.c, built by audio_io.polyphase_bank and uploaded once per device.
//
// One thread per output sample, consecutive outputs in consecutive lanes: a wave reads one window of x (lanes overlap by
// J - down/up samples, L1 / L2 serve the overlap) and up to 64 phase rows of the bank (each lane walks its own row
// ascending, so one cache line serves 16 of its taps).  The 441-phase banks (324 KB) do not fit in LDS and are read
// through L2; DESIGN.md 3.9 has the measured cost.  Positions are 64-bit: c + m*down passes 2^31 at m ~ 4.9 M for down 441.
// Eight partial sums per output (ILP, and an error ~ sqrt(J / 8) roundings instead of sqrt(J)); their fixed order makes
// the result bit-reproducible.
#include "vfx_common.h"

#define RS_THREADS 256
#define RS_NACC 8

__global__ __launch_bounds__(RS_THREADS) void resample_rows_kernel(const float* __restrict__ x, long long x_stride,
                                                                   const int* __restrict__ n_rows, int B,
                                                                   const int* __restrict__ row_index,
                                                                   const float* __restrict__ bank, int J, int up, int down,
                                                                   int c, float* __restrict__ y, long long y_stride,
                                                                   long long ny_max) {
    const int r = row_index ? row_index[blockIdx.y] : (int)blockIdx.y;
    if (r < 0 || r >= B) return;                          // (a bad row number writes nothing)
    const long long n = n_rows[r] > 0 ? n_rows[r] : 0;
    long long ny = (n * up + down - 1) / down;
    if (ny > ny_max) ny = ny_max;                         // never past the caller's row capacity
    const float* xr = x + (long long)r * x_stride;
    float* yr = y + (long long)r * y_stride;
    for (long long m = (long long)blockIdx.x * RS_THREADS + threadIdx.x; m < ny; m += (long long)gridDim.x * RS_THREADS) {
        const long long pos = (long long)c + m * down;    // tap index that meets x[0]
        const long long kmax = pos / up;                  // newest input sample under the filter
        const int p = (int)(pos - kmax * up);
        const long long lo = kmax - J + 1;                // input index under bank[p][0]
        const int i0 = lo < 0 ? (int)(lo < -(long long)J ? J : -lo) : 0;
        const int i1 = lo + J > n ? (int)(n - lo > 0 ? n - lo : 0) : J;
        const float* w = bank + (long long)p * J;
        float acc[RS_NACC];
#pragma unroll
        for (int l = 0; l < RS_NACC; ++l) acc[l] = 0.f;
        int i = i0;
        for (; i + RS_NACC <= i1; i += RS_NACC) {
#pragma unroll
            for (int l = 0; l < RS_NACC; ++l) acc[l] = fmaf(w[i + l], xr[lo + i + l], acc[l]);
        }
        for (; i < i1; ++i) acc[0] = fmaf(w[i], xr[lo + i], acc[0]);    // (<= 7 taps; a variable index would spill acc)
        const float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
        yr[m] = s;
    }
}

extern "C" int vfx_resample_rows_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B,
                                     const int32_t* row_index, int n_index, const float* bank, int J, int up, int down,
                                     int c, float* y, int64_t y_stride, int64_t ny_max, vfx_stream_t stream) {
    if (!x || !n_rows || !bank || !y || B <= 0 || J < 1 || up < 1 || down < 1 || c < 0 || ny_max < 0 || x_stride < 0 ||
        y_stride < ny_max)
        return VFX_EINVAL;
    if (row_index ? (n_index < 0 || n_index > 65535) : (n_index != B || B > 65535)) return VFX_EINVAL;
    if ((long long)up * J > (1LL << 31) || (long long)c >= (long long)up * J) return VFX_EINVAL;
    if (n_index == 0 || ny_max == 0) return VFX_OK;
    long long nbx = (ny_max + RS_THREADS - 1) / RS_THREADS;
    if (nbx > 4096) nbx = 4096;                           // grid-stride beyond: ~16 K waves per row are plenty
    hipLaunchKernelGGL(resample_rows_kernel, dim3((unsigned)nbx, (unsigned)n_index), dim3(RS_THREADS), 0,
                       (hipStream_t)stream, x, (long long)x_stride, (const int*)n_rows, B, (const int*)row_index, bank, J,
                       up, down, c, y, (long long)y_stride, (long long)ny_max);
    VFX_LAUNCHED();
    return vfx_last_error();
}

// Outputs [m0, m1) of ONE row of n_total samples from the window xw[k] = x[g0 + k]: resample_rows_kernel's loop body with
// the row pointer moved.  i0 / i1 -- which tap goes to which of the eight partial sums, which taps fall into the acc[0] tail
// -- come from the row's GLOBAL bounds [0, n_total) exactly as there, never from the window, so output m has the bits the
// whole-row kernel writes for it.  n_total = INT64_MAX (the row's end is not known yet) clips nothing at
// the top; the host check keeps every read inside the window either way.
__global__ __launch_bounds__(RS_THREADS) void resample_span_kernel(const float* __restrict__ xw, long long g0,
                                                                   long long n, const float* __restrict__ bank, int J,
                                                                   int up, int down, int c, long long m0, long long m1,
                                                                   float* __restrict__ y) {
    for (long long m = m0 + (long long)blockIdx.x * RS_THREADS + threadIdx.x; m < m1;
         m += (long long)gridDim.x * RS_THREADS) {
        const long long pos = (long long)c + m * down;
        const long long kmax = pos / up;
        const int p = (int)(pos - kmax * up);
        const long long lo = kmax - J + 1;
        const int i0 = lo < 0 ? (int)(lo < -(long long)J ? J : -lo) : 0;
        const int i1 = lo > n - J ? (int)(n - lo > 0 ? n - lo : 0) : J;    // (lo + J > n, without passing INT64_MAX)
        const float* w = bank + (long long)p * J;
        const long long off = lo - g0;                    // xw[off + i] = x[lo + i]; >= 0 wherever i0 <= i < i1
        float acc[RS_NACC];
#pragma unroll
        for (int l = 0; l < RS_NACC; ++l) acc[l] = 0.f;
        int i = i0;
        for (; i + RS_NACC <= i1; i += RS_NACC) {
#pragma unroll
            for (int l = 0; l < RS_NACC; ++l) acc[l] = fmaf(w[i + l], xw[off + i + l], acc[l]);
        }
        for (; i < i1; ++i) acc[0] = fmaf(w[i], xw[off + i], acc[0]);
        const float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
        y[m - m0] = s;
    }
}

extern "C" int vfx_resample_span_f32(const float* xw, int64_t g0, int64_t wlen, int64_t n_total, const float* bank, int J,
                                     int up, int down, int c, int64_t m0, int64_t m1, float* y, vfx_stream_t stream) {
    if (!xw || !bank || !y || J < 1 || up < 1 || down < 1 || c < 0 || g0 < 0 || wlen < 0 || n_total < 0 || m0 < 0 ||
        m1 < m0)
        return VFX_EINVAL;
    if ((long long)up * J > (1LL << 31) || (long long)c >= (long long)up * J) return VFX_EINVAL;
    if (g0 > INT64_MAX - wlen || m1 > ((1LL << 62) - c) / down) return VFX_EINVAL;     // (c + m*down stays in 64 bits)
    if (m0 == m1) return VFX_OK;
    const long long lo0 = ((long long)c + m0 * down) / up - J + 1;         // oldest sample under the first output's filter
    const long long k1 = ((long long)c + (m1 - 1) * down) / up;            // newest sample under the last output's
    const long long need_lo = lo0 > 0 ? lo0 : 0;
    const long long need_hi = k1 < n_total - 1 ? k1 : n_total - 1;
    if (need_lo < g0 || need_hi >= g0 + wlen) return VFX_EINVAL;
    long long nbx = (m1 - m0 + RS_THREADS - 1) / RS_THREADS;
    if (nbx > 4096) nbx = 4096;
    hipLaunchKernelGGL(resample_span_kernel, dim3((unsigned)nbx), dim3(RS_THREADS), 0, (hipStream_t)stream, xw,
                       (long long)g0, (long long)n_total, bank, J, up, down, c, (long long)m0, (long long)m1, y);
    VFX_LAUNCHED();
    return vfx_last_error();
}

// out[k] = tail[k] * (1 - fade[k]) + head[k] * fade[k]: four separately rounded fp32 operations (contraction is switched off
// for this body; hipcc's default would fuse a product into the sum), the bits of numpy's float32 expression in
// VoiceFixer.restore_stream.  out may be tail or head: every lane reads its own element before it writes it.
__global__ __launch_bounds__(RS_THREADS) void xfade_kernel(const float* tail, const float* head, const float* fade,
                                                           long long n, float* out) {
#pragma clang fp contract(off)
    for (long long k = (long long)blockIdx.x * RS_THREADS + threadIdx.x; k < n; k += (long long)gridDim.x * RS_THREADS) {
        const float f = fade[k];
        const float g = 1.0f - f;
        const float a = tail[k] * g;
        const float b = head[k] * f;
        out[k] = a + b;
    }
}

extern "C" int vfx_xfade_f32(const float* tail, const float* head, const float* fade, int64_t n, float* out,
                             vfx_stream_t stream) {
    if (!tail || !head || !fade || !out || n < 0) return VFX_EINVAL;
    if (n == 0) return VFX_OK;
    long long nbx = (n + RS_THREADS - 1) / RS_THREADS;
    if (nbx > 4096) nbx = 4096;
    hipLaunchKernelGGL(xfade_kernel, dim3((unsigned)nbx), dim3(RS_THREADS), 0, (hipStream_t)stream, tail, head, fade,
                       (long long)n, out);
    VFX_LAUNCHED();
    return vfx_last_error();
}
