// vfx_loudness.hip -- integrated loudness (ITU-R BS.1770-4, one channel) of B rows and the gain that normalises it
// (vfx_loudness_rows_f32).  Definition, chunk scan and measured cost: DESIGN.md 3.10.
//
//   K-weighting: two cascaded biquads (shelf, then high-pass), transposed direct form II, fp32.  Quarter q = sum of the
//   squared K-weighted samples [q*hop, (q+1)*hop) (fp64); block j = quarters j..j+3, z_j = sum / (4 hop),
//   l_j = -0.691 + 10 log10 z_j; absolute gate l_j > -70, relative gate l_j > Gr = mean-loudness - 10; L = -0.691 +
//   10 log10(mean z of the blocks that pass both); no block: L = -inf.  g = min(10^((T - L)/20), 10^(C/20) / max|x|)
//   (1 when L = -inf), out = float(g) * x.
//
// An IIR filter over a long row cannot run on one lane, so a row is cut into chunks of S samples (S a multiple of 32, S <= hop:
// a chunk straddles at most one quarter boundary), 256 chunks to a workgroup ("span"), and the state is carried by an affine
// scan.  With s = (z1, z2 of the shelf, z1, z2 of the high-pass) and A the 4x4 zero-input transition of one sample, the
// start state of chunk k + 1 is s_{k+1} = M s_k + e_k, M = A^S, e_k = the end state of chunk k filtered from zero.  The
// host passes M^(2^i), i < 16, in float64.
//   1. lk_chunk_kernel: every lane filters its chunk from zero (the span staged through LDS, 32 samples of every chunk at a
//      time, 16-byte loads), records e_k and folds max|x| of the span; a Hillis-Steele scan of the 256 (M, e_k) pairs in LDS
//      (fp64, 8 steps with M^(2^i)) gives every chunk's start state as if the span started from zero, and the span's
//      aggregate E_w (its end state from zero).
//   2. lk_filter_kernel: span w's true start state is sum_{j < w} Mspan^(w-1-j) E_j, Mspan = M^256; every workgroup evaluates
//      it itself from the aggregates of the `lookback` spans before it (terms further back are below 2^-80 of the state:
//      the high-pass pole contracts the state by ~0.3 per chunk, by ~1e-130 per span; the host picks `lookback`), adds
//      M^c times it to chunk c's span-relative start state, filters the chunk again from that state and accumulates y^2
//      (fp64) into the part in the quarter of its first sample and the part in the next one.
//   3. lk_gate_kernel: one workgroup per row: quarter sums from the chunk parts (fixed order), block energies, both gates
//      (fixed-order LDS reductions: bit-reproducible), L, the row peak, the gain -> result[r] = {L, g, peak}.
//   4. lk_apply_kernel: out = float(g) * x over each row's own length (float4 where aligned); not launched to measure only.
// Nothing is written past a row's length; at most 4 launches per call, none of them waits for the host.
#include <cmath>
#include "vfx_common.h"

#define LK_T 256                  // lanes (= chunks) per workgroup
#define LK_P 32                   // samples of every chunk staged per step
#define LK_LDSW (LK_P + 1)        // padded LDS row: lane c reads column i of row c, conflict-free
#define LK_NPOW 16                // M^(2^i), i < 16
#define LK_ALIGN 256

struct lk_coef {
    float b0s, b1s, b2s, a1s, a2s;    // shelf
    float b0h, b1h, b2h, a1h, a2h;    // high-pass
};

struct lk_ws {                    // per-row slices of the workspace
    float4* local;                // [B][nchunks]  start state of every chunk relative to its span
    double2* parts;               // [B][nchunks]  y^2 in the quarter of the chunk's first sample, in the next one
    double4* agg;                 // [B][nspans]   end state of every span filtered from zero
    float* peak;                  // [B][nspans]   max |x| of every span
    double* z;                    // [B][nblk]     block energies
    long long nchunks, nspans, nblk;
};

static inline size_t lk_round(size_t b) { return (b + LK_ALIGN - 1) / LK_ALIGN * LK_ALIGN; }

static void lk_layout(int B, long long n_max, int hop, int S, size_t* total, lk_ws* w, char* base) {
    const long long nspans = n_max > 0 ? (n_max + (long long)LK_T * S - 1) / ((long long)LK_T * S) : 1;
    const long long nchunks = nspans * LK_T;
    const long long nq = n_max / hop;
    const long long nblk = nq > 3 ? nq - 3 : 1;
    size_t off = 0;
    const size_t o_local = off; off += lk_round((size_t)B * nchunks * sizeof(float4));
    const size_t o_parts = off; off += lk_round((size_t)B * nchunks * sizeof(double2));
    const size_t o_agg = off;   off += lk_round((size_t)B * nspans * sizeof(double4));
    const size_t o_peak = off;  off += lk_round((size_t)B * nspans * sizeof(float));
    const size_t o_z = off;     off += lk_round((size_t)B * nblk * sizeof(double));
    *total = off;
    if (w) {
        w->local = (float4*)(base + o_local);
        w->parts = (double2*)(base + o_parts);
        w->agg = (double4*)(base + o_agg);
        w->peak = (float*)(base + o_peak);
        w->z = (double*)(base + o_z);
        w->nchunks = nchunks;
        w->nspans = nspans;
        w->nblk = nblk;
    }
}

// v <- m v (m row-major 4x4, float64)
__device__ __forceinline__ void lk_mv(const double* __restrict__ m, double v[4]) {
    double o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = m[4 * i] * v[0] + m[4 * i + 1] * v[1] + m[4 * i + 2] * v[2] + m[4 * i + 3] * v[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = o[i];
}

// one sample through both biquads (transposed direct form II); returns the K-weighted sample
__device__ __forceinline__ float lk_step(const lk_coef& k, float x, float s[4]) {
    const float ys = fmaf(k.b0s, x, s[0]);
    s[0] = fmaf(k.b1s, x, fmaf(-k.a1s, ys, s[1]));
    s[1] = fmaf(k.b2s, x, -k.a2s * ys);
    const float yh = fmaf(k.b0h, ys, s[2]);
    s[2] = fmaf(k.b1h, ys, fmaf(-k.a1h, yh, s[3]));
    s[3] = fmaf(k.b2h, ys, -k.a2h * yh);
    return yh;
}

// Stage samples [p*LK_P, (p+1)*LK_P) of every chunk of the span into tile[chunk][LK_LDSW]; samples at or past n read as 0.
// Returns max |x| of what this lane loaded.
template <bool VEC>
__device__ __forceinline__ float lk_stage(const float* __restrict__ xr, long long span0, int S, int p, long long n,
                                          float* tile) {
    float pk = 0.f;
#pragma unroll
    for (int i = 0; i < LK_T * LK_P / 4 / LK_T; ++i) {
        const int f = threadIdx.x + i * LK_T;             // float4 slot: chunk f / 8, quad f % 8
        const int c = f / (LK_P / 4), q = f % (LK_P / 4);
        const long long idx = span0 + (long long)c * S + p * LK_P + 4 * q;
        float v[4];
        if (VEC && idx + 3 < n) {
            const float4 u = *reinterpret_cast<const float4*>(xr + idx);
            v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = idx + e < n ? xr[idx + e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            tile[c * LK_LDSW + 4 * q + e] = v[e];
            pk = fmaxf(pk, fabsf(v[e]));
        }
    }
    return pk;
}

template <bool VEC>
__global__ __launch_bounds__(LK_T) void lk_chunk_kernel(const float* __restrict__ x, long long x_stride,
                                                        const int* __restrict__ n_rows, long long n_max, lk_coef k,
                                                        const double* __restrict__ mpow, int S, lk_ws w) {
    __shared__ float tile[LK_T * LK_LDSW];
    __shared__ double sc[LK_T][4];
    __shared__ float red[LK_T];
    const int r = blockIdx.y, c = threadIdx.x;
    long long n = n_rows[r];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    const long long span0 = (long long)blockIdx.x * LK_T * S;
    if (span0 >= n) return;                               // (uniform over the workgroup)
    const float* xr = x + (long long)r * x_stride;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    float pk = 0.f;
    for (int p = 0; p < S / LK_P; ++p) {
        __syncthreads();
        pk = fmaxf(pk, lk_stage<VEC>(xr, span0, S, p, n, tile));
        __syncthreads();
#pragma unroll 8
        for (int i = 0; i < LK_P; ++i) lk_step(k, tile[c * LK_LDSW + i], s);
    }
    // inclusive scan of v_c = e_c: after step i, v_c = sum_{j in (c - 2^(i+1), c]} M^(c-j) e_j
    double v[4] = {s[0], s[1], s[2], s[3]};
    for (int i = 0; i < 8; ++i) {
        const int d = 1 << i;
#pragma unroll
        for (int e = 0; e < 4; ++e) sc[c][e] = v[e];
        __syncthreads();
        if (c >= d) {
            double u[4] = {sc[c - d][0], sc[c - d][1], sc[c - d][2], sc[c - d][3]};
            lk_mv(mpow + 16 * i, u);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += u[e];
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sc[c][e] = v[e];
    red[c] = pk;
    __syncthreads();
    const long long chunk = (long long)blockIdx.x * LK_T + c;
    const float4 st = c == 0 ? make_float4(0.f, 0.f, 0.f, 0.f)
                             : make_float4((float)sc[c - 1][0], (float)sc[c - 1][1], (float)sc[c - 1][2], (float)sc[c - 1][3]);
    w.local[(long long)r * w.nchunks + chunk] = st;
    for (int h = LK_T / 2; h > 0; h >>= 1) {
        if (c < h) red[c] = fmaxf(red[c], red[c + h]);
        __syncthreads();
    }
    if (c == LK_T - 1) w.agg[(long long)r * w.nspans + blockIdx.x] = make_double4(v[0], v[1], v[2], v[3]);
    if (c == 0) w.peak[(long long)r * w.nspans + blockIdx.x] = red[0];
}

template <bool VEC>
__global__ __launch_bounds__(LK_T) void lk_filter_kernel(const float* __restrict__ x, long long x_stride,
                                                         const int* __restrict__ n_rows, long long n_max, lk_coef k,
                                                         const double* __restrict__ mpow, int S, int hop, int lookback,
                                                         lk_ws w) {
    __shared__ float tile[LK_T * LK_LDSW];
    __shared__ double sc[LK_T][4];
    __shared__ double carry[4];
    const int r = blockIdx.y, c = threadIdx.x;
    long long n = n_rows[r];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    const long long span0 = (long long)blockIdx.x * LK_T * S;
    if (span0 >= n) return;
    const float* xr = x + (long long)r * x_stride;
    // carry into this span: sum over the `lookback` spans before it of Mspan^(w-1-j) E_j (lane t: j = w-1-t)
    {
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        const long long j = (long long)blockIdx.x - 1 - c;
        if (c < lookback && j >= 0) {
            const double4 a = w.agg[(long long)r * w.nspans + j];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
            for (int b = 0; (c >> b) != 0; ++b)
                if ((c >> b) & 1) lk_mv(mpow + 16 * (8 + b), v);     // Mspan^(2^b) = M^(2^(8+b))
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) sc[c][e] = v[e];
        __syncthreads();
        if (c < 4) {
            double acc = 0.0;
            for (int t = 0; t < lookback; ++t) acc += sc[t][c];  // (fixed order)
            carry[c] = acc;
        }
        __syncthreads();
    }
    const long long chunk = (long long)blockIdx.x * LK_T + c;
    float s[4];
    {
        double v[4] = {carry[0], carry[1], carry[2], carry[3]};
        for (int b = 0; b < 8; ++b)
            if ((c >> b) & 1) lk_mv(mpow + 16 * b, v);        // M^c carry
        const float4 l = w.local[(long long)r * w.nchunks + chunk];
        s[0] = (float)(v[0] + l.x); s[1] = (float)(v[1] + l.y); s[2] = (float)(v[2] + l.z); s[3] = (float)(v[3] + l.w);
    }
    const long long start = span0 + (long long)c * S;
    const long long qb = (start / hop + 1) * hop;         // first sample of the next quarter
    double pa = 0.0, pb = 0.0;
    for (int p = 0; p < S / LK_P; ++p) {
        __syncthreads();
        lk_stage<VEC>(xr, span0, S, p, n, tile);
        __syncthreads();
        const long long i0 = start + p * LK_P;
#pragma unroll 8
        for (int i = 0; i < LK_P; ++i) {
            const double y = lk_step(k, tile[c * LK_LDSW + i], s);
            const long long pos = i0 + i;
            if (pos < n) {
                if (pos < qb) pa = fma(y, y, pa); else pb = fma(y, y, pb);
            }
        }
    }
    w.parts[(long long)r * w.nchunks + chunk] = make_double2(pa, pb);
}

__device__ __forceinline__ double lk_quarter(const double2* __restrict__ parts, long long q, int hop, int S) {
    const long long k0 = ((long long)q * hop + S - 1) / S;            // first chunk that starts in quarter q
    const long long k1 = ((long long)(q + 1) * hop + S - 1) / S;
    double a = k0 > 0 ? parts[k0 - 1].y : 0.0;                       // the tail of the chunk that straddles into q
    for (long long kk = k0; kk < k1; ++kk) a += parts[kk].x;
    return a;
}

// fixed-order workgroup sum of (s, count); every lane gets the totals
__device__ __forceinline__ void lk_reduce(double& s, long long& cnt, double* rs, long long* rc) {
    const int c = threadIdx.x;
    rs[c] = s;
    rc[c] = cnt;
    __syncthreads();
    for (int h = LK_T / 2; h > 0; h >>= 1) {
        if (c < h) { rs[c] += rs[c + h]; rc[c] += rc[c + h]; }
        __syncthreads();
    }
    s = rs[0];
    cnt = rc[0];
    __syncthreads();
}

__global__ __launch_bounds__(LK_T) void lk_gate_kernel(const int* __restrict__ n_rows, long long n_max, int S, int hop,
                                                       double target, double ceiling_db, double* __restrict__ result,
                                                       lk_ws w) {
    __shared__ double rs[LK_T];
    __shared__ long long rc[LK_T];
    __shared__ float rp[LK_T];
    const int r = blockIdx.x, c = threadIdx.x;
    long long n = n_rows[r];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    const long long nspan = (n + (long long)LK_T * S - 1) / ((long long)LK_T * S);
    float pk = 0.f;
    for (long long j = c; j < nspan; j += LK_T) pk = fmaxf(pk, w.peak[(long long)r * w.nspans + j]);
    rp[c] = pk;
    __syncthreads();
    for (int h = LK_T / 2; h > 0; h >>= 1) {
        if (c < h) rp[c] = fmaxf(rp[c], rp[c + h]);
        __syncthreads();
    }
    const double peak = rp[0];
    const long long nq = n / hop;
    const long long nblk = nq > 3 ? nq - 3 : 0;
    const double2* parts = w.parts + (long long)r * w.nchunks;
    double* z = w.z + (long long)r * w.nblk;
    const double inv = 1.0 / (4.0 * hop);
    double s1 = 0.0;
    long long c1 = 0;
    for (long long j = c; j < nblk; j += LK_T) {         // (each lane reads back only the z it wrote itself)
        const double zj = (lk_quarter(parts, j, hop, S) + lk_quarter(parts, j + 1, hop, S) + lk_quarter(parts, j + 2, hop, S) +
                           lk_quarter(parts, j + 3, hop, S)) * inv;
        z[j] = zj;
        if (-0.691 + 10.0 * log10(zj) > -70.0) { s1 += zj; ++c1; }
    }
    lk_reduce(s1, c1, rs, rc);
    double L = -INFINITY;
    if (c1 > 0) {
        const double gr = -0.691 + 10.0 * log10(s1 / (double)c1) - 10.0;
        double s2 = 0.0;
        long long c2 = 0;
        for (long long j = c; j < nblk; j += LK_T) {
            const double zj = z[j];
            const double l = -0.691 + 10.0 * log10(zj);
            if (l > -70.0 && l > gr) { s2 += zj; ++c2; }
        }
        lk_reduce(s2, c2, rs, rc);
        if (c2 > 0) L = -0.691 + 10.0 * log10(s2 / (double)c2);
    }
    if (c == 0) {
        double g = 1.0;
        if (isfinite(L) && !isnan(target)) {
            g = pow(10.0, (target - L) / 20.0);
            const double lim = pow(10.0, ceiling_db / 20.0) / peak;
            if (lim < g) g = lim;
        }
        result[3 * r] = L;
        result[3 * r + 1] = g;
        result[3 * r + 2] = peak;
    }
}

template <bool VEC>
__global__ __launch_bounds__(LK_T) void lk_apply_kernel(const float* x, long long x_stride,   // (out may alias x)
                                                        const int* __restrict__ n_rows, long long n_max,
                                                        const double* __restrict__ result, float* out,
                                                        long long out_stride) {
    const int r = blockIdx.y;
    long long n = n_rows[r];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    const float g = (float)result[3 * r + 1];
    const float* xr = x + (long long)r * x_stride;
    float* yr = out + (long long)r * out_stride;
    const long long step = (long long)gridDim.x * LK_T;
    if (VEC) {
        const long long n4 = n / 4;
        for (long long i = (long long)blockIdx.x * LK_T + threadIdx.x; i < n4; i += step) {
            float4 v = reinterpret_cast<const float4*>(xr)[i];
            v.x *= g; v.y *= g; v.z *= g; v.w *= g;
            reinterpret_cast<float4*>(yr)[i] = v;
        }
        const long long i = 4 * n4 + (long long)blockIdx.x * LK_T + threadIdx.x;
        if (i < n) yr[i] = xr[i] * g;                     // (< 4 tail samples)
    } else {
        for (long long i = (long long)blockIdx.x * LK_T + threadIdx.x; i < n; i += step) yr[i] = xr[i] * g;
    }
}

extern "C" size_t vfx_loudness_workspace_bytes(int B, int64_t n_max, int hop, int S) {
    if (B <= 0 || n_max < 0 || hop <= 0 || S <= 0) return 0;
    size_t total = 0;
    lk_layout(B, n_max, hop, S, &total, nullptr, nullptr);
    return total;
}

extern "C" int vfx_loudness_rows_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max,
                                     const double* coef, const double* mpow, int S, int hop, int lookback, double target,
                                     double ceiling_db, float* out, int64_t out_stride, double* result, void* ws,
                                     size_t ws_bytes, vfx_stream_t stream) {
    if (!x || !n_rows || !coef || !mpow || !result || !ws || B <= 0 || B > 65535 || n_max < 0 || n_max > INT32_MAX)
        return VFX_EINVAL;
    if (S < LK_P || S % LK_P != 0 || S > 8192 || hop < S || lookback < 1 || lookback > LK_T - 1) return VFX_EINVAL;
    if (x_stride < (B > 1 ? n_max : 0) || !std::isfinite(ceiling_db) || std::isinf(target)) return VFX_EINVAL;
    const bool apply = !std::isnan(target);
    if (apply && (!out || out_stride < (B > 1 ? n_max : 0))) return VFX_EINVAL;
    for (int i = 0; i < 10; ++i)
        if (!std::isfinite(coef[i])) return VFX_EINVAL;
    size_t need = 0;
    lk_ws w;
    lk_layout(B, n_max, hop, S, &need, &w, (char*)ws);
    if (ws_bytes < need || ((uintptr_t)ws & 15u)) return VFX_EINVAL;
    const lk_coef k = {(float)coef[0], (float)coef[1], (float)coef[2], (float)coef[3], (float)coef[4],
                       (float)coef[5], (float)coef[6], (float)coef[7], (float)coef[8], (float)coef[9]};
    hipStream_t s = (hipStream_t)stream;
    const bool vx = vfx_aligned16(x) && x_stride % 4 == 0;
    const dim3 gs((unsigned)w.nspans, (unsigned)B);
    if (vx) hipLaunchKernelGGL(lk_chunk_kernel<true>, gs, dim3(LK_T), 0, s, x, (long long)x_stride, (const int*)n_rows,
                               (long long)n_max, k, mpow, S, w);
    else hipLaunchKernelGGL(lk_chunk_kernel<false>, gs, dim3(LK_T), 0, s, x, (long long)x_stride, (const int*)n_rows,
                            (long long)n_max, k, mpow, S, w);
    VFX_LAUNCHED();
    if (vx) hipLaunchKernelGGL(lk_filter_kernel<true>, gs, dim3(LK_T), 0, s, x, (long long)x_stride, (const int*)n_rows,
                               (long long)n_max, k, mpow, S, hop, lookback, w);
    else hipLaunchKernelGGL(lk_filter_kernel<false>, gs, dim3(LK_T), 0, s, x, (long long)x_stride, (const int*)n_rows,
                            (long long)n_max, k, mpow, S, hop, lookback, w);
    VFX_LAUNCHED();
    hipLaunchKernelGGL(lk_gate_kernel, dim3((unsigned)B), dim3(LK_T), 0, s, (const int*)n_rows, (long long)n_max, S, hop,
                       target, ceiling_db, result, w);
    VFX_LAUNCHED();
    if (apply) {
        long long nbx = (n_max / 4 + LK_T - 1) / LK_T;
        nbx = nbx < 1 ? 1 : (nbx > 2048 ? 2048 : nbx);
        const bool vo = vx && vfx_aligned16(out) && out_stride % 4 == 0;
        if (vo) hipLaunchKernelGGL(lk_apply_kernel<true>, dim3((unsigned)nbx, (unsigned)B), dim3(LK_T), 0, s, x,
                                   (long long)x_stride, (const int*)n_rows, (long long)n_max, (const double*)result, out,
                                   (long long)out_stride);
        else hipLaunchKernelGGL(lk_apply_kernel<false>, dim3((unsigned)nbx, (unsigned)B), dim3(LK_T), 0, s, x,
                                (long long)x_stride, (const int*)n_rows, (long long)n_max, (const double*)result, out,
                                (long long)out_stride);
        VFX_LAUNCHED();
    }
    return vfx_last_error();
}
