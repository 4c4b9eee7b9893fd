// vfx_loudness.hip -- integrated loudness (ITU-R BS.1770-4) of B rows, or of programmes of several rows, and the gain that normalises it
// (vfx_loudness_rows_f32), its true peak and its EBU R 128 report.  Definition, chunk scan and measured cost: DESIGN.md 3.10, 3.11.
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
//
// vfx_loudness_tp_rows_f32 (a TRUE-peak ceiling) adds lk_truepeak_kernel before the gate -- the row
// oversampled R times and reduced to max |y| per tile without being stored -- and the gate kernel's RS = 4 form folds those
// partials: result[r] = {L, g, P, TP}, g limited by TP.  vfx_loudness_report_rows_f32 adds lk_report_kernel behind the gate:
// maximum momentary / short-term loudness and the loudness range from the same quarter sums.
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

// ---- true peak ------------------------------------------------------------------------------------------
// The polyphase sum of vfx_resample_rows_f32 at down = 1, reduced to max |y| without ever writing y:
//     y[m] = sum_i bank[p][i] * x[K - J + 1 + i],   t = c + m,  K = t / R,  p = t mod R,   m in [0, R n)
// A workgroup owns TP_TILE consecutive K (all R phases of each), lane l the TP_KPL of them from K0 + TP_KPL*l.  The tile of x
// with its halo (x[K0 - Jp + 1 .. K0 + TP_TILE), zero outside [0, n)) and the bank, front-padded with zero taps to Jp (a
// multiple of 8) per phase, are staged in LDS once; the tiles start at Kal + b*TP_TILE with Kal + 1 a multiple of 4, so
// every staged float4 is an aligned one in x.  A lane slides a 12-sample register window over its taps, 8 at a time:
// three 16-byte LDS reads of x (one kept from the step before) and 2 R broadcast reads of the bank feed 32 R FMAs.  Every
// output is two chains (taps 8b..8b+3 / 8b+4..8b+7, ascending) added once -- the same order whatever B, tile or row.
#define TP_T 256
#define TP_KPL 4
#define TP_TILE (TP_T * TP_KPL)
#define TP_JMAX 2048

struct lk_tp {
    const float* part;            // [B][ntiles]  max |y| of every tile
    long long ntiles, Kal;
    int c, R;
};

static inline long long tp_kal(int c, int R) { return (((long long)(c / R) + 1) & ~3LL) - 1; }
static inline long long tp_ntiles(long long n_max) { return (n_max + 4) / TP_TILE + 1; }     // K takes <= n + 4 values from Kal
static inline int tp_jp(int J) { return (J + 7) / 8 * 8; }

// tiles that hold outputs of a row of n samples
__device__ __forceinline__ long long tp_tiles(long long n, int R, int c, long long Kal) {
    return n > 0 ? (((long long)c + (long long)R * n - 1) / R - Kal) / TP_TILE + 1 : 0;
}

// Stage the bank and the tile from K0 of the row xr (n samples) into tp_lds, then form both chains of the R * TP_KPL outputs
// of this lane: output (K0 + TP_KPL * l + k) * R + p is aa[p][k] + ab[p][k].  Shared by lk_truepeak_kernel and the limiter's
// lk_env_kernel, so the envelope and the partials are the same bits.
template <int R, bool VEC>
__device__ __forceinline__ void tp_tile_sums(const float* __restrict__ xr, long long n, const float* __restrict__ bank, int J,
                                             int Jp, long long K0, float4* tp_lds, float (&aa)[R][TP_KPL],
                                             float (&ab)[R][TP_KPL]) {
    float* xs = reinterpret_cast<float*>(tp_lds);         // [TP_TILE + Jp]
    float* bk = xs + TP_TILE + Jp;                        // [R][Jp]
    const int l = threadIdx.x;
    for (int i = l; i < R * Jp; i += TP_T) {
        const int p = i / Jp, ii = i - p * Jp - (Jp - J);
        bk[i] = ii >= 0 ? bank[p * J + ii] : 0.f;
    }
    const long long g0 = K0 - Jp + 1;                     // (a multiple of 4)
    for (int f = l; f < (TP_TILE + Jp) / 4; f += TP_T) {
        const long long idx = g0 + 4 * f;
        float4 u;
        if (VEC && idx >= 0 && idx + 3 < n) {
            u = *reinterpret_cast<const float4*>(xr + idx);
        } else {
            u.x = idx >= 0 && idx < n ? xr[idx] : 0.f;
            u.y = idx + 1 >= 0 && idx + 1 < n ? xr[idx + 1] : 0.f;
            u.z = idx + 2 >= 0 && idx + 2 < n ? xr[idx + 2] : 0.f;
            u.w = idx + 3 >= 0 && idx + 3 < n ? xr[idx + 3] : 0.f;
        }
        tp_lds[f] = u;
    }
    __syncthreads();
    const float4* xs4 = tp_lds;
    const float4* bk4 = reinterpret_cast<const float4*>(bk);
    const int nb = Jp / 4;
#pragma unroll
    for (int p = 0; p < R; ++p)
#pragma unroll
        for (int k = 0; k < TP_KPL; ++k) { aa[p][k] = 0.f; ab[p][k] = 0.f; }
    float4 a = xs4[l];
    for (int ib = 0; ib < nb; ib += 2) {
        const float4 b = xs4[l + ib + 1], d = xs4[l + ib + 2];
        const float w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, d.x, d.y, d.z, d.w};
#pragma unroll
        for (int p = 0; p < R; ++p) {
            const float4 u = bk4[p * nb + ib], v = bk4[p * nb + ib + 1];
            const float tu[4] = {u.x, u.y, u.z, u.w}, tv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int k = 0; k < TP_KPL; ++k) {
                    aa[p][k] = fmaf(tu[e], w[k + e], aa[p][k]);
                    ab[p][k] = fmaf(tv[e], w[4 + k + e], ab[p][k]);
                }
        }
        a = d;
    }
}

template <int R, bool VEC>
__global__ __launch_bounds__(TP_T) void lk_truepeak_kernel(const float* __restrict__ x, long long x_stride,
                                                           const int* __restrict__ n_rows, long long n_max,
                                                           const float* __restrict__ bank, int J, int Jp, float* part,
                                                           lk_tp t) {
    extern __shared__ float4 tp_lds[];
    float* xs = reinterpret_cast<float*>(tp_lds);         // [TP_TILE + Jp]
    const int r = blockIdx.y, l = threadIdx.x;
    long long n = n_rows[r];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    if ((long long)blockIdx.x >= tp_tiles(n, R, t.c, t.Kal)) return;         // (uniform over the workgroup)
    const long long t_end = (long long)t.c + (long long)R * n;
    const long long K0 = t.Kal + (long long)blockIdx.x * TP_TILE;
    float aa[R][TP_KPL], ab[R][TP_KPL];
    tp_tile_sums<R, VEC>(x + (long long)r * x_stride, n, bank, J, Jp, K0, tp_lds, aa, ab);
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < TP_KPL; ++k)
#pragma unroll
        for (int p = 0; p < R; ++p) {
            const long long tt = (K0 + TP_KPL * l + k) * R + p;
            if (tt >= t.c && tt < t_end) m = fmaxf(m, fabsf(aa[p][k] + ab[p][k]));
        }
    __syncthreads();
    xs[l] = m;
    __syncthreads();
    for (int h = TP_T / 2; h > 0; h >>= 1) {
        if (l < h) xs[l] = fmaxf(xs[l], xs[l + h]);
        __syncthreads();
    }
    if (l == 0) part[(long long)r * t.ntiles + blockIdx.x] = xs[0];
}

// RS = 3: result[r] = {L, g, P}, the gain limited by the sample peak P.  RS = 4: result[r] = {L, g, P, TP}, TP = max(P, the
// row's true-peak partials of lk_truepeak_kernel), the gain limited by TP.
//
// GRP (a programme of adjacent rows per workgroup): workgroup g owns rows [start[g], start[g + 1]), all of
// the length of the first; peaks and true-peak partials are folded over all of them, z_j sums the rows' quarter sums times
// their weights in ascending row order (fp64; one row of weight 1.0: the bits of the per-row form), result[g] = {L, g, P, TP}
// and, where rowres is given, the same four values once per row of the programme for lk_apply_kernel<., 4>.
struct lk_grp {
    const int* start;             // [G + 1]  first row of every programme, start[G] = B
    const double* weight;         // [B]      channel weight of every row
    double* rowres;               // [B][4]   the programme's result repeated per row (NULL: not written)
    int B;
};

template <int RS, bool GRP = false>
__global__ __launch_bounds__(LK_T) void lk_gate_kernel(const int* __restrict__ n_rows, long long n_max, int S, int hop,
                                                       double target, double ceiling_db, double* __restrict__ result,
                                                       lk_ws w, lk_tp t, lk_grp grp) {
    __shared__ double rs[LK_T];
    __shared__ long long rc[LK_T];
    __shared__ float rp[LK_T];
    const int c = threadIdx.x;
    int r = blockIdx.x, r1 = r + 1;
    if (GRP) {                                            // (whatever start holds, the rows stay inside [0, B])
        r = grp.start[blockIdx.x];
        r1 = grp.start[blockIdx.x + 1];
        r = r < 0 ? 0 : (r > grp.B ? grp.B : r);
        r1 = r1 < r ? r : (r1 > grp.B ? grp.B : r1);
    }
    long long n = !GRP || r < r1 ? n_rows[r] : 0;
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    const long long nspan = (n + (long long)LK_T * S - 1) / ((long long)LK_T * S);
    float pk = 0.f;
    if (GRP) {
        for (int rr = r; rr < r1; ++rr)
            for (long long j = c; j < nspan; j += LK_T) pk = fmaxf(pk, w.peak[(long long)rr * w.nspans + j]);
    } else {
        for (long long j = c; j < nspan; j += LK_T) pk = fmaxf(pk, w.peak[(long long)r * w.nspans + j]);
    }
    rp[c] = pk;
    __syncthreads();
    for (int h = LK_T / 2; h > 0; h >>= 1) {
        if (c < h) rp[c] = fmaxf(rp[c], rp[c + h]);
        __syncthreads();
    }
    const double peak = rp[0];
    double tpk = peak;
    if (RS == 4) {
        float m = 0.f;
        const long long nt = t.R > 1 ? tp_tiles(n, t.R, t.c, t.Kal) : 0;
        for (int rr = r; rr < r1; ++rr) {                 // (one row unless GRP)
            const float* __restrict__ pr = t.part + (long long)rr * t.ntiles;
#pragma unroll 8
            for (long long j = c; j < nt; j += LK_T) m = fmaxf(m, pr[j]); // (8 loads in flight: one workgroup, ~300 per lane for 30 min)
        }
        __syncthreads();
        rp[c] = m;
        __syncthreads();
        for (int h = LK_T / 2; h > 0; h >>= 1) {
            if (c < h) rp[c] = fmaxf(rp[c], rp[c + h]);
            __syncthreads();
        }
        tpk = fmax(peak, (double)rp[0]);
    }
    const long long nq = n / hop;
    const long long nblk = nq > 3 ? nq - 3 : 0;
    const double2* parts = w.parts + (long long)r * w.nchunks;
    double* z = w.z + (long long)r * w.nblk;
    const double inv = 1.0 / (4.0 * hop);
    double s1 = 0.0;
    long long c1 = 0;
    for (long long j = c; j < nblk; j += LK_T) {         // (each lane reads back only the z it wrote itself)
        double zj;
        if (GRP) {
            double a = 0.0;
            for (int rr = r; rr < r1; ++rr) {             // (ascending rows: a fixed order)
                const double2* pc = w.parts + (long long)rr * w.nchunks;
                a += grp.weight[rr] * (lk_quarter(pc, j, hop, S) + lk_quarter(pc, j + 1, hop, S) + lk_quarter(pc, j + 2, hop, S) +
                                       lk_quarter(pc, j + 3, hop, S));
            }
            zj = a * inv;
        } else {
            zj = (lk_quarter(parts, j, hop, S) + lk_quarter(parts, j + 1, hop, S) + lk_quarter(parts, j + 2, hop, S) +
                  lk_quarter(parts, j + 3, hop, S)) * inv;
        }
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
            const double lim = pow(10.0, ceiling_db / 20.0) / (RS == 4 ? tpk : peak);
            if (lim < g) g = lim;
        }
        const int o = GRP ? blockIdx.x : r;
        result[RS * o] = L;
        result[RS * o + 1] = g;
        result[RS * o + 2] = peak;
        if (RS == 4) result[RS * o + 3] = tpk;
        if (GRP && RS == 4 && grp.rowres)
            for (int rr = r; rr < r1; ++rr) {
                grp.rowres[4 * rr] = L;
                grp.rowres[4 * rr + 1] = g;
                grp.rowres[4 * rr + 2] = peak;
                grp.rowres[4 * rr + 3] = tpk;
            }
    }
}

// ---- loudness report (EBU Tech 3341 / 3342) -----------------------------------------------------------------
#define LK_ST 30                  // quarters of one 3 s short-term block

// number of keys below `cand` (every lane gets it)
__device__ __forceinline__ long long lk_count_below(const unsigned long long* __restrict__ key, long long nst,
                                                    unsigned long long cand, long long* rc) {
    const int c = threadIdx.x;
    long long cnt = 0;
    for (long long j = c; j < nst; j += LK_T) cnt += key[j] < cand;
    rc[c] = cnt;
    __syncthreads();
    for (int h = LK_T / 2; h > 0; h >>= 1) {
        if (c < h) rc[c] += rc[c + h];
        __syncthreads();
    }
    cnt = rc[0];
    __syncthreads();
    return cnt;
}

// the k-th smallest key (k from 0), bit by bit from the top: exact, and the same whatever the order of the keys
__device__ __forceinline__ unsigned long long lk_select(const unsigned long long* __restrict__ key, long long nst, long long k,
                                                        long long* rc) {
    unsigned long long pre = 0;
    for (int b = 63; b >= 0; --b) {
        const unsigned long long cand = pre | (1ULL << b);
        if (lk_count_below(key, nst, cand, rc) <= k) pre = cand;
    }
    return pre;
}

// One workgroup per row, after lk_gate_kernel<4>: report[r] = {L, LRA, max momentary, max short-term, P, TP}.
// qs [B][nqmax]: the row's quarter sums; st [B][nqmax]: its short-term energies, then their bit patterns as sort keys
// (positive doubles order as their bits do; a block below a gate gets the key ~0 and is never counted).
// GRP: one workgroup per programme, after lk_gate_kernel<4, true>: the quarter sums are Q_i = sum over the programme's rows of
// weight * q_i (ascending rows, fp64), kept in the slices of its first row; res4 and report are indexed by programme.
template <bool GRP>
__global__ __launch_bounds__(LK_T) void lk_report_kernel(const int* __restrict__ n_rows, long long n_max, int S, int hop,
                                                         const double* __restrict__ res4, double* __restrict__ report,
                                                         double* __restrict__ qs, double* __restrict__ st,
                                                         long long nqmax, lk_ws w, lk_grp grp) {
    __shared__ double rs[LK_T];
    __shared__ long long rc[LK_T];
    const int c = threadIdx.x;
    int r = blockIdx.x, r1 = r + 1;
    if (GRP) {
        r = grp.start[blockIdx.x];
        r1 = grp.start[blockIdx.x + 1];
        r = r < 0 ? 0 : (r > grp.B ? grp.B : r);
        r1 = r1 < r ? r : (r1 > grp.B ? grp.B : r1);
    }
    long long n = !GRP || r < r1 ? n_rows[r] : 0;
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    const long long nq = n / hop;
    const long long nblk = nq > 3 ? nq - 3 : 0;
    const long long nst = nq >= LK_ST ? nq - LK_ST + 1 : 0;
    const double2* parts = w.parts + (long long)r * w.nchunks;
    const double* z = w.z + (long long)r * w.nblk;
    double* q = qs + (long long)r * nqmax;
    double* e = st + (long long)r * nqmax;
    unsigned long long* key = reinterpret_cast<unsigned long long*>(e);
    double zm = -1.0;                                     // (max is exact: any order gives the same bits)
    for (long long j = c; j < nblk; j += LK_T) zm = fmax(zm, z[j]);
    if (GRP) {
        for (long long j = c; j < nq; j += LK_T) {
            double a = 0.0;
            for (int rr = r; rr < r1; ++rr) a += grp.weight[rr] * lk_quarter(w.parts + (long long)rr * w.nchunks, j, hop, S);
            q[j] = a;
        }
    } else {
        for (long long j = c; j < nq; j += LK_T) q[j] = lk_quarter(parts, j, hop, S);
    }
    __syncthreads();                                      // (q is read across lanes below)
    const double inv = 1.0 / ((double)LK_ST * hop);
    double em = -1.0, s1 = 0.0;
    long long c1 = 0;
    for (long long j = c; j < nst; j += LK_T) {
        double a = 0.0;
        for (int i = 0; i < LK_ST; ++i) a += q[j + i];    // (fixed order)
        a *= inv;
        e[j] = a;
        em = fmax(em, a);
        if (-0.691 + 10.0 * log10(a) > -70.0) { s1 += a; ++c1; }
    }
    rs[c] = zm;
    __syncthreads();
    for (int h = LK_T / 2; h > 0; h >>= 1) {
        if (c < h) rs[c] = fmax(rs[c], rs[c + h]);
        __syncthreads();
    }
    zm = rs[0];
    __syncthreads();
    rs[c] = em;
    __syncthreads();
    for (int h = LK_T / 2; h > 0; h >>= 1) {
        if (c < h) rs[c] = fmax(rs[c], rs[c + h]);
        __syncthreads();
    }
    em = rs[0];
    __syncthreads();
    lk_reduce(s1, c1, rs, rc);
    double lra = 0.0;
    if (c1 > 0) {
        const double gr = -0.691 + 10.0 * log10(s1 / (double)c1) - 20.0;
        long long c2 = 0;
        double zero = 0.0;
        for (long long j = c; j < nst; j += LK_T) {      // (each lane rewrites only the entries it wrote itself)
            const double a = e[j];
            const double lj = -0.691 + 10.0 * log10(a);
            const bool keep = lj > -70.0 && lj > gr;
            key[j] = keep ? (unsigned long long)__double_as_longlong(a) : ~0ULL;
            c2 += keep;
        }
        lk_reduce(zero, c2, rs, rc);                      // (also orders the key writes before the counting reads)
        if (c2 > 0) {
            const double lo = __longlong_as_double((long long)lk_select(key, nst, (c2 - 1 + 5) / 10, rc));
            const double hi = __longlong_as_double((long long)lk_select(key, nst, ((c2 - 1) * 95 + 50) / 100, rc));
            lra = (-0.691 + 10.0 * log10(hi)) - (-0.691 + 10.0 * log10(lo));
        }
    }
    if (c == 0) {
        const int o = GRP ? blockIdx.x : r;
        report[6 * o] = res4[4 * o];
        report[6 * o + 1] = lra;
        report[6 * o + 2] = zm >= 0.0 ? -0.691 + 10.0 * log10(zm) : -INFINITY;
        report[6 * o + 3] = em >= 0.0 ? -0.691 + 10.0 * log10(em) : -INFINITY;
        report[6 * o + 4] = res4[4 * o + 2];
        report[6 * o + 5] = res4[4 * o + 3];
    }
}

template <bool VEC, int RS>
__global__ __launch_bounds__(LK_T) void lk_apply_kernel(const float* x, long long x_stride,   // (out may alias x)
                                                        const int* __restrict__ n_rows, long long n_max,
                                                        const double* __restrict__ result, float* out,
                                                        long long out_stride) {
    const int r = blockIdx.y;
    long long n = n_rows[r];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    const float g = (float)result[RS * r + 1];
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

// Extra workspace behind lk_layout's: the true-peak partials, then (report only) the {L, g, P, TP} rows, the quarter sums and
// the short-term energies.
struct lk_ext {
    float* part;
    double* res4;
    double* qs;
    double* st;
    long long ntiles, nqmax;
};

static void lk_ext_layout(int B, long long n_max, int hop, bool report, size_t* total, lk_ext* e, char* base) {
    const long long ntiles = tp_ntiles(n_max);
    const long long nqmax = hop > 0 && n_max / hop > 0 ? n_max / hop : 1;
    size_t off = 0;
    const size_t o_part = off; off += lk_round((size_t)B * ntiles * sizeof(float));
    size_t o_res = 0, o_q = 0, o_st = 0;
    if (report) {
        o_res = off; off += lk_round((size_t)B * 4 * sizeof(double));
        o_q = off;   off += lk_round((size_t)B * nqmax * sizeof(double));
        o_st = off;  off += lk_round((size_t)B * nqmax * sizeof(double));
    }
    *total = off;
    if (e) {
        e->part = (float*)(base + o_part);
        e->res4 = report ? (double*)(base + o_res) : nullptr;
        e->qs = report ? (double*)(base + o_q) : nullptr;
        e->st = report ? (double*)(base + o_st) : nullptr;
        e->ntiles = ntiles;
        e->nqmax = nqmax;
    }
}

#include "vfx_limit.inc"

// mode 0: vfx_loudness_rows_f32 ({L, g, P});  1: with the true peak ({L, g, P, TP});  2: the report (measure only);
// 3: the look-ahead limiter (vfx_loudness_limit_f32: the measurement of mode 1, then lk_limit_run; result has 8 columns).
// G > 0 (modes 1, 2 and 3): the rows form G programmes (group_start, weight: lk_grp), result / report have G rows.
static int lk_run(int mode, const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max, const double* coef,
                  const double* mpow, int S, int hop, int lookback, double target, double ceiling_db, const float* bank, int J,
                  int R, int c, float* out, int64_t out_stride, double* result, void* ws, size_t ws_bytes, vfx_stream_t stream,
                  int G = 0, const int32_t* group_start = nullptr, const double* weight = nullptr, int H = 0) {
    if (!x || !n_rows || !coef || !mpow || !result || !ws || B <= 0 || B > 65535 || n_max < 0 || n_max > INT32_MAX)
        return VFX_EINVAL;
    const bool grouped = G != 0 || group_start || weight;
    if (grouped && (G < 1 || G > B || !group_start || !weight || mode == 0)) return VFX_EINVAL;
    if (S < LK_P || S % LK_P != 0 || S > 8192 || hop < S || lookback < 1 || lookback > LK_T - 1) return VFX_EINVAL;
    if (x_stride < (B > 1 ? n_max : 0) || !std::isfinite(ceiling_db) || std::isinf(target)) return VFX_EINVAL;
    const bool apply = !std::isnan(target);
    if (apply && (!out || out_stride < (B > 1 ? n_max : 0))) return VFX_EINVAL;
    for (int i = 0; i < 10; ++i)
        if (!std::isfinite(coef[i])) return VFX_EINVAL;
    if (mode != 0 && (!bank || J < 1 || J > TP_JMAX || (R != 1 && R != 2 && R != 4) || c < 0 || (long long)c >= (long long)R * J))
        return VFX_EINVAL;
    size_t need = 0, more = 0;
    lk_ws w;
    lk_ext e = {nullptr, nullptr, nullptr, nullptr, 0, 0};
    lk_layout(B, n_max, hop, S, &need, &w, (char*)ws);
    if (mode != 0) lk_ext_layout(B, n_max, hop, mode == 2, &more, &e, (char*)ws + need);
    const size_t rowres_bytes = grouped && mode == 1 ? lk_round((size_t)B * 4 * sizeof(double)) : 0;
    size_t lim_bytes = 0;
    lk_lim lm = {};
    if (mode == 3) {
        if (H < 1 || H > LM_HMAX || std::isnan(target) || !lk_lim_alias_ok(x, x_stride, out, out_stride, B, n_max)) return VFX_EINVAL;
        lk_lim_layout(B, n_max, &lim_bytes, &lm, (char*)ws + need + more);
    }
    if (ws_bytes < need + more + rowres_bytes + lim_bytes || ((uintptr_t)ws & 15u)) return VFX_EINVAL;
    const lk_grp grp = {(const int*)group_start, weight, rowres_bytes ? (double*)((char*)ws + need + more) : nullptr, B};
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
    lk_tp t = {e.part, e.ntiles, 0, c, R};
    if (mode != 0 && R > 1 && n_max > 0) {
        t.Kal = tp_kal(c, R);
        const int Jp = tp_jp(J);
        const size_t lds = (size_t)(TP_TILE + Jp + R * Jp) * sizeof(float);
        const dim3 gt((unsigned)e.ntiles, (unsigned)B);
#define TP_LAUNCH(RR, VV) hipLaunchKernelGGL((lk_truepeak_kernel<RR, VV>), gt, dim3(TP_T), lds, s, x, (long long)x_stride, \
                                             (const int*)n_rows, (long long)n_max, bank, J, Jp, e.part, t)
        if (R == 4) { if (vx) TP_LAUNCH(4, true); else TP_LAUNCH(4, false); }
        else { if (vx) TP_LAUNCH(2, true); else TP_LAUNCH(2, false); }
#undef TP_LAUNCH
        VFX_LAUNCHED();
    } else {
        t.R = 1;                                          // (no partials: TP = P)
    }
    if (mode == 0) hipLaunchKernelGGL((lk_gate_kernel<3, false>), dim3((unsigned)B), dim3(LK_T), 0, s, (const int*)n_rows,
                                      (long long)n_max, S, hop, target, ceiling_db, result, w, t, grp);
    else if (!grouped) hipLaunchKernelGGL((lk_gate_kernel<4, false>), dim3((unsigned)B), dim3(LK_T), 0, s, (const int*)n_rows,
                                          (long long)n_max, S, hop, target, ceiling_db,
                                          mode == 2 ? e.res4 : (mode == 3 ? lm.res4 : result), w, t, grp);
    else hipLaunchKernelGGL((lk_gate_kernel<4, true>), dim3((unsigned)G), dim3(LK_T), 0, s, (const int*)n_rows,
                            (long long)n_max, S, hop, target, ceiling_db, mode == 2 ? e.res4 : (mode == 3 ? lm.res4 : result), w, t,
                            grp);
    VFX_LAUNCHED();
    if (mode == 2) {
        if (!grouped) hipLaunchKernelGGL(lk_report_kernel<false>, dim3((unsigned)B), dim3(LK_T), 0, s, (const int*)n_rows,
                                         (long long)n_max, S, hop, (const double*)e.res4, result, e.qs, e.st, e.nqmax, w, grp);
        else hipLaunchKernelGGL(lk_report_kernel<true>, dim3((unsigned)G), dim3(LK_T), 0, s, (const int*)n_rows,
                                (long long)n_max, S, hop, (const double*)e.res4, result, e.qs, e.st, e.nqmax, w, grp);
        VFX_LAUNCHED();
    }
    if (mode == 3)
        return lk_limit_run(x, x_stride, n_rows, B, n_max, target, ceiling_db, bank, J, H, out, out_stride, result, s, t, grp,
                            grouped ? G : 0, lm);
    if (apply) {
        long long nbx = (n_max / 4 + LK_T - 1) / LK_T;
        nbx = nbx < 1 ? 1 : (nbx > 2048 ? 2048 : nbx);
        const bool vo = vx && vfx_aligned16(out) && out_stride % 4 == 0;
        const dim3 ga((unsigned)nbx, (unsigned)B);
#define AP_LAUNCH(VV, RS) hipLaunchKernelGGL((lk_apply_kernel<VV, RS>), ga, dim3(LK_T), 0, s, x, (long long)x_stride, \
                                             (const int*)n_rows, (long long)n_max, \
                                             (const double*)(grp.rowres ? grp.rowres : result), out, (long long)out_stride)
        if (mode == 0) { if (vo) AP_LAUNCH(true, 3); else AP_LAUNCH(false, 3); }
        else { if (vo) AP_LAUNCH(true, 4); else AP_LAUNCH(false, 4); }
#undef AP_LAUNCH
        VFX_LAUNCHED();
    }
    return vfx_last_error();
}

extern "C" int vfx_loudness_rows_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max,
                                     const double* coef, const double* mpow, int S, int hop, int lookback, double target,
                                     double ceiling_db, float* out, int64_t out_stride, double* result, void* ws,
                                     size_t ws_bytes, vfx_stream_t stream) {
    return lk_run(0, x, x_stride, n_rows, B, n_max, coef, mpow, S, hop, lookback, target, ceiling_db, nullptr, 0, 1, 0, out,
                  out_stride, result, ws, ws_bytes, stream);
}

extern "C" size_t vfx_true_peak_workspace_bytes(int B, int64_t n_max, int R, int J) {
    if (B <= 0 || n_max < 0 || n_max > INT32_MAX || J < 1 || J > TP_JMAX || (R != 1 && R != 2 && R != 4)) return 0;
    size_t total = 0;
    lk_ext_layout(B, n_max, 0, false, &total, nullptr, nullptr);
    return total;
}

extern "C" int vfx_loudness_tp_rows_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max,
                                        const double* coef, const double* mpow, int S, int hop, int lookback, double target,
                                        double ceiling_db, const float* bank, int J, int R, int c, float* out,
                                        int64_t out_stride, double* result, void* ws, size_t ws_bytes, vfx_stream_t stream) {
    return lk_run(1, x, x_stride, n_rows, B, n_max, coef, mpow, S, hop, lookback, target, ceiling_db, bank, J, R, c, out,
                  out_stride, result, ws, ws_bytes, stream);
}

extern "C" size_t vfx_loudness_report_workspace_bytes(int B, int64_t n_max, int hop, int S, int R, int J) {
    if (B <= 0 || n_max < 0 || n_max > INT32_MAX || hop <= 0 || S <= 0 || J < 1 || J > TP_JMAX || (R != 1 && R != 2 && R != 4))
        return 0;
    size_t total = 0, more = 0;
    lk_layout(B, n_max, hop, S, &total, nullptr, nullptr);
    lk_ext_layout(B, n_max, hop, true, &more, nullptr, nullptr);
    return total + more;
}

extern "C" int vfx_loudness_report_rows_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max,
                                            const double* coef, const double* mpow, int S, int hop, int lookback,
                                            const float* bank, int J, int R, int c, double* report, void* ws, size_t ws_bytes,
                                            vfx_stream_t stream) {
    return lk_run(2, x, x_stride, n_rows, B, n_max, coef, mpow, S, hop, lookback, NAN, -1.0, bank, J, R, c, nullptr, 0, report,
                  ws, ws_bytes, stream);
}

/* ---- programmes of several channels ------------------------------------------------------------------------ */

extern "C" size_t vfx_loudness_groups_workspace_bytes(int B, int64_t n_max, int hop, int S, int R, int J) {
    if (B <= 0 || n_max < 0 || n_max > INT32_MAX || hop <= 0 || S <= 0 || J < 1 || J > TP_JMAX || (R != 1 && R != 2 && R != 4))
        return 0;
    size_t total = 0, more = 0;
    lk_layout(B, n_max, hop, S, &total, nullptr, nullptr);
    lk_ext_layout(B, n_max, hop, false, &more, nullptr, nullptr);
    return total + more + lk_round((size_t)B * 4 * sizeof(double));
}

extern "C" int vfx_loudness_groups_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max,
                                       const int32_t* group_start, const double* weight, int G, const double* coef,
                                       const double* mpow, int S, int hop, int lookback, double target, double ceiling_db,
                                       const float* bank, int J, int R, int c, float* out, int64_t out_stride, double* result,
                                       void* ws, size_t ws_bytes, vfx_stream_t stream) {
    if (G < 1 || !group_start || !weight) return VFX_EINVAL;
    return lk_run(1, x, x_stride, n_rows, B, n_max, coef, mpow, S, hop, lookback, target, ceiling_db, bank, J, R, c, out,
                  out_stride, result, ws, ws_bytes, stream, G, group_start, weight);
}

extern "C" size_t vfx_loudness_report_groups_workspace_bytes(int B, int64_t n_max, int hop, int S, int R, int J) {
    return vfx_loudness_report_workspace_bytes(B, n_max, hop, S, R, J);
}

extern "C" int vfx_loudness_report_groups_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max,
                                              const int32_t* group_start, const double* weight, int G, const double* coef,
                                              const double* mpow, int S, int hop, int lookback, const float* bank, int J, int R,
                                              int c, double* report, void* ws, size_t ws_bytes, vfx_stream_t stream) {
    if (G < 1 || !group_start || !weight) return VFX_EINVAL;
    return lk_run(2, x, x_stride, n_rows, B, n_max, coef, mpow, S, hop, lookback, NAN, -1.0, bank, J, R, c, nullptr, 0, report,
                  ws, ws_bytes, stream, G, group_start, weight);
}

/* ---- look-ahead peak limiter (kernels: vfx_limit.inc) -------------------------------------------------------- */

extern "C" size_t vfx_loudness_limit_workspace_bytes(int B, int64_t n_max, int hop, int S, int R, int J) {
    if (B <= 0 || n_max < 0 || n_max > INT32_MAX || hop <= 0 || S <= 0 || J < 1 || J > TP_JMAX || (R != 1 && R != 2 && R != 4))
        return 0;
    size_t total = 0, more = 0, lim = 0;
    lk_layout(B, n_max, hop, S, &total, nullptr, nullptr);
    lk_ext_layout(B, n_max, hop, false, &more, nullptr, nullptr);
    lk_lim_layout(B, n_max, &lim, nullptr, nullptr);
    return total + more + lim;
}

extern "C" int vfx_loudness_limit_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max,
                                      const int32_t* group_start, const double* weight, int G, const double* coef,
                                      const double* mpow, int S, int hop, int lookback, double target, double ceiling_db,
                                      const float* bank, int J, int R, int c, float* out, int64_t out_stride, int H,
                                      int true_peak, double* result, void* ws, size_t ws_bytes, vfx_stream_t stream) {
    if (G < 0 || (true_peak != 0 && true_peak != 1)) return VFX_EINVAL;
    if (!true_peak) R = 1;                                // (the sample-peak limiter: nothing is oversampled)
    return lk_run(3, x, x_stride, n_rows, B, n_max, coef, mpow, S, hop, lookback, target, ceiling_db, bank, J, R, c, out,
                  out_stride, result, ws, ws_bytes, stream, G, group_start, weight, H);
}

/* ---- the span stages of a streaming session, one row or the linked channels of a programme ----------- */

#include "vfx_limit_span.inc"
#include "vfx_level_span.inc"
#include "vfx_meter_span.inc"
