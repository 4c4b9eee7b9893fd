// Train-mode restorer (the reference's mode 2): BatchNorm with batch statistics and seeded dropout.
//
//   vfx_bn_stats_f32   per (batch row, BN channel): mean and biased variance of a strided region -> the affine
//                      scale = gamma / sqrt(var + eps), shift = beta - mean * scale.  Two launches: per-chunk partials
//                      (count, mean, M2) into a workspace, then a finalize that combines them in a fixed order in fp64
//                      (Chan et al.), so the result is bit-reproducible: no float atomics, no inter-workgroup flags.
//   vfx_bn_apply_f32   y = act(x * scale + shift) over the valid region; writes the pitch map's spare column as 0.
//   vfx_dropout_f32    the Philox4x32-10 mask of voicefixer_amd/dropout.py, in place, optionally fused with ReLU.
//
// Every kernel here is memory-bound; the scale / shift products are kept as scalar FMAs (Makefile: check_no_pk_fma
// covers this object too).
#include "vfx_common.h"
#include "vfx_philox.h"      // philox4x32_10

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_VEC_PER_THREAD = 4;                                   // float4 loads per thread per chunk
constexpr int BN_CHUNK = BN_THREADS * 4 * BN_VEC_PER_THREAD;           // 4096 elements per stats workgroup

// Region of one (batch row, BN channel) pair, flattened: `nseg` segments of `span` elements (a multiple of 4), the
// segments `segstride` elements apart.  Element j lives at seg = j / span, off = j % span; it counts when off < valid
// (the row's own extent) and, in the map form (pmask = P - 1 > 0), when its column off & pmask is not the spare one.
struct BnGeom {
    long long bstride, cstride;
    int C, G, nseg, span, L, pitch_log2;
};

__device__ __forceinline__ int bn_valid(const BnGeom& g, const int32_t* rows, int b) {
    return rows ? min(rows[b], g.L) : g.L;
}

__device__ __forceinline__ bool bn_counts(int off, int valid, int pmask) {
    return off < valid && (pmask == 0 || (off & pmask) != pmask);
}

// One wave-of-four block reduction in double, fixed order (LDS tree): the same inputs give the same bits.
__device__ double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = BN_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// grid (nblk, G, B): workgroup x of pair (b, g) reads chunk [x * BN_CHUNK, (x + 1) * BN_CHUNK) of the flattened region
// twice (the second pass from L2): sum -> chunk mean m, then sum (x - m)^2.  Partial = (count, mean, M2) in fp64.
__global__ __launch_bounds__(BN_THREADS) void bn_partial_kernel(const float* __restrict__ x, BnGeom g,
                                                                const int32_t* __restrict__ rows,
                                                                double* __restrict__ part, int nblk) {
    __shared__ double red[BN_THREADS];
    const int blk = blockIdx.x, gc = blockIdx.y, b = blockIdx.z;
    const int valid = bn_valid(g, rows, b);
    const int pmask = g.pitch_log2 > 0 ? (1 << g.pitch_log2) - 1 : 0;
    // map form: BN channel gc = map channel gc; 1-D form: the one BN channel spans the C map channels (segments)
    const float* base = x + (long long)b * g.bstride + (g.nseg == 1 ? (long long)gc * g.cstride : 0);
    const long long total = (long long)g.nseg * g.span;
    const long long j0 = (long long)blk * BN_CHUNK;
    float v[BN_VEC_PER_THREAD][4];
    int n = 0;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < BN_VEC_PER_THREAD; ++k) {
        const long long j = j0 + ((long long)k * BN_THREADS + threadIdx.x) * 4;
        const int seg = (int)(j / g.span), off = (int)(j - (long long)seg * g.span);
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < total && off < valid) q = *reinterpret_cast<const float4*>(base + (long long)seg * g.cstride + off);
        const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool c = j < total && bn_counts(off + i, valid, pmask);
            v[k][i] = c ? e[i] : 0.f;
            n += c ? 1 : 0;
            s += v[k][i];
        }
    }
    const double cnt = block_sum((double)n, red);
    const double sum = block_sum((double)s, red);
    const double mean = cnt > 0.0 ? sum / cnt : 0.0;
    const float mf = (float)mean;
    float q2 = 0.f;
#pragma unroll
    for (int k = 0; k < BN_VEC_PER_THREAD; ++k) {
        const long long j = j0 + ((long long)k * BN_THREADS + threadIdx.x) * 4;
        const int seg = (int)(j / g.span), off = (int)(j - (long long)seg * g.span);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool c = j < total && bn_counts(off + i, valid, pmask);
            const float d = c ? v[k][i] - mf : 0.f;
            q2 = fmaf(d, d, q2);
        }
    }
    double m2 = block_sum((double)q2, red);
    // the squares were taken about the fp32 rounding mf of the chunk mean: sum (x - mean)^2 = sum (x - mf)^2 - n (mean - mf)^2
    const double dm = mean - (double)mf;
    m2 = fmax(m2 - cnt * dm * dm, 0.0);
    if (threadIdx.x == 0) {
        double* p = part + (((long long)b * g.G + gc) * nblk + blk) * 3;
        p[0] = cnt;
        p[1] = mean;
        p[2] = m2;
    }
}

// grid (G, B), one wave: lane l folds partials l, l + 64, ... in order, then the 64 lane states are folded pairwise in a
// fixed tree (Chan's parallel formula throughout, fp64).
__global__ __launch_bounds__(64) void bn_finalize_kernel(const double* __restrict__ part, int nblk, int G,
                                                         const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps,
                                                         float* __restrict__ scale, float* __restrict__ shift) {
    __shared__ double sc[64], sm[64], sq[64];
    const int gc = blockIdx.x, b = blockIdx.y, l = threadIdx.x;
    const double* p = part + ((long long)b * G + gc) * nblk * 3;
    double n = 0.0, m = 0.0, q = 0.0;
    for (int i = l; i < nblk; i += 64) {
        const double nb = p[3 * i], mb = p[3 * i + 1], qb = p[3 * i + 2];
        if (nb == 0.0) continue;
        const double nn = n + nb, d = mb - m;
        m += d * (nb / nn);
        q += qb + d * d * (n * nb / nn);
        n = nn;
    }
    sc[l] = n;
    sm[l] = m;
    sq[l] = q;
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {
        if (l < s) {
            const double na = sc[l], nb = sc[l + s];
            if (nb > 0.0) {
                const double nn = na + nb, d = sm[l + s] - sm[l];
                sm[l] += d * (nb / nn);
                sq[l] += sq[l + s] + d * d * (na * nb / nn);
                sc[l] = nn;
            }
        }
        __syncthreads();
    }
    if (l == 0) {
        const double cnt = sc[0];
        const double mean = sm[0], var = cnt > 0.0 ? sq[0] / cnt : 0.0;   // biased variance (BatchNorm's normaliser)
        const double a = (double)gamma[gc] / sqrt(var + (double)eps);
        scale[b * G + gc] = (float)a;
        shift[b * G + gc] = (float)((double)beta[gc] - mean * a);
    }
}

// grid (ceil(L / 1024), C, B): four consecutive elements per thread (a float4 when both tensors allow it).  Map form:
// positions below the row's extent in column P - 1 are written 0; positions at or past the extent are not touched: the
// float4 instance may LOAD the whole last vector of a row (a span is padded to 4) but stores only what lies below the extent.
template <bool VEC>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, long long x_bs, long long x_cs,
                                                       float* __restrict__ y, long long y_bs, long long y_cs,
                                                       const int32_t* __restrict__ rows, int L, int pitch_log2,
                                                       int G, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, int act, float slope) {
    const int c = blockIdx.y, b = blockIdx.z;
    const int l0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int valid = rows ? min(rows[b], L) : L;
    if (l0 >= valid) return;
    const int gi = b * G + (G == 1 ? 0 : c);
    const float a = scale[gi], s = shift[gi];
    const int pmask = pitch_log2 > 0 ? (1 << pitch_log2) - 1 : 0;
    const float* xp = x + (long long)b * x_bs + (long long)c * x_cs + l0;
    float* yp = y + (long long)b * y_bs + (long long)c * y_cs + l0;
    float e[4];
    if (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(xp);
        e[0] = q.x; e[1] = q.y; e[2] = q.z; e[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) e[i] = l0 + i < valid ? xp[i] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float r = fmaf(e[i], a, s);
        if (act == VFX_POST_LRELU) r = vfx_lrelu(r, slope);
        if (pmask != 0 && ((l0 + i) & pmask) == pmask) r = 0.f;
        e[i] = r;
    }
    if (VEC && l0 + 4 <= valid) {
        *reinterpret_cast<float4*>(yp) = make_float4(e[0], e[1], e[2], e[3]);
    } else {      // the scalar instance, and the last vector of a row whose extent is no multiple of 4
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (l0 + i < valid) yp[i] = e[i];
    }
}

// grid (ceil(T / 256), C / 4, B): thread (t, c4) draws philox((t * C + 4 c4) / 4, seg_b, layer, 0) once and masks the
// four features 4 c4 .. 4 c4 + 3 of frame t (word i % 4 for feature 4 c4 + i; C % 4 == 0).
__global__ __launch_bounds__(256) void dropout_kernel(float* __restrict__ x, long long bs, long long cs,
                                                      const int32_t* __restrict__ rows, int T, int C,
                                                      const uint32_t* __restrict__ rowkey, int layer, int relu) {
    const int t = blockIdx.x * 256 + threadIdx.x, c4 = blockIdx.y, b = blockIdx.z;
    const int valid = rows ? min(rows[b], T) : T;
    if (t >= valid) return;
    const uint32_t seg = rowkey[3 * b], k0 = rowkey[3 * b + 1], k1 = rowkey[3 * b + 2];
    const unsigned long long i = (unsigned long long)t * (unsigned)C + 4u * (unsigned)c4;
    const uint4 w = philox4x32_10(make_uint4((uint32_t)(i >> 2), seg, (uint32_t)layer, 0u), make_uint2(k0, k1));
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
    float* p = x + (long long)b * bs + (long long)(4 * c4) * cs + t;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float v = p[(long long)k * cs];
        v = ws[k] < 0x80000000u ? 0.f : v * 2.f;
        if (relu) v = fmaxf(v, 0.f);
        p[(long long)k * cs] = v;
    }
}

int bn_geom(const vfx_tensor* x, int C, int L, int pitch_log2, BnGeom* g) {
    if (!x || !x->ptr || C <= 0 || L <= 0 || pitch_log2 < 0 || pitch_log2 > 7 || x->lstride != 1) return VFX_EINVAL;
    if (!vfx_aligned16(x->ptr) || (x->cstride & 3) || (x->bstride & 3)) return VFX_EALIGN;
    if (pitch_log2 > 0 && (L & ((1 << pitch_log2) - 1))) return VFX_EINVAL;
    g->bstride = x->bstride;
    g->cstride = x->cstride;
    g->C = C;
    g->L = L;
    g->pitch_log2 = pitch_log2;
    const int span = (L + 3) & ~3;
    if (pitch_log2 > 0) {
        g->G = C;
        g->nseg = 1;
    } else {
        if (C > 1 && x->cstride < span) return VFX_EINVAL;
        g->G = 1;
        g->nseg = C;
    }
    g->span = span;
    return VFX_OK;
}

int bn_nblk(const BnGeom& g) { return (int)(((long long)g.nseg * g.span + BN_CHUNK - 1) / BN_CHUNK); }

}  // namespace

extern "C" size_t vfx_bn_stats_workspace_bytes(int B, int C, int L, int pitch_log2) {
    vfx_tensor t = {};
    t.ptr = reinterpret_cast<void*>(16);
    t.lstride = 1;
    t.cstride = (L + 3) & ~3;
    BnGeom g;
    if (B <= 0 || bn_geom(&t, C, L, pitch_log2, &g) != VFX_OK) return 0;
    return (size_t)B * g.G * bn_nblk(g) * 3 * sizeof(double);
}

extern "C" int vfx_bn_stats_f32(const vfx_tensor* x, int B, int C, int L, int pitch_log2, const float* gamma,
                                const float* beta, float eps, float* scale, float* shift, void* ws, size_t ws_bytes,
                                vfx_stream_t stream) {
    BnGeom g;
    const int rc = bn_geom(x, C, L, pitch_log2, &g);
    if (rc != VFX_OK) return rc;
    if (B <= 0 || B > 65535 || g.G > 65535 || !gamma || !beta || !scale || !shift || !ws || !(eps > 0.f))
        return VFX_EINVAL;
    const int nblk = bn_nblk(g);
    if ((size_t)B * g.G * nblk * 3 * sizeof(double) > ws_bytes) return VFX_EINVAL;
    if (((uintptr_t)ws & 7u) != 0) return VFX_EALIGN;
    hipLaunchKernelGGL(bn_partial_kernel, dim3(nblk, g.G, B), dim3(BN_THREADS), 0, (hipStream_t)stream,
                       (const float*)x->ptr, g, x->rows, (double*)ws, nblk);
    VFX_LAUNCHED();
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(g.G, B), dim3(64), 0, (hipStream_t)stream, (const double*)ws, nblk,
                       g.G, gamma, beta, eps, scale, shift);
    VFX_LAUNCHED();
    return vfx_last_error();
}

extern "C" int vfx_bn_apply_f32(const vfx_tensor* x, const vfx_tensor* y, int B, int C, int L, int pitch_log2,
                                int groups, const float* scale, const float* shift, int act, float slope,
                                vfx_stream_t stream) {
    if (!x || !y || !x->ptr || !y->ptr || !scale || !shift || B <= 0 || C <= 0 || L <= 0 || B > 65535 || C > 65535)
        return VFX_EINVAL;
    if (x->lstride != 1 || y->lstride != 1 || pitch_log2 < 0 || pitch_log2 > 7) return VFX_EINVAL;
    if (pitch_log2 > 0 && (L & ((1 << pitch_log2) - 1))) return VFX_EINVAL;
    if (groups != 1 && groups != C) return VFX_EINVAL;
    if (act != VFX_POST_NONE && act != VFX_POST_LRELU) return VFX_EINVAL;
    // x->rows (the region's per-row extent) decides what is written; y is written exactly there
    const bool vec = vfx_aligned16(x->ptr) && vfx_aligned16(y->ptr) && !((x->cstride | x->bstride | y->cstride |
                                                                          y->bstride) & 3);
    dim3 grid((L + 1023) / 1024, C, B);
    if (vec)
        hipLaunchKernelGGL(bn_apply_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x->ptr,
                           x->bstride, x->cstride, (float*)y->ptr, y->bstride, y->cstride, x->rows, L, pitch_log2,
                           groups, scale, shift, act, slope);
    else
        hipLaunchKernelGGL(bn_apply_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x->ptr,
                           x->bstride, x->cstride, (float*)y->ptr, y->bstride, y->cstride, x->rows, L, pitch_log2,
                           groups, scale, shift, act, slope);
    VFX_LAUNCHED();
    return vfx_last_error();
}

extern "C" int vfx_dropout_f32(const vfx_tensor* x, int B, int C, int T, const uint32_t* rowkey, int layer, int relu,
                               vfx_stream_t stream) {
    if (!x || !x->ptr || !rowkey || B <= 0 || C <= 0 || (C & 3) || T <= 0 || B > 65535 || x->lstride != 1 || layer < 0)
        return VFX_EINVAL;
    dim3 grid((T + 255) / 256, C / 4, B);
    hipLaunchKernelGGL(dropout_kernel, grid, dim3(256), 0, (hipStream_t)stream, (float*)x->ptr, x->bstride,
                       x->cstride, x->rows, T, C, rowkey, layer, relu ? 1 : 0);
    VFX_LAUNCHED();
    return vfx_last_error();
}
