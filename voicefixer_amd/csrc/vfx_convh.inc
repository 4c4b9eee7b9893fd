// vfx_convh.inc -- opt-in f16 arithmetic for the k = 3 dilated Conv1d of the wide ResStack layers (vfx_conv1d_f16,
// included from vfx_conv.hip).
//
// A direct implicit GEMM on v_mfma_f32_32x32x16_f16: operands rounded to fp16 (round to nearest even), products
// accumulated in fp32.  No Winograd: the transforms amplify operand rounding, and at 16x the fp32 MFMA rate per clock
// the direct sum already costs less than F(4,3)'s halved fp32 product count.
//
//   M = Cout (MFMA rows, A = weights, pre-packed fp16 [tap][C/8][Cout][8], read from L2 straight into registers),
//   N = positions (MFMA columns, B = activations from LDS),
//   K = Cin x 3 taps, in chunks of 32 channels.
//
// Workgroup = 256 threads = 4 wave64 on a 128 (Cout) x 128 (position) tile, 2 x 2 waves of 64 x 64 (2 x 2
// accumulators of 32 x 32).  Per chunk the activations are staged ONCE as fp16 into LDS as [c8][position][8 channels]
// (16 bytes per (8-channel group, position): one ds_read_b128 per lane is an MFMA B operand, 32 lanes read 512
// contiguous bytes): one span of 128 + 2d positions that the three taps read at shifted columns when the halo is short
// (d <= 64), three spans of 128 positions (one per tap) otherwise.  Staging reads fp32 from HBM, applies the
// pre-activation in fp32, checks the range, and converts RNE (v_cvt_f16_f32 in the default rounding mode -- never the
// round-toward-zero v_cvt_pkrtz_f16_f32).  Positions outside [0, row length) are staged as zeros and never read, so
// guard bands are irrelevant (guard 0 is legal) and a ragged row computes exactly what a launch of its own does.
// LDS is double buffered: the next chunk's activations travel HBM -> VGPR while the MFMAs of the current one run, one
// barrier per chunk.  The epilogue (bias, residual, post-activation) is fp32.
//
// Range guard: a staged operand that is not finite or exceeds 65504 in magnitude (fp16 overflow) sets *range_flag
// (one atomic per wave at most); the output of the launch is then unspecified and the caller re-runs it in fp32.

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2h __attribute__((ext_vector_type(2)));

namespace convh {
constexpr int BM = 128, BL = 128, KC = 32, NTHR = 256;
constexpr int NPMAX = 3 * BL;                        // staged positions per chunk (three tap spans)
constexpr int NU = (KC / 8) * NPMAX / NTHR;          // (8-channel group, position) staging units per thread: 6
constexpr int BUFB = (KC / 8) * NPMAX * 16;          // bytes per LDS buffer: 24 KB
constexpr float F16_MAX = 65504.f;
}  // namespace convh

struct ConvhArgs {
    const float* x; long long x_bs, x_cs;
    const int32_t* x_rows;
    const _Float16* w;
    const float* bias;
    const float* res; long long r_bs, r_cs;
    float* y; long long y_bs, y_cs;
    int C, L, d, ntiles, nm;
    int pre_act; float pre_slope;
    int post_act; float post_slope;
    int32_t* flag;
};

// BIAS / RES: bias and residual present (template arguments: no run-time test around their loads)
template <bool BIAS, bool RES>
__global__ __launch_bounds__(256, 2) void convh_kernel(const ConvhArgs a) {
    using namespace convh;
    __shared__ __attribute__((aligned(16))) unsigned char sm[2 * BUFB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lo = lane & 31, hi = lane >> 5;
    const int wm = wave >> 1, wl = wave & 1;
    const int mb = blockIdx.x % a.nm, tile = blockIdx.x / a.nm;
    const int b = blockIdx.z;
    const int m0 = mb * BM, l0 = tile * BL;
    const int len = a.x_rows ? min(a.x_rows[b], a.L) : a.L;
    if (l0 >= len) return;   // past the row's valid length: outputs unspecified (whole workgroup, before any barrier)

    const int d = a.d;
    const bool span = 2 * d <= BL;                   // one shared span (halo fits) or one span per tap
    const int np = span ? BL + 2 * d : 3 * BL;
    const int nunits = (KC / 8) * np;

    // per-thread staging units, fixed for the whole K loop: (8-channel group g, staged position p) -> global position l
    const float* px[NU];
    unsigned okm[NU];   // all ones: the unit's position is inside the row; 0: staged as +0 (an AND, never a branch)
    bool live[NU];
    int lds_off[NU];
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        const int u = tid + NTHR * j;
        live[j] = u < nunits;
        const int uu = live[j] ? u : 0;
        const int g = uu / np, p = uu - g * np;
        const int l = span ? l0 - d + p : l0 + ((p >> 7) - 1) * d + (p & (BL - 1));
        const bool ok = live[j] && l >= 0 && l < len;
        okm[j] = ok ? 0xffffffffu : 0u;
        px[j] = a.x + (long long)b * a.x_bs + (long long)(8 * g) * a.x_cs + (ok ? l : 0);   // always a valid address
        lds_off[j] = live[j] ? (g * np + p) * 16 : u * 16;   // units past the tile write zeros where no MFMA reads
    }
    const int nchunks = a.C / KC;
    const long long xcs = a.x_cs;
    const float slope = a.pre_act == VFX_PRE_LRELU ? a.pre_slope : 1.f;
    bool bad = false;

    float xr[NU][8];
    auto load_x = [&](int c) {
        const long long co = (long long)c * KC * xcs;
#pragma unroll
        for (int j = 0; j < NU; ++j)
#pragma unroll
            for (int i = 0; i < 8; ++i) xr[j][i] = px[j][co + i * xcs];   // unconditional: masked in stage()
    };
    auto stage = [&](unsigned char* buf) {
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            u32x4 q;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v0 = xr[j][2 * i], v1 = xr[j][2 * i + 1];
                // zero padding / ragged row end / unit past the tile: the bits are cleared, then the pre-activation
                v0 = __uint_as_float(__float_as_uint(v0) & okm[j]);
                v1 = __uint_as_float(__float_as_uint(v1) & okm[j]);
                v0 *= v0 > 0.f ? 1.f : slope;
                v1 *= v1 > 0.f ? 1.f : slope;
                bad |= !(__builtin_fabsf(v0) <= F16_MAX) || !(__builtin_fabsf(v1) <= F16_MAX);
                const f32x2h v = {v0, v1};
                q[i] = __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));   // RNE
            }
            *reinterpret_cast<u32x4*>(buf + lds_off[j]) = q;
        }
    };

    // A operand (weights): lane (lo, hi) holds row m = m0 + wm*64 + i*32 + lo, channels 8*hi .. 8*hi+7 of a 16-channel step
    const int C8 = a.C >> 3;
    const f16x8* __restrict__ wv = reinterpret_cast<const f16x8*>(a.w);
    const int wrow = m0 + wm * 64 + lo;
    f16x8 wr[3][2][2];   // [tap][k-step][i]
    auto load_w = [&](int c) {
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    wr[t][ks][i] = wv[(long long)(t * C8 + c * (KC / 8) + ks * 2 + hi) * a.C + wrow + i * 32];
    };
    // B operand (activations): lane (lo, hi) reads position tap_base + wl*64 + j*32 + lo of 8-channel group ks*2 + hi
    int tap_base[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) tap_base[t] = span ? t * d : t * BL;
    const int b_off = (wl * 64 + lo) * 16;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto mfma_chunk = [&](const unsigned char* buf) {
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const unsigned char* xb = buf + ((ks * 2 + hi) * np + tap_base[t]) * 16 + b_off;
                f16x8 bx[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) bx[j] = *reinterpret_cast<const f16x8*>(xb + j * 32 * 16);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr[t][ks][i], bx[j], acc[i][j], 0, 0, 0);
            }
    };

    load_x(0);
    stage(sm);
    __syncthreads();
    // Every load is unconditional -- no branch around a load (the compiler would wait for every load in flight at the join);
    // out-of-row positions read a valid address and are cleared in stage(); the last iteration reloads the last chunk and
    // discards it.  Per chunk: the weights of c, the activations of c + 1, then the MFMAs of c, which wait for the weights
    // only (the 48 younger activation loads stay in flight: vmcnt(48)).  The weights' L2 latency is exposed once per chunk
    // and covered by the other workgroup on the CU; loading them a chunk ahead as well (a second register set) was tried and
    // spills at 256 VGPRs.
#pragma nounroll
    for (int c = 0; c < nchunks; ++c) {
        const int cn = c + 1 < nchunks ? c + 1 : c;
        load_w(c);
        __builtin_amdgcn_sched_barrier(0);   // all weight loads first (left alone, the scheduler sinks each next to its MFMA
        load_x(cn);                          // and exposes twelve L2 round trips per chunk one after the other)
        __builtin_amdgcn_sched_barrier(0);
        mfma_chunk(sm + (c & 1) * BUFB);
        if (c + 1 < nchunks) stage(sm + ((c + 1) & 1) * BUFB);
        __syncthreads();
    }

    if (a.flag && __any(bad) && lane == 0) atomicOr(a.flag, 1);

    // epilogue (fp32): C/D layout of 32x32 -- col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).  (Preloading the
    // residual into the accumulators before the K loop was tried: it pushes the kernel past 256 VGPRs and spills.)
    const float* rb = a.res + (long long)b * a.r_bs;
    float* yb = a.y + (long long)b * a.y_bs;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int l = l0 + wl * 64 + j * 32 + lo;
        if (l >= a.L) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                float v = acc[i][j][r];
                if (BIAS) v += a.bias[m];
                if (RES) v += rb[(long long)m * a.r_cs + l];
                yb[(long long)m * a.y_cs + l] = vfx_post(v, a.post_act, a.post_slope);
            }
    }
}

extern "C" int vfx_conv1d_f16(const vfx_tensor* x, const void* w_f16, const float* bias, const vfx_tensor* res,
                              const vfx_tensor* y, int B, int C, int L, int dilation, const vfx_act* act,
                              int32_t* range_flag, vfx_stream_t stream) {
    if (!x || !y || !w_f16 || !x->ptr || !y->ptr || B < 1 || L < 1 || dilation < 1) return VFX_EINVAL;
    if (B > 65535) return VFX_ENOTSUP;
    if (C != 128 && C != 256 && C != 512) return VFX_ENOTSUP;
    if (x->lstride != 1 || y->lstride != 1 || (res && (!res->ptr || res->lstride != 1))) return VFX_ENOTSUP;
    const int pre = act ? act->pre_act : VFX_PRE_NONE;
    const int post = act ? act->post_act : VFX_POST_NONE;
    if (pre != VFX_PRE_NONE && pre != VFX_PRE_LRELU) return VFX_ENOTSUP;
    if (post != VFX_POST_NONE && post != VFX_POST_LRELU && post != VFX_POST_LRELU_SNAKE) return VFX_ENOTSUP;
    ConvhArgs a;
    a.x = static_cast<const float*>(x->ptr); a.x_bs = x->bstride; a.x_cs = x->cstride;
    a.x_rows = x->rows;
    a.w = static_cast<const _Float16*>(w_f16);
    a.bias = bias;
    a.res = res ? static_cast<const float*>(res->ptr) : nullptr;
    a.r_bs = res ? res->bstride : 0; a.r_cs = res ? res->cstride : 0;
    a.y = static_cast<float*>(y->ptr); a.y_bs = y->bstride; a.y_cs = y->cstride;
    a.C = C; a.L = L; a.d = dilation;
    a.ntiles = (L + convh::BL - 1) / convh::BL;
    a.nm = C / convh::BM;
    a.pre_act = pre; a.pre_slope = act ? act->pre_slope : 0.f;
    a.post_act = post; a.post_slope = act ? act->post_slope : 0.f;
    a.flag = range_flag;
    const long long nblk = (long long)a.ntiles * a.nm;
    if (nblk > 0x7fffffffLL) return VFX_ENOTSUP;
    auto kern = bias ? (a.res ? convh_kernel<true, true> : convh_kernel<true, false>)
                     : (a.res ? convh_kernel<false, true> : convh_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk, 1, B), dim3(convh::NTHR), 0, (hipStream_t)stream, a);
    VFX_LAUNCHED();
    set_last_tile(convh::BM, convh::BL, TILE_CONVH);
    return vfx_last_error();
}
