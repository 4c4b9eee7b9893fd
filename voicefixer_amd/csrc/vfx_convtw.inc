// vfx_convtw.inc -- included by vfx_conv.hip after vfx_convwg4x.inc.
//
// convtw_kernel (round 6): the polyphase ConvTranspose1d of the vocoder's UpsampleNet (kernel 2s, stride s,
// voicefixer/vocoder/model/modules.py:449-459,501-528) as Winograd F(3,2) along the INPUT axis, exact-fp32 MFMA.
//
// Every output phase r of the transposed convolution is a TWO-tap correlation over the input (SURVEY.md a15):
//     out[q s + r - pad] = w[r + s] x[q - 1] + w[r] x[q],      q = 0 .. Lin   (x[-1] = x[Lin] = 0)
// so three consecutive q of one phase share four inputs, d_j = x[3T - 1 + j]:
//     V = B^T d:  V0 = d0 - d2, V1 = d1 + d2, V2 = d2 - d1, V3 = d3 - d1            (additions only)
//     U = G g:    U0 = g0, U1 = (g0 + g1) / 2, U2 = (g0 - g1) / 2, U3 = g1            (g0 = w[r + s], g1 = w[r]; host, float64)
//     m_k = sum_ci U_k V_k;   y(3T) = m0 + m1 + m2,  y(3T + 1) = m1 - m2,  y(3T + 2) = m1 + m2 + m3
// FOUR products per three outputs where the direct sum (convw_kernel<.., NT = 2>) has six: 2/3 of the fp32 MFMAs, transform constants
// 1 and 1/2 only (rounding as the direct sum's).  V does not depend on the phase, so the s phases are ONE GEMM with s Cout rows, row
// c s + r = (channel c, phase r), phase fastest: the s phases of a channel's output line come from neighbouring rows of one wave (of two
// waves of one workgroup where a wave boundary cuts a channel), and the epilogue writes the line once, as 16-byte vectors, where one
// phase per workgroup wrote dwords s apart and every 32-byte sector s times (round 13, profiles/r13_convtw_rows_ab.txt; work order and
// epilogue: see the kernel).
// Structure: convwg4_kernel's (vfx_convwg.inc) -- a workgroup owns 32 WGP consecutive triples x 32 WGM consecutive rows, a
// wave 32 rows x 32 triples x 4 planes (64 accumulators); taps as dword buffer loads with one vector offset per tap (outside the row:
// out-of-range offset = the zero padding, per-row lengths cost nothing), B^T, four planes to LDS [plane][channel][triple], double
// buffered, 16 channels per chunk, the staging of chunk c + 1 woven between the MFMAs of chunk c; weights as 16-byte A vectors straight
// from L2 ([plane][Cin/8][s Cout][8], packing.pack_wino32_tr), two register sets.  All four planes start at zero; the bias (of the row's channel) is
// added after the output transform (see the epilogue).  Strides 1 .. 32.  No pre- / post-activation (the UpsampleNet has none: the x + sin x in front of it
// is the producing kernel's epilogue); anything else stays on convw_kernel.
template <int WGM, int WGP>
__global__ __launch_bounds__(256, 2) void convtw_kernel(const ConvArgs a) {
    static_assert(WGM * WGP == 4, "four waves");
    constexpr int KC = 16, NSTEP = KC / 2, NPL = 4;
    constexpr int BM = 32 * WGM, BT = 32 * WGP;
    constexpr int CG = 256 / BT;                  // channel groups of the staging map
    constexpr int NSLOT = KC / CG;                // staged (channel, triple) elements per thread per chunk: 2 (<4,1>) or 4 (<2,2>)
    constexpr int SPAN = NSTEP / NSLOT;           // k-pair steps an element's staging is spread over: 4 or 2
    constexpr int PLANE = KC * BT;
    constexpr int BUF = NPL * PLANE;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lo = lane & 31, hi = lane >> 5;
    const int wm = wave / WGP, wp = wave % WGP;
    // Work order (the workgroups that run side by side on an XCD are a contiguous piece of it), chosen per launch by the host:
    //  * a.tile_lo == 0: (row block, tile), TILE fastest -- for layers whose transformed weights (16 s Cin Cout bytes: 59 MB at
    //    up1, 15 MB at up2) do not fit an XCD's 4 MB L2.  What a workgroup streams is mostly weights (four planes x Cin x 128 rows = 2 MB at
    //    up1 against 0.4 MB of input taps), so neighbours share their row block and its planes stay in L2 while the tiles
    //    stream past.  Phase fastest there shared the small operand and re-fetched the large one: 18.5 GB of L2 misses per launch for
    //    2.2 GB of tensors (profiles/r06_pmc_hbm_traffic_bench_b32.json of the first form), up1 3.51 -> 2.93 ms, up2 6.04 -> 5.58;
    //  * a.tile_lo == 1: (tile, row block), ROW BLOCK fastest -- where all rows' planes fit L2 together (1.6 MB at up3, 0.4 MB at
    //    up4): the row blocks of a tile side by side share its taps as well (tile fastest there: up3 3.88 -> 4.36 ms, up4 3.91 -> 5.0).
    //  profiles/r06_convtw_order_ab.txt
    const int s = a.nph_fold, gy = a.tpw;        // gy: row blocks of the s Cout rows
    int lin = blockIdx.x;
    if (a.xcd_chunk > 0) lin = (lin & 7) * a.xcd_chunk + (lin >> 3);
    if (lin >= a.ntiles_l * gy) return;
    int mblk, tile;
    if (a.tile_lo == 0) {
        tile = lin % a.ntiles_l; mblk = lin / a.ntiles_l;
    } else {
        mblk = lin % gy; tile = lin / gy;
    }
    const int b = blockIdx.z;
    const int Lrow = a.x_rows ? __builtin_amdgcn_readfirstlane(a.x_rows[b]) : a.Lin;   // inputs of this row; q = 0 .. Lrow
    const int T0 = tile * BT;
    if (3 * T0 > Lrow) return;
    const int xcs = (int)a.x_cs;
    const int S = a.Cin / KC;                     // chunks (host: even, >= 2)

    // ---- staging map and tap offsets
    const int st = tid % BT, cg = tid / BT;
    int xvoff[4];
    {
        const int p0 = 3 * (T0 + st) - 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) xvoff[j] = (p0 + j >= 0 && p0 + j < Lrow) ? (cg * xcs + p0 + j) * 4 : VFX_W_OOB;
    }
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.x) + (long long)b * a.x_bs, (short)0, 0x7fffffff, 0x00020000);
    float* const wbase = smem + cg * BT + st;
    float xv[NSLOT][4];
    auto x_load_part = [&](int j, int t, int s0) {
        xv[j][t] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xrsrc, xvoff[t], s0 + j * CG * xcs * 4, 0));
    };
    auto x_load = [&](int chunk) {
        const int s0 = chunk * KC * xcs * 4;
#pragma unroll
        for (int j = 0; j < NSLOT; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) x_load_part(j, t, s0);
    };
    auto x_transform = [&](int j, float (&V)[4]) {
        V[0] = xv[j][0] - xv[j][2];
        V[1] = xv[j][1] + xv[j][2];
        V[2] = xv[j][2] - xv[j][1];
        V[3] = xv[j][3] - xv[j][1];
    };

    // ---- A operands: [4 planes][Cin/8][s Cout][8]; two register sets, one 8-channel group each
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wd), (short)0, 0x7fffffff, 0x00020000);
    const int row0 = mblk * BM + wm * 32;
    const int avoff = ((row0 + lo) * 8 + 4 * hi) * 4;
    const int gstride = s * a.Cout * 32;          // bytes per (plane, 8-channel group)
    const int pstride = (a.CinPad >> 3) * gstride;
    float4 aw[2][NPL];
    auto a_load_one = [&](auto set_tag, int k, int grp) {
        constexpr int SET = decltype(set_tag)::value;
        const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, avoff, k * pstride + grp * gstride, 0);
        aw[SET][k] = make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;

    // ---- rows to (channel, phase): row R = row0 + j of the wave is channel R / s, phase R % s -- wave-uniform, so scalar work; the
    // quotient as the high half of R x ceil(2^32 / s) (a.tw_rdiv, from the host: exact while R s < 2^32).  A lane's register row r is
    // row (r & 3) + 8 (r >> 2) + 4 hi of the wave
    const int s1mask = s == 1 ? -1 : 0;           // (s = 1: ceil(2^32 / s) does not fit, tw_rdiv = 0 and the channel is R itself)
    auto row_cp = [&](int R, int& c, int& p) {
        c = (int)__umulhi((unsigned)R, a.tw_rdiv) + (R & s1mask);
        p = R - c * s;
    };
    // the issue block: taps of chunk 0, first A vectors (nothing but loads)
    x_load(0);
#pragma unroll
    for (int k = 0; k < NPL; ++k) a_load_one(S0{}, k, 0);
    __builtin_amdgcn_sched_barrier(0);

    f32x16 acc[NPL];
    const int boffs = hi * BT + wp * 32 + lo;
    // one chunk: 8 k-pair steps x 4 MFMAs; element el of the thread is staged during steps SPAN el (transform + four LDS writes) and
    // SPAN el + SPAN / 2 (its four tap loads for the chunk after next); A vectors of the next 8-channel group in the first step of each group
    auto mma_chunk = [&](auto first_tag, const float* xs, float* wdst, int xchunk, int agrp0) {
        constexpr bool FIRST = decltype(first_tag)::value;
        const float* bp = xs + boffs;
        const int agrp1 = min(agrp0 + 1, 2 * S - 1), agrp2 = min(agrp0 + 2, 2 * S - 1);
        float bf[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) bf[k] = bp[k * PLANE];
        const int xs0 = xchunk * KC * xcs * 4;
        float V[4];
#pragma unroll
        for (int u = 0; u < NSTEP; ++u) {
            const int el = u / SPAN, ph = u % SPAN;
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                if (ph == 0 && k == 0) x_transform(el, V);
                if (ph == 0) wdst[el * CG * BT + k * PLANE] = V[k];
                if (ph == SPAN / 2) x_load_part(el, k, xs0);
                if (u == 0) a_load_one(S1{}, k, agrp1);
                if (u == 4) a_load_one(S0{}, k, agrp2);
                const float4 av4 = (u < 4) ? aw[0][k] : aw[1][k];
                const int kk = u & 3;
                const float av = kk == 0 ? av4.x : (kk == 1 ? av4.y : (kk == 2 ? av4.z : av4.w));
                if (FIRST && u == 0) {
                    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[k], zero16, 0, 0, 0);
                } else {
                    acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[k], acc[k], 0, 0, 0);
                }
                if (u < NSTEP - 1) bf[k] = bp[k * PLANE + (u + 1) * 2 * BT];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    {   // chunk 0 to LDS, chunk 1 in flight
#pragma unroll
        for (int j = 0; j < NSLOT; ++j) {
            float V[4];
            x_transform(j, V);
#pragma unroll
            for (int k = 0; k < NPL; ++k) wbase[j * CG * BT + k * PLANE] = V[k];
        }
        x_load(1);
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    mma_chunk(std::true_type{}, smem, wbase + BUF, 2 < S ? 2 : S - 1, 0);   // (the first pair of chunks peeled: chunk 0 starts the accumulators)
    __syncthreads();
    mma_chunk(std::false_type{}, smem + BUF, wbase, 3 < S ? 3 : S - 1, 2);
    __syncthreads();
#pragma unroll 1
    for (int c = 2; c < S; c += 2) {
        mma_chunk(std::false_type{}, smem, wbase + BUF, min(c + 2, S - 1), 2 * c);
        __syncthreads();
        mma_chunk(std::false_type{}, smem + BUF, wbase, min(c + 3, S - 1), 2 * c + 2);
        __syncthreads();
    }

    // ---- output transform and stores: row (c, r), q = 3T + i  ->  y[c][q s + r - pad], valid for 0 <= o < s Lrow (which implies q <= Lrow).
    // The whole channels of the wave's 32 rows go through LDS, laid out [channel][q s + r] as in y, and leave as 16-byte vectors
    // (unaligned dwordx4, legal on gfx950: a channel's span starts pad dwords before a multiple of s): every output line is written once,
    // by one wave, in 12 vector stores per lane and tile where phase-strided dwords took 48.  Half a wave tile (16 triples, 6 KB) at a
    // time, in a wave-private piece of the staging buffers (free after the K loop's last barrier): no workgroup barrier.  The rows of a
    // channel shared with another wave (jf rows at the top, 32 - jt at the bottom; none where s divides 32) stay dword stores: their
    // neighbours in the line come from the other wave's epilogue at about the same time, L2 merges them before write-back.  Range
    // checks only in waves that hold q = 0 or q >= Lrow; there a vector that straddles 0 or s Lrow goes dword by dword.
    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(
        a.y + (long long)b * a.y_bs, (short)0, 0x7fffffff, 0x00020000);
    const int ycs = (int)a.y_cs, pad = a.w_ooff0;    // (w_ooff0: the padding of the transposed convolution)
    const int q0 = 3 * (T0 + wp * 32 + lo);
    const int qs4[3] = {q0 * s * 4, (q0 + 1) * s * 4, (q0 + 2) * s * 4};
    int rowe = row0;
    asm volatile("" : "+s"(rowe));               // (decoded again here, not carried in 64 SGPRs through the K loop)
    const bool edge = __any(q0 == 0 || q0 + 2 >= Lrow);
    constexpr int HT = 16;
    float* const lt = smem + wave * (32 * 3 * HT);
    int cA, pA, nfull, rem;
    row_cp(rowe, cA, pA);
    const int jf = pA == 0 ? 0 : s - pA;
    const int cf = pA == 0 ? cA : cA + 1;
    row_cp(32 - jf, nfull, rem);
    const int jt = 32 - rem;
    const int cspan = 3 * HT * s, sL = s * Lrow;
    // The bias of each register row's channel (a gather), added AFTER the output transform in both paths below: as a start value of plane 1
    // it would round every partial sum of that plane at the size of the bias (up to 15 x the error of a plain fp32 F(3,2) per output on
    // channels with a small weight-norm gain, tests/test_convtw_gpu.py).  Gathered here, not before the K loop: 16 registers less through it.
    const __amdgpu_buffer_rsrc_t brsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.bias ? a.bias : a.x), (short)0, 0x7fffffff, 0x00020000);
    float bv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int k = (r & 3) + 8 * (r >> 2);
        int c0, p0, c1, p1;
        row_cp(rowe + k, c0, p0);
        row_cp(rowe + k + 4, c1, p1);
        const int bvoff = a.bias ? (hi ? c1 : c0) * 4 : VFX_W_OOB;
        bv[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(brsrc, bvoff, 0, 0));
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {               // the shared channels' rows
        const int k = (r & 3) + 8 * (r >> 2);
        const bool part0 = k < jf || k >= jt, part1 = k + 4 < jf || k + 4 >= jt;
        if (part0 || part1) {
            int c0, p0, c1, p1;
            row_cp(rowe + k, c0, p0);
            row_cp(rowe + k + 4, c1, p1);
            const float p12 = acc[1][r] + acc[2][r];
            const float yo[3] = {acc[0][r] + p12 + bv[r], acc[1][r] - acc[2][r] + bv[r], p12 + acc[3][r] + bv[r]};
            const int rowb = hi ? (c1 * ycs + p1 - pad) * 4 : (c0 * ycs + p0 - pad) * 4;
            const int o0 = hi ? p1 - pad : p0 - pad;
            const bool mine = hi ? part1 : part0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int o = (q0 + i) * s + o0;
                const int yv = (mine && o >= 0 && o < sL) ? rowb + qs4[i] : VFX_W_OOB;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(yo[i]), yrsrc, yv, 0, 0);
            }
        }
    }
    const int nv = nfull * (cspan >> 2);         // 16-byte vectors per pass
    const float inv_cv = 1.0f / (float)(cspan >> 2);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int tl = lo - HT * h;
        if (tl >= 0 && tl < HT) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = (r & 3) + 8 * (r >> 2);
                int c0, p0, c1, p1;
                row_cp(rowe + k, c0, p0);
                row_cp(rowe + k + 4, c1, p1);
                const bool whole = hi ? (k + 4 >= jf && k + 4 < jt) : (k >= jf && k < jt);
                if (whole) {
                    const float p12 = acc[1][r] + acc[2][r];
                    float* const d = lt + (hi ? (c1 - cf) * cspan + p1 : (c0 - cf) * cspan + p0) + 3 * tl * s;
                    d[0] = acc[0][r] + p12 + bv[r];
                    d[s] = acc[1][r] - acc[2][r] + bv[r];
                    d[2 * s] = p12 + acc[3][r] + bv[r];
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int os = 3 * (T0 + wp * 32 + HT * h) * s - pad;    // y index of a channel's first dword of this pass
        for (int v = lane; v < nv; v += 64) {
            const int cl = fast_div(v, cspan >> 2, inv_cv);
            const int w4 = (v - cl * (cspan >> 2)) * 4;
            const float4 d = *reinterpret_cast<const float4*>(lt + cl * cspan + w4);
            const u32x4 u = {__float_as_uint(d.x), __float_as_uint(d.y), __float_as_uint(d.z), __float_as_uint(d.w)};
            const int o4 = os + w4;
            const int yb = ((cf + cl) * ycs + o4) * 4;
            if (!edge) {
                __builtin_amdgcn_raw_buffer_store_b128(u, yrsrc, yb, 0, 0);
            } else {
                const bool all4 = o4 >= 0 && o4 + 3 < sL;
                __builtin_amdgcn_raw_buffer_store_b128(u, yrsrc, all4 ? yb : VFX_W_OOB, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool one = !all4 && o4 + j >= 0 && o4 + j < sL;
                    __builtin_amdgcn_raw_buffer_store_b32(u[j], yrsrc, one ? yb + 4 * j : VFX_W_OOB, 0, 0);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

template <int WGM, int WGP>
static int launch_convtw(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t s) {
    return vfx_launch<convtw_kernel<WGM, WGP>>(grid, dim3(256), lds, s, a);
}

// vfx_convtr1d_f32 on convtw_kernel: w32 = vfx_act.w_wino4 of this entry point (packing.pack_wino32_tr).  VFX_ENOTSUP = not this launch.
// It runs before launch_conv validates the call, so whatever launch_conv rejects (no tap slabs, Cin or Cout <= 0) is declined here too.
static int try_launch_convtw(const vfx_tensor* x, const float* w_packed, const float* w32, const float* bias, const vfx_tensor* y, int B,
                             int Cin, int Cout, int Lin, int stride, const vfx_act* act, hipStream_t stream) {
    static const bool off = VFX_DEV_ENV("VFX_CONVTW") && atoi(VFX_DEV_ENV("VFX_CONVTW")) == 0;   // development: A/B against convw_kernel
    if (off || !w_packed || !w32 || !vfx_aligned16(w32) || !x || !y || !x->ptr || !y->ptr) return VFX_ENOTSUP;
    if (act && (act->pre_act != VFX_PRE_NONE || act->post_act != VFX_POST_NONE || act->math != VFX_MATH_F32)) return VFX_ENOTSUP;
    // (stride > 32: a wave's 32 rows would lie inside one channel -- the epilogue's split into whole and shared channels, 32 - jf rows from
    // the first whole one, assumes s <= 32)
    if (Cin < 32 || Cout <= 0 || Cin % 32 != 0 || Cout % 64 != 0 || B <= 0 || B > 65535 || Lin < 1 || stride < 1 || stride > 32) return VFX_ENOTSUP;
    if (x->lstride != 1 || y->lstride != 1 || (bias && !vfx_aligned16(bias))) return VFX_ENOTSUP;
    if (!offsets_fit31(((long long)Cin * x->cstride + Lin) * 4) || !offsets_fit31(((long long)Cout * y->cstride + (long long)stride * Lin) * 4))
        return VFX_ENOTSUP;
    if (!offsets_fit31(4ll * stride * (Cin >> 3) * Cout * 32) || (long long)stride * stride * Cout >= (1ll << 32)) return VFX_ENOTSUP;   // (tw_rdiv's range)
    const bool wide = Cout % 128 == 0;
    const int BT = wide ? 32 : 64;
    const int ntriples = (Lin + 1 + 2) / 3;
    const int ntiles = (ntriples + BT - 1) / BT;
    const int gy = Cout / (wide ? 128 : 64);
    const long long nwg = (long long)ntiles * stride * gy;
    if (nwg * B < 512 || nwg >= (1ll << 30)) return VFX_ENOTSUP;
    ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x = (const float*)x->ptr;
    a.wd = w32;
    a.bias = bias;
    a.y = (float*)y->ptr;
    a.B = B; a.Cin = Cin; a.CinPad = Cin; a.Cout = Cout;
    a.Lin = Lin; a.Lq = Lin + 1; a.Lout = stride * Lin;
    a.x_bs = x->bstride; a.x_cs = x->cstride;
    a.x_rows = x->rows;
    a.y_bs = y->bstride; a.y_cs = y->cstride; a.y_ls = 1;
    a.nph_fold = stride;
    a.tpw = stride * gy;                          // row blocks of the s Cout rows
    a.w_ooff0 = stride / 2 + stride % 2;          // pad
    a.tw_rdiv = (unsigned)(((1ull << 32) + stride - 1) / stride);   // (stride 1: 0, see the kernel)
    a.ntiles_l = ntiles;
    a.tile_lo = 16ll * stride * Cin * Cout <= (3ll << 20) ? 1 : 0;     // row block fastest while all rows' planes fit an XCD's L2 together, else tile fastest
    if (VFX_DEV_ENV("VFX_CONVTW_ORDER")) a.tile_lo = atoi(VFX_DEV_ENV("VFX_CONVTW_ORDER")) == 0 ? 1 : 0;   // development: 0 = row block fastest, 1 = tile fastest everywhere
    a.xcd_chunk = nwg >= 64 ? (int)((nwg + 7) / 8) : 0;
    const dim3 grid(a.xcd_chunk > 0 ? (unsigned)(8 * a.xcd_chunk) : (unsigned)nwg, 1, B);
    const size_t lds = (wide ? 4ull * 32 * 48 : 2ull * 4 * 16 * BT) * sizeof(float);   // staging buffers 2 x 4 x 16 x BT floats; epilogue: 4 waves x 6 KB (more, where BT = 32)
    set_last_tile(wide ? 128 : 64, 3 * BT, TILE_CONVTW);
    return wide ? launch_convtw<4, 1>(a, grid, lds, stream) : launch_convtw<2, 2>(a, grid, lds, stream);
}
