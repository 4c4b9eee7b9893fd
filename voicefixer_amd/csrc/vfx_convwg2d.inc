// vfx_convwg2d.inc -- included by vfx_conv.hip after vfx_convwg.inc.
//
// convwg4s_kernel: the 3x3 convolutions of the ResUNet (restorer/modules.py:7-76, ConvBlockRes) as Winograd F(4,3) along the
// map ROWS with the three kernel COLUMNS sharing one staged tile (round 3).
//
// convwg4_kernel<.., NKX = 3> (round 2) treats the kernel columns kx = -1, 0, +1 as an outer part of its K loop: the
// "virtual chunk" (16 channels, kx) stages x[q + kx] afresh -- six tap loads, eval-BatchNorm, leaky ReLU, the B^T transform
// (13 VALU) and six LDS writes per element, THREE times for the same data shifted by one column.  The counters
// (profiles/r03_pmc_diag_winograd_kernels.txt) show what that costs where the contraction is short: UNet level 0 (Cout = 32,
// convwg_kernel<1,4,3,8>) issues 8.1 VALU and 1.3 memory-read instructions per MFMA and keeps the matrix pipe 57 % busy.
// Here a chunk is staged ONCE: V[plane][channel][column] with the tile's quads as columns, and the B fragment of kernel
// column kx is the same tile read one column to the left / right (on a pitch map "one column" is "one position", exactly
// as convw_kernel's NT = 9 instance reads its halo tile).  One barrier per 3 x (KC/2) x 6 MFMAs per wave (144 for KC = 16).
//
// No halo columns are needed: a tile is BQ = 64 or 128 consecutive quads and the map pitch P (a power of two) divides BQ,
// so a tile is a whole number of map rows.  The left neighbour of a row's first column is the previous row's pad column and
// the right neighbour of its last valid column is its own pad column -- structural zeros of the pitch-map layout
// (include/vfx_hip.h), staged as zeros after the activation like every tap outside the map.  Only the tile's own edges
// need care: LDS rows carry one extra zero column on each side (written once, never overwritten).
//
// Everything else follows convwg4_kernel: quad index space (q = 4P*blk + r is output 0 of quad blk*P + r: the four outputs
// are vertical neighbours), weights packing.pack_wino4_2d = [kx*6 + plane][Cin/8][Cout][8] straight from L2 as 16-byte
// A-operand vectors in two register sets (one 8-channel group ahead), staging
// woven between the MFMAs, per-row lengths (ragged batches), XCD-aware tile order with the channel blocks of a tile folded in.
// NOT from convwg4_kernel: bias and residual are added after the output transform (see the accumulators' start below).
// Instances: <2,2,16> (64 output channels x 64 quads, levels 1-4: P <= 64) and <1,4,8> (32 x 128, UNet level 0: Cout = 32).
// AFF (round 4): false = the launch has no pre-activation (the SECOND convolution of a ConvBlockRes: bn2 is folded into the first one's
// weights, whose epilogue applies the leaky ReLU), so the staging is the B^T transform alone -- a tap outside the map or in the pad
// column reads 0 through its out-of-range offset and needs neither the scale / shift, nor the leaky ReLU, nor the select that zeroes
// it AFTER the activation: 12 VALU operations per staged element instead of 36.  (The fp32 MFMA shares its issue cycles with the
// VALU on this chip, profiles/r04_convwg4_prologue_ab.txt: instructions that compute nothing are matrix-pipe time.)
// TWO (contractions longer than WG4S_TWO_CIN channels): a two-level sum.  One accumulator chain per plane adds 3 * Cin / 2
// MFMA results in sequence, and its rounding error grows with the square root of that count while a blocked fp32 sum's does
// not: the maximum error was 3.2 - 3.4 x a plain fp32 F(4,3) statement's at Cin = 384, 3.9 - 4.1 x at 512 and 4.7 x at 768 (the
// decoder's 768 -> 384), against the bound of 4 of tests/test_convwg4s_gpu.py; two-level it is 0.7 - 1.1 x.  So every 64 channels the accumulators are added to a second set and
// start again at zero (conv_taps_kernel's remedy).  The second set is 96 more registers, which do not fit two waves per SIMD:
// this instance runs one wave per SIMD, and only the launches that need it take it.
constexpr int WG4S_TWO_CIN = 384;
template <int WGM, int WGP, int KC, bool AFF = true, bool TWO = false>
__global__ __launch_bounds__(256, TWO ? 1 : 2) void convwg4s_kernel(const ConvArgs a) {
    static_assert(WGM * WGP == 4 && (KC == 8 || KC == 16), "four waves; 8- or 16-channel chunks");
    constexpr int NSTEP = KC / 2;                 // k-pair steps per kernel column and chunk
    constexpr int NG = KC / 8;                    // 8-channel weight groups per chunk
    constexpr int NSEQ = 3 * NG;                  // weight groups per chunk over the three kernel columns
    constexpr int BM = 32 * WGM, BQ = 32 * WGP;
    constexpr int ROW = BQ + 2;                   // LDS row: [zero][BQ quads][zero]
    constexpr int CG = 256 / BQ;                  // channel groups of the staging map
    constexpr int NSLOT = KC / CG;                // staged (channel, quad) elements per thread per chunk
    constexpr int PLANE = KC * ROW;
    constexpr int BUF = 6 * PLANE;
    static_assert(2 * NSLOT <= 3 * NSTEP, "two steps of staging per element must fit the chunk");
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lo = lane & 31, hi = lane >> 5;
    const int wm = wave / WGP, wp = wave % WGP;
    int bx = blockIdx.x;
    int mblk = blockIdx.y;
    if (a.xcd_chunk > 0) {                        // XCD-aware order, channel blocks of a tile folded in (see convwg_kernel)
        int k = bx >> 3;
        if (a.nph_fold > 1) {
            const int t = k / a.nph_fold;
            mblk = k - t * a.nph_fold;
            k = t;
        }
        bx = (bx & 7) * a.xcd_chunk + k;
        if (bx >= a.ntiles_l) return;
    }
    const int m0 = mblk * BM;
    const int b = blockIdx.z;
    const int d = a.wg_d;                         // = the map pitch P
    const int dsh = 31 - __builtin_clz(d);        // P is a power of two
    const int Lrow = a.x_rows ? __builtin_amdgcn_readfirstlane(a.x_rows[b]) : a.Lin;
    const int Q0 = bx * BQ;
    {
        const int nblk = (Lrow + 4 * d - 1) >> (dsh + 2);
        if (Q0 >= nblk * d) return;
    }
    const int xcs = (int)a.x_cs;
    auto quad_q = [&](int Q) {                    // first output of quad Q = blk*P + r
        const int blk = Q >> dsh;
        return (blk << (dsh + 2)) + (Q - (blk << dsh));
    };

    // ---- staging map: quad = tid % BQ, channel group = tid / BQ; element j = channel cg + j*CG
    const int sq = tid % BQ, cg = tid / BQ;
    int xvoff[6];                                 // vector offset of tap j (map row -1 .. +4 of the quad), out of range = padding
    bool xok[6];
    bool padcol;                                  // this element's column is the map's pad column
    {
        const int q = quad_q(Q0 + sq);
        padcol = (q & a.in_mask) == a.in_mask;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int p = q + (j - 1) * d;
            xok[j] = p >= 0 && p < Lrow && !padcol;
            xvoff[j] = xok[j] ? (cg * xcs + p) * 4 : VFX_W_OOB;
        }
    }
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.x) + (long long)b * a.x_bs, (short)0, 0x7fffffff, 0x00020000);
    const float slope = (a.pre_act == VFX_PRE_LRELU || a.pre_act == VFX_PRE_AFFINE_LRELU) ? a.pre_slope : 1.f;
    float* const aff = smem + 2 * BUF;            // [Cin][2] (scale, shift) of the eval-BatchNorm pre-activation (1, 0 without)
    {
        const bool affine = a.pre_act == VFX_PRE_AFFINE_LRELU;
        for (int c = tid; c < a.Cin; c += 256) {
            aff[2 * c] = affine ? a.pre_scale[c] : 1.f;
            aff[2 * c + 1] = affine ? a.pre_shift[c] : 0.f;
        }
        // the zero column on either side of every LDS row (both buffers); the staging writes columns 1 .. BQ only
        for (int r = tid; r < 2 * 6 * KC; r += 256) {
            smem[r * ROW] = 0.f;
            smem[r * ROW + ROW - 1] = 0.f;
        }
        __syncthreads();
    }
    float* const wbase = smem + cg * ROW + 1 + sq;

    float xv[NSLOT][6];
    auto x_load = [&](int chunk) {
        const int s0 = chunk * KC * xcs * 4;
#pragma unroll
        for (int j = 0; j < NSLOT; ++j)
#pragma unroll
            for (int t = 0; t < 6; ++t)
                xv[j][t] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xrsrc, xvoff[t], s0 + j * CG * xcs * 4, 0));
    };
    // BatchNorm scale / shift, leaky ReLU, zero outside the map and in the pad column (AFTER the activation), B^T
    auto x_transform = [&](int j, int chunk, float (&V)[6]) {
        float e[6];
        if constexpr (AFF) {
            const float2 ss = *reinterpret_cast<const float2*>(aff + 2 * (chunk * KC + cg + j * CG));
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const float u = fmaf(xv[j][t], ss.x, ss.y);
                e[t] = xok[t] ? fmaxf(u, u * slope) : 0.f;
            }
        } else {
#pragma unroll
            for (int t = 0; t < 6; ++t) e[t] = xv[j][t];   // (padding taps and the pad column read 0: out-of-range offsets)
        }
        const float s1 = fmaf(-4.f, e[2], e[4]), s2 = fmaf(-4.f, e[1], e[3]);
        const float s3 = e[4] - e[2], s4 = e[3] - e[1];
        V[0] = fmaf(4.f, e[0], fmaf(-5.f, e[2], e[4]));
        V[1] = s1 + s2;
        V[2] = s1 - s2;
        V[3] = fmaf(2.f, s4, s3);
        V[4] = fmaf(-2.f, s4, s3);
        V[5] = fmaf(4.f, e[1], fmaf(-5.f, e[3], e[5]));
    };
    auto x_write = [&](float* dst, int chunk) {
#pragma unroll
        for (int j = 0; j < NSLOT; ++j) {
            float V[6];
            x_transform(j, chunk, V);
#pragma unroll
            for (int k = 0; k < 6; ++k) dst[j * CG * ROW + k * PLANE] = V[k];
        }
    };

    // ---- A operands: [kx*6 + plane][Cin/8][Cout][8]; two register sets, one 8-channel group each
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wd), (short)0, 0x7fffffff, 0x00020000);
    const int avoff = ((m0 + wm * 32 + lo) * 8 + 4 * hi) * 4;
    const int gstride = a.Cout * 32;
    const int pstride = (a.CinPad >> 3) * gstride;
    float4 aw[2][6];
    auto a_load_one = [&](auto set_tag, int k, int goff) {
        constexpr int SET = decltype(set_tag)::value;
        const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, avoff, k * pstride + goff, 0);
        aw[SET][k] = make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
    };

    // ---- accumulators start at zero.  Bias and residual do NOT enter through them (convwg4_kernel's scheme, which this kernel
    // used before): an accumulator that starts at a residual or bias of order 1 rounds every product added to it at 2^-24 of
    // THAT value, so where the weights are small next to the skip connection (heavy-tailed gains) the convolution came out
    // 10 - 80 x less exact than an fp32 F(4,3) that adds them last -- and any solution of A^T m = residual couples the four
    // outputs of a quad (a small residual between large vertical neighbours was off by 2^-24 of the neighbours).
    // tests/test_convwg4s_gpu.py, profiles/convwg4s_parity.txt.  Both are added after the output transform (below), as
    // conv_taps_kernel does.
    const int row0 = m0 + wm * 32;
    f32x16 acc[6];
    // the issue block, in the order in which the results are consumed (see convwg4_kernel): taps of chunk 0, first A vectors
    x_load(0);
#pragma unroll
    for (int k = 0; k < 6; ++k) a_load_one(std::integral_constant<int, 0>{}, k, 0);
    __builtin_amdgcn_sched_barrier(0);            // (nothing that consumes a loaded value may be scheduled up into the issue block)
    auto acc_start = [&]() {
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;
    };

    // ---- B fragments: lane (column lo, k-half hi) of k-pair u of plane k for kernel column kx reads
    //      xs[k*PLANE + (2u + hi)*ROW + (1 + wp*32 + lo) + (kx - 1)]
    const int boffs = hi * ROW + wp * 32 + lo;

    // One chunk: 3 kernel columns x NSTEP k-pair steps x 6 MFMAs on the tile staged one chunk ago, with the staging of the
    // next chunk (element el during steps 2 el, 2 el + 1: transform + six LDS writes, then its six tap loads for the chunk
    // after next) and the A vectors of the next 8-channel group (all six in the first step of each group) woven in.
    // PAR: parity of the chunk -- with one group per kernel column (KC = 8) a chunk has an odd number of groups and the
    // register set a group lives in alternates from chunk to chunk.
    auto mma_chunk = [&](auto par_tag, const float* xs, float* wdst, int cst, int cld, int ccur, int cnext) {
        constexpr int PAR = decltype(par_tag)::value;
        const float* bp = xs + boffs;
        float bf[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) bf[k] = bp[k * PLANE];
        const int xs0 = cld * KC * xcs * 4;
        const int acur = NG * ccur * gstride, anext = NG * cnext * gstride;
        float V[6];
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
            for (int u = 0; u < NSTEP; ++u) {
                const int s = kx * NSTEP + u;                 // step of the chunk
                const int el = s >> 1, ph = s & 1;
                const int gs = kx * NG + (u >> 2);            // weight group of this step within the chunk
                const bool newgrp = (u & 3) == 0;
                // the group after gs: same chunk, or group 0 of the next one
                const int gn = gs + 1;
                const int goff_next = gn < NSEQ ? (gn / NG) * 6 * pstride + (gn % NG) * gstride + acur : anext;
                const bool last_step = kx == 2 && u == NSTEP - 1;
                const int un = u + 1 < NSTEP ? u + 1 : 0, kxn = u + 1 < NSTEP ? kx : kx + 1;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    if (el < NSLOT) {
                        if (ph == 0 && k == 0) x_transform(el, cst, V);
                        if (ph == 0) wdst[el * CG * ROW + k * PLANE] = V[k];
                        if (ph == 1)
                            xv[el][k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xrsrc, xvoff[k], xs0 + el * CG * xcs * 4, 0));
                    }
                    if (newgrp) {
                        if (((gs + 1 + PAR * NSEQ) & 1) == 0) a_load_one(std::integral_constant<int, 0>{}, k, goff_next);
                        else a_load_one(std::integral_constant<int, 1>{}, k, goff_next);
                    }
                    const float4 av4 = ((gs + PAR * NSEQ) & 1) ? aw[1][k] : aw[0][k];
                    const int kk = u & 3;
                    const float av = kk == 0 ? av4.x : (kk == 1 ? av4.y : (kk == 2 ? av4.z : av4.w));
                    acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[k], acc[k], 0, 0, 0);
                    if (!last_step) bf[k] = bp[k * PLANE + un * 2 * ROW + kxn];
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    };

    const int S = a.Cin / KC;                     // chunks (host: Cin % (2 * KC) == 0, so S is even)
    x_write(wbase, 0);
    x_load(S > 1 ? 1 : 0);
    __builtin_amdgcn_sched_barrier(0);
    acc_start();
    f32x16 tot[TWO ? 6 : 1];
    if constexpr (TWO) {
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[k][r] = 0.f;
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < S; s += 2) {
        // chunk s (LDS buffer 0): stages chunk s+1 into buffer 1, loads x of chunk s+2
        mma_chunk(std::integral_constant<int, 0>{}, smem, wbase + BUF, s + 1, min(s + 2, S - 1), s, min(s + 1, S - 1));
        __syncthreads();
        // chunk s+1 (buffer 1): stages chunk s+2 into buffer 0, loads x of chunk s+3
        mma_chunk(std::integral_constant<int, 1>{}, smem + BUF, wbase, min(s + 2, S - 1), min(s + 3, S - 1), s + 1, min(s + 2, S - 1));
        __syncthreads();
        if constexpr (TWO) {
            if (((s + 2) * KC) % 64 == 0) {       // 64 channels done: close the partial sum (the last one below)
#pragma unroll
                for (int k = 0; k < 6; ++k)
#pragma unroll
                    for (int r = 0; r < 16; ++r) tot[k][r] += acc[k][r];
                acc_start();
            }
        }
    }
    if constexpr (TWO) {
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[k][r] += tot[k][r];
    }

    // ---- output transform, bias, residual, activation, stores; the outputs of a quad in the map's pad column are written as zero
    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(
        a.y + (long long)b * a.y_bs, (short)0, 0x7fffffff, 0x00020000);
    const int ycs4 = (int)a.y_cs * 4;
    const int post = a.post_act;
    const float ps = a.post_slope;
    int yv[4];
    bool keep;
    {
        const int q = quad_q(Q0 + wp * 32 + lo);
#pragma unroll
        for (int i = 0; i < 4; ++i) yv[i] = q + i * d < Lrow ? (4 * hi * (int)a.y_cs + q + i * d) * 4 : VFX_W_OOB;
        keep = (q & a.out_mask) != a.out_mask;
    }
    // the residual of the lane's 16 rows x 4 outputs, all fetched before the first store: res may be y (the in-place update
    // of a ConvBlockRes), and a lane reads exactly the elements it later writes
    f32x16 rres[4];
    __builtin_amdgcn_sched_barrier(0);            // (after the last chunk: 64 more live registers do not fit next to the A operands)
    u32x4 bq[4];                                  // bias of rows row0 + 4 hi + 8 g + e (0 without: out-of-range offset)
    {
        const __amdgpu_buffer_rsrc_t brsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(a.bias ? a.bias : a.x), (short)0, 0x7fffffff, 0x00020000);
        const int bvoff = a.bias ? (row0 + 4 * hi) * 4 : VFX_W_OOB;
#pragma unroll
        for (int g = 0; g < 4; ++g) bq[g] = __builtin_amdgcn_raw_buffer_load_b128(brsrc, bvoff, g * 32, 0);
    }
    if (a.res) {
        const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(a.res) + (long long)b * a.r_bs, (short)0, 0x7fffffff, 0x00020000);
        const int cs4 = (int)a.r_cs * 4;
        const int q = quad_q(Q0 + wp * 32 + lo);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rvo = q + i * d < Lrow ? (4 * hi * (int)a.r_cs + q + i * d) * 4 : VFX_W_OOB;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                rres[i][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, rvo, (row0 + (r & 3) + 8 * (r >> 2)) * cs4, 0));
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) rres[i][r] = 0.f;
    }
    auto outs = [&](int r, float (&y)[4]) {
        const float p12 = acc[1][r] + acc[2][r], m12 = acc[1][r] - acc[2][r];
        const float p34 = acc[3][r] + acc[4][r], m34 = acc[3][r] - acc[4][r];
        const u32x4 b4 = bq[r >> 2];
        const float bb = __uint_as_float((r & 3) == 0 ? b4.x : ((r & 3) == 1 ? b4.y : ((r & 3) == 2 ? b4.z : b4.w)));
        y[0] = (((acc[0][r] + p12) + p34) + bb) + rres[0][r];
        y[1] = (fmaf(2.f, m34, m12) + bb) + rres[1][r];
        y[2] = (fmaf(4.f, p34, p12) + bb) + rres[2][r];
        y[3] = ((fmaf(8.f, m34, m12) + acc[5][r]) + bb) + rres[3][r];
    };
    if (post == VFX_POST_NONE) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int soff = (row0 + (r & 3) + 8 * (r >> 2)) * ycs4;
            float y[4];
            outs(r, y);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(keep ? y[i] : 0.f), yrsrc, yv[i], soff, 0);
        }
    } else if (post == VFX_POST_LRELU) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int soff = (row0 + (r & 3) + 8 * (r >> 2)) * ycs4;
            float y[4];
            outs(r, y);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(keep ? fmaxf(y[i], y[i] * ps) : 0.f), yrsrc, yv[i], soff, 0);
        }
    } else {
#pragma unroll 1
        for (int r = 0; r < 16; ++r) {
            const int soff = (row0 + (r & 3) + 8 * (r >> 2)) * ycs4;
            float y[4];
            outs(r, y);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(keep ? vfx_post(y[i], post, ps) : 0.f), yrsrc, yv[i], soff, 0);
        }
    }
}

template <int WGM, int WGP, int KC, bool AFF, bool TWO>
static int launch_wg4s_aff(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t s) {
    return vfx_launch<convwg4s_kernel<WGM, WGP, KC, AFF, TWO>>(grid, dim3(256), lds, s, a);
}

template <int WGM, int WGP, int KC>
static int launch_wg4s_one(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t s) {
    if (a.Cin > WG4S_TWO_CIN)
        return a.pre_act == VFX_PRE_NONE ? launch_wg4s_aff<WGM, WGP, KC, false, true>(a, grid, lds, s)
                                         : launch_wg4s_aff<WGM, WGP, KC, true, true>(a, grid, lds, s);
    return a.pre_act == VFX_PRE_NONE ? launch_wg4s_aff<WGM, WGP, KC, false, false>(a, grid, lds, s)
                                     : launch_wg4s_aff<WGM, WGP, KC, true, false>(a, grid, lds, s);
}

// 3x3 convolution on a pitch map on convwg4s_kernel (weights packing.pack_wino4_2d); same contract as
// try_launch_convwg4_2d, which it precedes.  VFX_ENOTSUP -> the next kernel in the chain.
static int try_launch_convwg4s_2d(ConvArgs a, const vfx_tensor* x, int P, const float* wg4, hipStream_t stream) {
    static const bool off = (VFX_DEV_ENV("VFX_WINO") && atoi(VFX_DEV_ENV("VFX_WINO")) == 0) ||
                            (VFX_DEV_ENV("VFX_WINO4") && atoi(VFX_DEV_ENV("VFX_WINO4")) == 0) ||
                            (VFX_DEV_ENV("VFX_WINO4_2D") && atoi(VFX_DEV_ENV("VFX_WINO4_2D")) == 0) ||
                            (VFX_DEV_ENV("VFX_WINO4S") && atoi(VFX_DEV_ENV("VFX_WINO4S")) == 0);   // development
    if (off || !wg4 || !vfx_aligned16(wg4)) return VFX_ENOTSUP;
    if (a.pad_mode != VFX_PAD_ZERO || a.in_mask != P - 1 || a.out_mask != P - 1 || (P & (P - 1)) != 0) return VFX_ENOTSUP;
    if (a.pre_act != VFX_PRE_NONE && a.pre_act != VFX_PRE_AFFINE_LRELU) return VFX_ENOTSUP;
    if (a.pre_act == VFX_PRE_AFFINE_LRELU && !(a.pre_slope >= 0.f && a.pre_slope <= 1.f)) return VFX_ENOTSUP;   // lrelu = max(v, slope v)
    if (a.post_act == VFX_POST_LRELU && !(a.post_slope >= 0.f && a.post_slope <= 1.f)) return VFX_ENOTSUP;
    if (!plain_output_map(a, 1, 0) || a.y_ls != 1 || a.Lq != a.Lin) return VFX_ENOTSUP;   // (one phase at offset 0: the caller's 3x3)
    if (a.res && a.r_ls != 1) return VFX_ENOTSUP;
    if (a.Cout % 32 != 0 || a.Cin != a.CinPad) return VFX_ENOTSUP;
    const bool narrow = a.Cout % 64 != 0;         // 32 channels x 128 quads, 8-channel chunks (UNet level 0)
    const int BQ = narrow ? 128 : 64, kc = narrow ? 8 : 16;
    if (a.Cin % (2 * kc) != 0 || P > BQ) return VFX_ENOTSUP;
    if (!offsets_fit31(((long long)a.Cin * a.x_cs + a.Lin) * 4) || !offsets_fit31(((long long)a.Cout * a.y_cs + a.Lout) * 4) ||
        (a.res && !offsets_fit31(((long long)a.Cout * a.r_cs + a.Lout) * 4)))
        return VFX_ENOTSUP;
    if (!offsets_fit31(18ll * (a.CinPad >> 3) * a.Cout * 32)) return VFX_ENOTSUP;   // (the transformed weights)
    const int d = P;
    const long long nquads = ((long long)a.Lin + 4 * d - 1) / (4 * d) * d;
    const int ntiles = (int)((nquads + BQ - 1) / BQ);
    const int gy = a.Cout / (narrow ? 32 : 64);
    if ((long long)ntiles * gy * a.B < 384) return VFX_ENOTSUP;   // the deep levels keep the small tiles / split-K
    a.wd = wg4;
    a.wg_d = d;
    a.x_guard = 0;
    a.tab = nullptr;
    a.stagger = 0; a.stagger_wgs = 0;
    if (!a.res) { a.r_bs = a.x_bs; a.r_cs = a.x_cs; }
    const size_t lds = (2ull * 6 * kc * (BQ + 2) + 2ull * a.Cin) * sizeof(float);
    dim3 grid(convw_grid_x(a, ntiles), gy, a.B);
    convwg_fold_blocks(a, grid, gy);
    set_last_tile(narrow ? 32 : 64, 4 * BQ % 1000, TILE_WG4S);
    return narrow ? launch_wg4s_one<1, 4, 8>(a, grid, lds, stream) : launch_wg4s_one<2, 2, 16>(a, grid, lds, stream);
}
