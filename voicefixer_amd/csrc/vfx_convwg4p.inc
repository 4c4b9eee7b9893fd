// vfx_convwg4p.inc -- included by vfx_conv.hip after vfx_convwg.inc.
//
// convwg4p_kernel (round 5): convwg4_kernel's arithmetic (Winograd F(4,3) along the dilated axis, exact fp32 MFMA; same staging map,
// same woven K loop, same weights, results bit-identical to its SPEC 1 / 2 instances: tests/test_wg4_gpu.py launches the same operands
// on either side of the threshold below and compares the bits) as PERSISTENT workgroups whose pipeline runs ACROSS tiles.
//
// Why.  tools/wg4_timeline.py on the one-tile-per-workgroup kernel (profiles/r05_wg4_timeline_and_stagger.txt, r05_wg4_slots.txt): a CU's
// two workgroup slots are EMPTY 5-12 % of the time (a freed slot is re-filled 3.5-4 us later), a workgroup spends 10-39 % of its life
// outside its K loop (C = 512 .. 128: the tap round trip to HBM, the first transform, the first barrier, then the output transform and
// the stores), and the two co-resident workgroups run half a lifetime apart, so that at C = 128 only ONE wave per SIMD is inside its K
// loop 85 % of the time.  Prologue VALU counts and phase alignment, the two explanations of round 4, were measured and ruled out
// (profiles/r05_convwg4_spec_pk_ab.txt).
// Measured (profiles/r05_convwg4_persistent_ab.txt): the C = 64 launches (four chunks per tile: the shortest K loop) 7-11 % faster, the
// C >= 128 launches within the noise, the whole step -0.5 %: with the prologue, the dispatch gap and the phase spread all gone the
// C >= 128 launches still take what they took: they run at the chip's 1400 W power cap (profiles/r05_power_cap.txt: 1375 W, shader clock
// 2.18 GHz, while a bare fp32 MFMA loop holds 154.8 TFLOP/s at 2.40 GHz on 1067 W) -- a busier matrix pipe is answered with a lower
// clock, and what is left to win is energy per product (DESIGN.md 3.0), not schedule.
//
// What.  2 workgroups per CU for the whole launch (grid = 2 x CUs), each walking a fixed list of tiles: the work items n = (batch
// item, tile, channel block) -- channel block fastest -- are cut into 8 contiguous chunks, one per XCD (workgroup w runs on XCD w & 7:
// round-robin dispatch, as the tile order of convwg4_kernel assumes), and workgroup j of an XCD takes items j, j + 64, j + 128, ... of
// its chunk: neighbouring tiles run at the same time on one XCD (their taps overlap: L2 hits), every workgroup gets the same number of
// tiles +- 1, its channel block never changes (64 % gy == 0).  Inside a workgroup the tap prefetch, the staging into LDS and the A-vector
// prefetch simply CONTINUE from the last chunks of tile n into the first chunks of tile n + 64: where convwg4_kernel re-issues clamped
// duplicate loads at the end of its K loop, this kernel loads chunks 0 and 1 of the next tile, stages chunk 0 while the last chunk
// multiplies, and wraps the A groups around.  Between two tiles stand the output transform and the stores of the finished one -- no
// load round trip, no barrier wait, no dispatch.  The accumulators restart through the C operand of the first k-step (0), as in
// convwg4_kernel, so nothing has to be zeroed either; the residual quads of the second convolution (SPEC 2) are
// requested at the start of the last chunk and added in the epilogue.
// Instances exist for the two launches a ResStack layer consists of (SPEC 1 / 2, see convwg4_kernel) with at least four chunks
// (Cin >= 64); everything else stays on convwg4_kernel.  Per-row lengths (ragged batches): a tile past its row's end is skipped, the
// pipeline restarts at the next valid one.
template <int WGM, int WGP, bool D1, bool PRE, int SPEC>
__global__ __launch_bounds__(256, 2) void convwg4p_kernel(const ConvArgs a) {
    static_assert(WGM * WGP == 4, "four waves");
    static_assert((SPEC == 1 && PRE) || (SPEC == 2 && D1 && !PRE), "specialised instances only");
    constexpr int KC = 16, NSTEP = KC / 2;
    constexpr int BM = 32 * WGM, BQ = 32 * WGP;
    constexpr int CG = 256 / BQ;
    constexpr int NSLOT = KC / CG;
    constexpr int SPAN = NSTEP / NSLOT;
    constexpr int PLANE = KC * BQ;
    constexpr int BUF = 6 * PLANE;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lo = lane & 31, hi = lane >> 5;
    const int wm = wave / WGP, wp = wave % WGP;
    // ---- the work list of this workgroup
    const int gy = a.nph_fold;                    // channel blocks per tile
    const int per = gridDim.x >> 3;               // workgroups per XCD (host: a multiple of gy)
    const int xcd = blockIdx.x & 7, jw = blockIdx.x >> 3;
    const int nend = min(a.B * a.ntiles_l * gy, (xcd + 1) * a.xcd_chunk);   // (host: xcd_chunk is a multiple of gy)
    int n = xcd * a.xcd_chunk + jw;
    if (n >= nend) return;
    const int m0 = (jw % gy) * BM;                // the channel block never changes: n = jw (mod gy) for every item of the list
    const int d = D1 ? 1 : a.wg_d;
    const float inv_d = 1.0f / (float)d;
    const int xcs = (int)a.x_cs;
    const int S = a.Cin / KC;                     // chunks per tile (host: even, >= 4: the first and the last pair are distinct code)
    auto quad_q = [&](int Q) {                    // first output of quad Q
        if constexpr (D1) return 4 * Q;
        const int blk = fast_div(Q, d, inv_d);
        return 4 * d * blk + (Q - blk * d);
    };
    const int sq = tid % BQ, cg = tid / BQ;       // staging map: quad, channel group

    // ---- tile state.  Uniform part (SGPRs) of the tile being multiplied (t_*) and of the next one of the list (u_*); per-thread part
    // (xvoff: tap offsets of the thread's staging quad, out of range = zero padding; xin: D1, position 4Q + i inside the row) of the tile
    // whose taps are being LOADED -- the current tile up to chunk S-3, the next one from chunk S-2 on.
    int t_b = 0, t_Q0 = 0, t_Lrow = 0, u_b = 0, u_Q0 = 0, u_Lrow = 0;
    bool t_valid = false, u_valid = false;
    auto tile_uniform = [&](int nn, int& b_, int& Q0_, int& Lrow_, bool& valid_) {
        valid_ = nn < nend;
        const int u = (valid_ ? nn : n) / gy;     // (batch item, tile)
        b_ = u / a.ntiles_l;
        Q0_ = (u - b_ * a.ntiles_l) * BQ;
        Lrow_ = a.x_rows ? __builtin_amdgcn_readfirstlane(a.x_rows[b_]) : a.Lin;
        const int nblk = fast_div(Lrow_ + 4 * d - 1, 4 * d, 0.25f * inv_d);
        valid_ = valid_ && Q0_ < nblk * d;
    };
    int xvoff[6];
    bool xin[4] = {true, true, true, true};       // ... of the tile whose taps are being loaded
    bool xin_st[4] = {true, true, true, true};    // ... of the tile whose chunk is being STAGED (one chunk behind the loads)
    auto tile_thread = [&](int Q0_, int Lrow_, bool valid_) {
        const int q = quad_q(Q0_ + sq);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int p = q + (j - 1) * d;
            xvoff[j] = (valid_ && p >= 0 && p < Lrow_) ? (cg * xcs + p) * 4 : VFX_W_OOB;
        }
        if constexpr (D1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) xin[i] = q + i < Lrow_;
        }
    };
    auto x_rsrc = [&](int b_) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x) + (long long)b_ * a.x_bs, (short)0, 0x7fffffff, 0x00020000);
    };
    const float slope = a.pre_slope;
    auto x_soff = [&](int v) { return v * KC * xcs * 4; };
    const int wcol = BQ == 32 ? sq : ((sq & ~63) | ((sq + 32 * (cg & 1)) & 63));
    float* const wbase = smem + cg * BQ + wcol;

    float xv[NSLOT][6];
    // the tap loads of element j; D1: part 0 = the 16-byte vector (taps 1-4), parts 1 / 2 = taps 0 / 5; else part t = tap t
    auto x_load_part = [&](const __amdgpu_buffer_rsrc_t& rs, int j, int part, int s0) {
        const int so = s0 + j * CG * xcs * 4;
        if constexpr (D1) {
            if (part == 0) {
                const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rs, xvoff[1], so, 0);
                xv[j][1] = __uint_as_float(r.x); xv[j][2] = __uint_as_float(r.y);
                xv[j][3] = __uint_as_float(r.z); xv[j][4] = __uint_as_float(r.w);
            } else if (part == 1) {
                xv[j][0] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, xvoff[0], so, 0));
            } else if (part == 2) {
                xv[j][5] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, xvoff[5], so, 0));
            }
        } else {
            xv[j][part] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, xvoff[part], so, 0));
        }
    };
    auto x_load = [&](const __amdgpu_buffer_rsrc_t& rs, int v) {
        const int s0 = x_soff(v);
#pragma unroll
        for (int j = 0; j < NSLOT; ++j)
#pragma unroll
            for (int p = 0; p < 6; ++p) x_load_part(rs, j, p, s0);
    };
    // pre-activation + B^T of element j
    auto x_transform = [&](int j, float (&V)[6]) {
        float e[6];
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            e[p] = PRE ? fmaxf(xv[j][p], xv[j][p] * slope) : xv[j][p];
            if constexpr (D1) {
                if (p >= 1 && p <= 4) e[p] = xin_st[p - 1] ? e[p] : 0.f;   // (the vector was loaded whole)
            }
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

    // ---- A operands: [6 planes][Cin/8][Cout][8]; two register sets, one 8-channel group each
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wd), (short)0, 0x7fffffff, 0x00020000);
    const int row0 = m0 + wm * 32;
    const int avoff = ((row0 + lo) * 8 + 4 * hi) * 4;
    const int gstride = a.Cout * 32;
    const int pstride = (a.CinPad >> 3) * gstride;
    const int ngrp = 2 * S;                       // 8-channel groups per tile
    float4 aw[2][6];
    auto a_goff = [&](int vg) { return (VFX_WG4_ABL & 1) ? 0 : (vg >= ngrp ? vg - ngrp : vg) * gstride; };   // (groups wrap into the next tile)
    auto a_load_one = [&](auto set_tag, int k, int goff) {
        constexpr int SET = decltype(set_tag)::value;
        const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, avoff, k * pstride + goff, 0);
        aw[SET][k] = make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
    };
    using A0 = std::integral_constant<int, 0>;
    using A1 = std::integral_constant<int, 1>;

    // ---- bias: ONE register.  Every tile closes plane 1 with an extra MFMA  acc[1] += bias (x) 1  behind its last k-step: A operand =
    // bias[row] in k-column 0 (lanes 0-31) and 0 in k-column 1, B operand = 1.0 -- y_i = m1 + ... for all four outputs, so the bias
    // added to plane 1 IS the bias.  BEHIND the K loop, not in front of it: as the start value of plane 1 the bias made every one of
    // the Cin partial sums of m1 round at the size of the bias (tests/test_wg4_gpu.py, profiles/wg4_parity.txt: up to 7 x the fp32
    // statement's RMS under heavy-tailed weight-norm gains); here it is rounded once, into the finished sum.  (The SPEC instances of
    // convwg4_kernel do the same; its run-time instance adds bias and residual to the transformed outputs.)  One MFMA in 48 S.
    const float bias_a = (a.bias && hi == 0) ? a.bias[row0 + lo] : 0.f;
    f32x16 acc[6];
    const int bcol = BQ == 32 ? lo : ((wp * 32 + lo + 32 * hi) & 63);
    const int boffs = hi * BQ + bcol;
    u32x4 rl[2][4];                               // SPEC 2: residual quads, four accumulator rows per batch, two batches in flight
    const int cs4r = (int)a.r_cs * 4;
    const int ycs4 = (int)a.y_cs * 4;

    // One chunk (8 k-pair steps x 6 MFMAs) with the staging of the next chunk and the A vectors of the next group woven in, as in
    // convwg4_kernel.  first_tag: k-step 0 starts the accumulators (C = 0).
    auto mma_chunk = [&](auto first_tag, const __amdgpu_buffer_rsrc_t& rsl, const float* xs, float* wdst, int xchunk, int agrp0) {
        constexpr bool FIRST = decltype(first_tag)::value;
        const float* bp = xs + boffs;
        const int agrp1 = a_goff(agrp0 + 1), agrp2 = a_goff(agrp0 + 2);
        float bf[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) bf[k] = bp[k * PLANE];
        const int xs0 = x_soff(xchunk);
        float V[6];
#pragma unroll
        for (int u = 0; u < NSTEP; ++u) {
            const int el = u / SPAN, ph = u % SPAN;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                constexpr bool ST = !(VFX_WG4_ABL & 8), LD = !(VFX_WG4_ABL & 2);   // (development ablations, see convwg4_kernel)
                if constexpr (SPAN == 4) {
                    if (ST && ph == 0 && k == 0) x_transform(el, V);
                    if (ST && ph == 0 && k < 3) wdst[el * CG * BQ + k * PLANE] = V[k];
                    if (ST && ph == 1 && k < 3) wdst[el * CG * BQ + (k + 3) * PLANE] = V[k + 3];
                    if (LD && ph == 2 && k < 3) x_load_part(rsl, el, k, xs0);
                    if (LD && ph == 3 && k < 3) x_load_part(rsl, el, k + 3, xs0);
                } else {
                    if (ST && ph == 0 && k == 0) x_transform(el, V);
                    if (ST && ph == 0) wdst[el * CG * BQ + k * PLANE] = V[k];
                    if (LD && ph == 1) x_load_part(rsl, el, k, xs0);
                }
                if (u == 0) a_load_one(A1{}, k, agrp1);
                if (u == 4) a_load_one(A0{}, k, agrp2);
                const float4 av4 = (u < 4) ? aw[0][k] : aw[1][k];
                const int kk = u & 3;
                const float av = kk == 0 ? av4.x : (kk == 1 ? av4.y : (kk == 2 ? av4.z : av4.w));
                if constexpr (FIRST) {
                    if (u == 0) {
                        const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                        acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[k], zero16, 0, 0, 0);
                    } else {
                        acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[k], acc[k], 0, 0, 0);
                    }
                } else {
                    acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[k], acc[k], 0, 0, 0);
                }
                if (u < NSTEP - 1 && !(VFX_WG4_ABL & 4)) bf[k] = bp[k * PLANE + (u + 1) * 2 * BQ];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    using Yes = std::true_type;
    using No = std::false_type;

    tile_uniform(n, t_b, t_Q0, t_Lrow, t_valid);
    bool restart = true;                          // the pipeline holds nothing of the current tile yet
#pragma unroll 1
    for (; n < nend; n += per) {
        tile_uniform(n + per, u_b, u_Q0, u_Lrow, u_valid);   // (invalid past the end of the list: every offset out of range, loads return zeros)
        if (t_valid) {
            __amdgpu_buffer_rsrc_t xrs = x_rsrc(t_b);
            if (restart) {
                // the prologue of convwg4_kernel: taps of chunk 0, first A vectors, chunk 0 into LDS buffer 0, taps of chunk 1
                tile_thread(t_Q0, t_Lrow, true);
                if constexpr (D1) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) xin_st[i] = xin[i];
                }
                x_load(xrs, 0);
#pragma unroll
                for (int k = 0; k < 6; ++k) a_load_one(A0{}, k, 0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < NSLOT; ++j) {
                    float V[6];
                    x_transform(j, V);
#pragma unroll
                    for (int k = 0; k < 6; ++k) wbase[j * CG * BQ + k * PLANE] = V[k];
                }
                x_load(xrs, 1);
                __builtin_amdgcn_sched_barrier(0);
                __syncthreads();
            }
            // chunks 0 and 1: the accumulators start
            mma_chunk(Yes{}, xrs, smem, wbase + BUF, 2, 0);
            __syncthreads();
            mma_chunk(No{}, xrs, smem + BUF, wbase, 3, 2);
            __syncthreads();
            // output / residual addressing of this lane's quad
            const int qe = quad_q(t_Q0 + wp * 32 + lo);
            const bool full = qe + 3 < t_Lrow;
            const bool has_tail = D1 && (t_Lrow & 3) != 0 && (t_Lrow >> 2) >= t_Q0 && (t_Lrow >> 2) < t_Q0 + BQ;   // (uniform)
            const __amdgpu_buffer_rsrc_t rrs = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float*>(a.res ? a.res : a.x) + (long long)t_b * a.r_bs, (short)0, 0x7fffffff, 0x00020000);
            const int rvq = (SPEC == 2 && full) ? (4 * hi * (int)a.r_cs + qe) * 4 : VFX_W_OOB;
            // chunks 2 .. S-1 in pairs.  The LAST pair differs in data only: before chunk S-2 the per-thread load state moves on to the next
            // tile (chunk S-2 stages chunk S-1 of this tile and loads chunk 0 of the next, chunk S-1 stages that chunk 0 -- with the next
            // tile's xin -- and loads chunk 1), the chunk index wraps, and (SPEC 2) the first two residual batches of this tile are
            // requested in front of chunk S-1.  (One code path for all pairs: a separate copy of the last pair, six chunk bodies in a row,
            // drove the register allocator into 90-190 spilled VGPRs.)
#pragma unroll 1
            for (int s = 2; s < S; s += 2) {
                const bool last = s == S - 2;
                if (last) {
                    tile_thread(u_Q0, u_Lrow, u_valid);
                    xrs = x_rsrc(u_b);
                }
                mma_chunk(No{}, xrs, smem, wbase + BUF, last ? 0 : s + 2, 2 * s);
                __syncthreads();
                if (last) {
                    if constexpr (D1) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) xin_st[i] = xin[i];
                    }
                    if constexpr (SPEC == 2) {
#pragma unroll
                        for (int bt = 0; bt < 2; ++bt)
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                rl[bt][e] = __builtin_amdgcn_raw_buffer_load_b128(rrs, rvq, (row0 + e + 8 * bt) * cs4r, 0);
                    }
                }
                mma_chunk(No{}, xrs, smem + BUF, wbase, last ? 1 : s + 3, 2 * s + 2);
                __syncthreads();
            }

            // ---- the bias product closes plane 1 (see bias_a); output transform, activation / residual, stores of the finished tile
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(bias_a, 1.0f, acc[1], 0, 0, 0);
            const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(
                a.y + (long long)t_b * a.y_bs, (short)0, 0x7fffffff, 0x00020000);
            const float ps = a.post_slope;
            int yv[4];
            int yvq = VFX_W_OOB;
#pragma unroll
            for (int i = 0; i < 4; ++i) yv[i] = qe + i * d < t_Lrow ? (4 * hi * (int)a.y_cs + qe + i * d) * 4 : VFX_W_OOB;
            if constexpr (D1) {
                yvq = full ? yv[0] : VFX_W_OOB;
#pragma unroll
                for (int i = 0; i < 4; ++i) yv[i] = full ? VFX_W_OOB : yv[i];
            }
            auto store4 = [&](const float (&v)[4], int soff) {
                if constexpr (D1) {
                    u32x4 u;
                    u.x = __float_as_uint(v[0]); u.y = __float_as_uint(v[1]); u.z = __float_as_uint(v[2]); u.w = __float_as_uint(v[3]);
                    __builtin_amdgcn_raw_buffer_store_b128(u, yrsrc, yvq, soff, 0);
                }
                if (!D1 || has_tail) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[i]), yrsrc, yv[i], soff, 0);
                }
            };
            auto outs = [&](int r, float (&y)[4]) {
                const float p12 = acc[1][r] + acc[2][r], m12 = acc[1][r] - acc[2][r];
                const float p34 = acc[3][r] + acc[4][r], m34 = acc[3][r] - acc[4][r];
                y[0] = (acc[0][r] + p12) + p34;
                y[1] = fmaf(2.f, m34, m12);
                y[2] = fmaf(4.f, p34, p12);
                y[3] = fmaf(8.f, m34, m12) + acc[5][r];
            };
            if constexpr (SPEC == 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int soff = (row0 + (r & 3) + 8 * (r >> 2)) * ycs4;
                    float y[4];
                    outs(r, y);
#pragma unroll
                    for (int i = 0; i < 4; ++i) y[i] = fmaxf(y[i], y[i] * ps);   // (0 <= slope <= 1, checked on the host)
                    store4(y, soff);
                }
            } else {
                int tv[4];                        // the straddling quad's single elements (has_tail only)
#pragma unroll
                for (int i = 0; i < 4; ++i) tv[i] = (qe + i < t_Lrow && !full) ? (4 * hi * (int)a.r_cs + qe + i) * 4 : VFX_W_OOB;
#pragma unroll
                for (int bt = 0; bt < 4; ++bt) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = 4 * bt + e;
                        const int srow = row0 + e + 8 * bt;
                        float y[4];
                        outs(r, y);
                        const u32x4 t = rl[bt & 1][e];
                        y[0] += __uint_as_float(t.x); y[1] += __uint_as_float(t.y); y[2] += __uint_as_float(t.z); y[3] += __uint_as_float(t.w);
                        if (has_tail) {           // (uniform, one tile per row at most; every other lane's offsets read 0, this quad's
                                                  // vector load returned zeros)
#pragma unroll
                            for (int i = 0; i < 4; ++i) y[i] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrs, tv[i], srow * cs4r, 0));
                        }
                        store4(y, srow * ycs4);
                    }
                    if (bt + 2 < 4) {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            rl[bt & 1][e] = __builtin_amdgcn_raw_buffer_load_b128(rrs, rvq, (row0 + e + 8 * (bt + 2)) * cs4r, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            restart = !u_valid;                   // (the next tile's chunks 0 / 1 are staged / in flight -- unless there is none)
        } else {
            restart = true;                       // (ragged batches) nothing to compute here: the pipeline restarts at the next valid tile
        }
        t_b = u_b; t_Q0 = u_Q0; t_Lrow = u_Lrow; t_valid = u_valid;
    }
}

template <int WGM, int WGP, bool D1, bool PRE, int SPEC>
static int launch_wg4p(const ConvArgs& a, int nwg, size_t lds, hipStream_t s) {
    return vfx_launch<convwg4p_kernel<WGM, WGP, D1, PRE, SPEC>>(dim3(nwg), dim3(256), lds, s, a);
}

// Compute units of the current device (cached per device)
static int vfx_cu_count() {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    dev &= 63;
    if (!cus[dev]) {
        hipDeviceProp_t p;
        cus[dev] = (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256;
    }
    return cus[dev];
}

// The persistent form of a convwg4_kernel launch (a, ntiles, gy, BQ as try_launch_convwg4 prepared them): VFX_ENOTSUP = not this launch
static int try_launch_convwg4p(ConvArgs a, int ntiles, int gy, bool wide, bool d1vec, hipStream_t stream) {
    static const bool off = VFX_DEV_ENV("VFX_WG4_PERSIST") && atoi(VFX_DEV_ENV("VFX_WG4_PERSIST")) == 0;   // development
    if (off) return VFX_ENOTSUP;
    const int S = a.Cin / 16;
    if (S < 4 || (S & 1)) return VFX_ENOTSUP;     // (the first and the last pair of chunks are distinct code)
    if (a.bias && !vfx_aligned16(a.bias)) return VFX_ENOTSUP;
    const bool first = !a.res && a.pre_act == VFX_PRE_LRELU && a.post_act == VFX_POST_LRELU;
    const bool second = d1vec && a.res && a.pre_act == VFX_PRE_NONE && a.post_act == VFX_POST_NONE;
    if (!first && !second) return VFX_ENOTSUP;
    const long long N = (long long)a.B * ntiles * gy;
    if (N >= (1ll << 30)) return VFX_ENOTSUP;
    int nwg = 2 * vfx_cu_count();                 // two workgroups per CU, resident for the whole launch
    nwg -= nwg % (8 * gy);                        // whole XCD groups, a multiple of gy per XCD
    if (nwg < 8 * gy || N < 4ll * nwg) return VFX_ENOTSUP;   // short launches: convwg4_kernel
    long long chunk = (N + 7) / 8;
    chunk = (chunk + gy - 1) / gy * gy;
    a.ntiles_l = ntiles;
    a.nph_fold = gy;
    a.xcd_chunk = (int)chunk;
    // (181-226 VGPRs: never more than two workgroups per CU; the LDS is not padded, so that another stream's small kernels still fit beside them)
    const size_t lds = 2ull * 6 * 16 * (wide ? 32 : 64) * sizeof(float);
    if (first) {
        if (d1vec) return wide ? launch_wg4p<4, 1, true, true, 1>(a, nwg, lds, stream) : launch_wg4p<2, 2, true, true, 1>(a, nwg, lds, stream);
        return wide ? launch_wg4p<4, 1, false, true, 1>(a, nwg, lds, stream) : launch_wg4p<2, 2, false, true, 1>(a, nwg, lds, stream);
    }
    return wide ? launch_wg4p<4, 1, true, false, 2>(a, nwg, lds, stream) : launch_wg4p<2, 2, true, false, 2>(a, nwg, lds, stream);
}
