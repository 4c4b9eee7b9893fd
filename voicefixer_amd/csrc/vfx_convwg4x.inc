// vfx_convwg4x.inc -- included by vfx_conv.hip after vfx_convwg4p.inc.
//
// convwg4x_kernel (round 6): convwg4p_kernel's arithmetic and persistent work list with a RE-BLOCKED wave tile -- 32 output channels x
// 64 quads x 6 planes per wave (twelve accumulator tiles, 192 registers) instead of 32 x 32 x 6 -- and a DEFERRED epilogue.
//
// Why (DESIGN.md 3.0, profiles/r05_power_cap.txt).  The C >= 128 ResStack convolutions run at the chip's 1400 W power cap: matrix-pipe
// busy share x shader clock is what the firmware conserves, so what is left to win is ENERGY per product, and the MFMAs are less than
// half of it.  In the 32 x 32 wave tile every 16-byte A vector (weights, straight from L2: 6.7 TB/s through L2 -> L1 over a launch)
// feeds FOUR MFMAs and every B fragment costs one ds_read_b32 per MFMA.  Here
//   * every A vector feeds EIGHT MFMAs (two quad blocks): half the L2 -> L1 weight stream per product;
//   * the two quad blocks' B fragments of a (plane, channel pair) are ONE ds_read_b64 -- quad q of a chunk row lives at LDS position
//     2 (q & 31) + (q >> 5), so lane lo finds quads lo and lo + 32 side by side: half the LDS read instructions per product;
//   * a workgroup tile is 128 channels x 64 quads: per product the same tap loads, transform VALU and LDS writes as before.
// Price: ~330 live registers, i.e. ONE wave per SIMD and one workgroup per CU: nothing covers a wave's own stalls.  The first form of
// this kernel (profiles/r06_convwg4x_ab.txt) ran its matrix loop at 0.93 of the fp32 MFMA peak at the full 2.4 GHz (the power cap no
// longer binds) and then lost 22 % (C = 128) / 10 % (C = 256) of the launch in the output transform + stores of every finished tile:
// 128 KB of stores (+ as much residual) per workgroup and tile, issued by waves that have nothing else to do while the store path drains.
// Hence the deferred epilogue: a finished tile's outputs are transformed and written to LDS (32 KB per wave, private to it: no barrier),
// and the global stores -- with the residual loads / additions of the second convolution and the leaky ReLU of the first -- TRICKLE out
// under the NEXT tile's K loop, a few per k-pair step, their LDS reads and residual loads issued one chunk before they are used.
// To make room the staging chunk is 8 channels (two 12 KB buffers; a barrier per 48 MFMAs per wave).
//
// Work list, tile walk, SPEC instances, bias through an extra MFMA behind the last k-step, per-row lengths: exactly convwg4p_kernel
// (see there).  Every output is one chain over the input channels in ascending order and the bias closes plane 1, as in the SPEC
// instances of convwg4_kernel: the three kernels return the same bits (tests/test_wg4_gpu.py pins it on either side of the threshold).
// Development ablations (wrong results, timing only; `make dev DEVDEFS=-DVFX_WG4X_ABL=n DEVNAME=xabln`):
//   1 = no output transform / LDS hand-over / trickle     2 = no staging in the K loop (no tap loads, transform, LDS writes)
//   4 = no barriers in the K loop     8 = every A vector from 8-channel group 0 (L1 hits instead of the L2 stream)     16 = no trickle (outputs stay in LDS)
//   32 = trickle without its global stores     64 = trickle without its residual loads
#ifndef VFX_WG4X_ABL
#define VFX_WG4X_ABL 0
#endif
template <bool D1, bool PRE, int SPEC>
__global__ __launch_bounds__(256, 1) void convwg4x_kernel(const ConvArgs a) {
    static_assert((SPEC == 1 && PRE) || (SPEC == 2 && D1 && !PRE), "specialised instances only");
    constexpr int KC = 8, NSTEP = KC / 2;         // 8-channel chunks: 4 k-pair steps x 6 planes x 2 quad blocks = 48 MFMAs per wave and chunk
    constexpr int BM = 128, BQ = 64;
    constexpr int CG = 256 / BQ;                  // 4 channel groups = the four waves
    constexpr int NSLOT = KC / CG;                // 2 staged (channel, quad) elements per thread per chunk
    constexpr int SPAN = NSTEP / NSLOT;           // 2 k-pair steps per element: transform + writes, then the next loads
    constexpr int PLANE = KC * BQ;
    constexpr int BUF = 6 * PLANE;                // 12 KB
    constexpr int OBUF = 32 * 4 * BQ;             // a wave's output tile: 32 rows x 256 positions (32 KB)
    constexpr int TPK = D1 ? 1 : 4;               // trickle units per k-pair step; a unit = one 16-byte quad row (D1) / one dword row of one output index
    constexpr int NSL = NSTEP * TPK;              // trickle slots per chunk = the units of FOUR output rows
    constexpr int NUNIT = D1 ? 32 : 128;          // units per tile and wave
    constexpr int NIT = NUNIT / NSL;              // trickle iterations (chunks) per tile: 8
    static_assert(NIT * NSL == NUNIT && NIT == 8, "an iteration is valid or not as a whole");
    static_assert(SPAN == 2, "staging map");
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lo = lane & 31, hi = lane >> 5;
    // ---- the work list of this workgroup (convwg4p_kernel's: XCD chunk, workgroup j takes items j, j + per, ...)
    const int gy = a.nph_fold;                    // channel blocks per tile
    const int per = gridDim.x >> 3;               // workgroups per XCD (host: a multiple of gy)
    const int xcd = blockIdx.x & 7, jw = blockIdx.x >> 3;
    const int nend = min(a.B * a.ntiles_l * gy, (xcd + 1) * a.xcd_chunk);
    int n = xcd * a.xcd_chunk + jw;
    if (n >= nend) return;
    const int m0 = (jw % gy) * BM;
    const int d = D1 ? 1 : a.wg_d;
    const float inv_d = 1.0f / (float)d;
    const int xcs = (int)a.x_cs;
    const int S = a.Cin / KC;                     // chunks per tile (host: even, >= 4)
    auto quad_q = [&](int Q) {                    // first output of quad Q
        if constexpr (D1) return 4 * Q;
        const int blk = fast_div(Q, d, inv_d);
        return 4 * d * blk + (Q - blk * d);
    };
    const int sq = lane, cg = wave;               // staging map: quad, channel group

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
    // LDS: [buffer][plane][channel][position], quad q at position 2 (q & 31) + (q >> 5); then the four waves' output tiles
    float* const wbase = smem + cg * BQ + 2 * (sq & 31) + (sq >> 5);
    float* const obuf = smem + 2 * BUF + wave * OBUF;

    float xv[2][NSLOT][6];                        // taps of chunk c: set c & 1, loaded TWO chunks before they are staged (a chunk is 48 MFMAs,
                                                  // ~1.3 us: one chunk of distance is about an L2 / HBM round trip under load)
    auto x_load_part = [&](const int xset, const __amdgpu_buffer_rsrc_t& rs, int j, int part, int s0) {
        const int so = s0 + j * CG * xcs * 4;
        if constexpr (D1) {
            if (part == 0) {
                const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rs, xvoff[1], so, 0);
                xv[xset][j][1] = __uint_as_float(r.x); xv[xset][j][2] = __uint_as_float(r.y);
                xv[xset][j][3] = __uint_as_float(r.z); xv[xset][j][4] = __uint_as_float(r.w);
            } else if (part == 1) {
                xv[xset][j][0] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, xvoff[0], so, 0));
            } else if (part == 2) {
                xv[xset][j][5] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, xvoff[5], so, 0));
            }
        } else {
            xv[xset][j][part] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, xvoff[part], so, 0));
        }
    };
    auto x_load = [&](const int xset, const __amdgpu_buffer_rsrc_t& rs, int v) {
        const int s0 = x_soff(v);
#pragma unroll
        for (int j = 0; j < NSLOT; ++j)
#pragma unroll
            for (int p = 0; p < 6; ++p) x_load_part(xset, rs, j, p, s0);
    };
    auto x_transform = [&](const int xset, int j, float (&V)[6]) {
        float e[6];
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            e[p] = PRE ? fmaxf(xv[xset][j][p], xv[xset][j][p] * slope) : xv[xset][j][p];
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

    // ---- A operands: [6 planes][Cin/8][Cout][8]; two register sets, chunk c (= 8-channel group c) multiplies from set c & 1
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wd), (short)0, 0x7fffffff, 0x00020000);
    const int row0 = m0 + wave * 32;
    const int avoff = ((row0 + lo) * 8 + 4 * hi) * 4;
    const int gstride = a.Cout * 32;
    const int pstride = (a.CinPad >> 3) * gstride;
    float4 aw[2][6];
    auto a_goff = [&](int vg) { return (VFX_WG4X_ABL & 8) ? 0 : (vg >= S ? vg - S : vg) * gstride; };   // (groups wrap into the next tile)
    auto a_load_one = [&](auto set_tag, int k, int goff) {
        constexpr int SET = decltype(set_tag)::value;
        const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, avoff, k * pstride + goff, 0);
        aw[SET][k] = make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
    };
    using A0 = std::integral_constant<int, 0>;
    using A1 = std::integral_constant<int, 1>;

    // ---- bias: every tile CLOSES plane 1 of both quad blocks with an extra MFMA  acc += bias (x) 1  behind its last k-step (see
    // convwg4p_kernel): the bias is rounded once, into the finished sum -- never into the partial sums of the K loop
    const float bias_a = (a.bias && hi == 0) ? a.bias[row0 + lo] : 0.f;
    f32x16 acc[6][2];
    const int boffs = hi * BQ + 2 * lo;           // B fragments of quads lo, lo + 32: one 8-byte read
    const int cs4r = (int)a.r_cs * 4;
    const int ycs4 = (int)a.y_cs * 4;
    const float ps = a.post_slope;

    // ---- the deferred epilogue.  `obuf` holds the outputs of the last finished tile; trickle iteration counter `tm` (one iteration = the
    // NSL slots of one chunk = four output rows): slot j of iteration m USES unit (m - 1) NSL + j -- its LDS read (and residual load)
    // were issued by slot j of iteration m - 1 -- and LOADS unit m NSL + j.  Units: D1: row rr = t of the wave's 32, lane L <-> quad L of
    // the tile (16 bytes); otherwise row rr = t >> 2, output index i = t & 3 (= j & 3: a constant per slot), lane L <-> quad L (one dword
    // at quad_q + i d).  An iteration is valid or not AS A WHOLE (m in 1 .. NIT uses, m in 0 .. NIT - 1 loads): what depends on m -- the
    // descriptors (zero records when invalid: loads return 0, stores are dropped), the row offsets, the LDS offset -- is formed once per
    // chunk, and a slot is STRAIGHT-LINE code with one scalar addition.  One wave per SIMD: a branch costs its instruction-fetch latency
    // in matrix-pipe time (the branchy first form of these slots cost 0.8 ms per launch with its stores and loads compiled OUT), long
    // scalar sequences between two MFMAs idle the pipe just the same, and conditional memory operations keep the compiler from counting vmcnt.
    int tm = 0x1000000;                           // (nothing pending)
    int pyv[4] = {VFX_W_OOB, VFX_W_OOB, VFX_W_OOB, VFX_W_OOB};   // !D1: byte offset of output i of this lane's quad (out of range past the row's end)
    int pq4 = 0, p_Lrow4 = 0;                     // D1: byte offset of this lane's quad inside its row; the row's length in bytes = the num_records of
                                                  // the per-row descriptors: a raw-buffer dwordx4 access is range-checked PER DWORD on gfx950
                                                  // (tools/probe/oob_clip.hip), so the quad that straddles the row's end is stored / loaded
                                                  // exactly as far as the row goes -- no single-element path, no branch
    float tl[NSL][D1 ? 4 : 1];                    // LDS data in flight
    u32x4 tres[SPEC == 2 ? NSL : 1];              // residual quads in flight
    const float* p_ybase = a.y;
    const float* p_rbase = a.res ? a.res : a.x;
    struct TrickleIter {                          // the uniform state of one iteration
        __amdgpu_buffer_rsrc_t yrs, rrs;          // !D1: the whole batch item (rows through soff_u)
        int soff_u, soff_l;
        const float* yrow;                        // D1: first of the four rows used / loaded; records of a row
        const float* rrow;
        int nrec_u, nrec_l;
        const float* lds;
    };
    auto trickle_pending = [&]() { return tm <= NIT; };
    auto trickle_iter = [&]() {
        TrickleIter it;
        const bool ok_u = tm >= 1 && tm <= NIT, ok_l = tm < NIT;
        const int ml = ok_l ? tm : 0;
        it.yrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p_ybase), (short)0, ok_u ? 0x7fffffff : 0, 0x00020000);
        it.rrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p_rbase), (short)0, ok_l ? 0x7fffffff : 0, 0x00020000);
        it.soff_u = ok_u ? (row0 + (tm - 1) * 4) * ycs4 : 0;
        it.soff_l = (row0 + ml * 4) * cs4r;
        it.yrow = p_ybase + (long long)(row0 + (ok_u ? tm - 1 : 0) * 4) * a.y_cs;
        it.rrow = p_rbase + (long long)(row0 + ml * 4) * a.r_cs;
        it.nrec_u = ok_u ? p_Lrow4 : 0;
        it.nrec_l = ok_l ? p_Lrow4 : 0;
        it.lds = obuf + ml * (4 * 4 * BQ) + (D1 ? lane * 4 : lane);
        return it;
    };
    auto trickle_slot = [&](const TrickleIter& it, const int J) {   // (J: a constant after unrolling -- it indexes register arrays)
        if constexpr ((VFX_WG4X_ABL & 17) != 0) return;
        const int soff = it.soff_u + (D1 ? J : (J >> 2)) * ycs4;
        if constexpr (D1) {
            float y[4] = {tl[J][0], tl[J][1], tl[J][2], tl[J][3]};
            if constexpr (SPEC == 2) {
                y[0] += __uint_as_float(tres[J].x); y[1] += __uint_as_float(tres[J].y);
                y[2] += __uint_as_float(tres[J].z); y[3] += __uint_as_float(tres[J].w);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) y[i] = fmaxf(y[i], y[i] * ps);   // (0 <= slope <= 1, checked on the host)
            }
            u32x4 v;
            v.x = __float_as_uint(y[0]); v.y = __float_as_uint(y[1]); v.z = __float_as_uint(y[2]); v.w = __float_as_uint(y[3]);
            if constexpr (!(VFX_WG4X_ABL & 32)) {
                const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(it.yrow + (long long)J * a.y_cs), (short)0, it.nrec_u, 0x00020000);
                __builtin_amdgcn_raw_buffer_store_b128(v, yr, pq4, 0, 0);
            } else if (y[0] + y[1] + y[2] + y[3] == 12345.678f) a.y[1] = y[0];
            const float4 nv = *reinterpret_cast<const float4*>(it.lds + J * (4 * BQ));
            tl[J][0] = nv.x; tl[J][1] = nv.y; tl[J][2] = nv.z; tl[J][3] = nv.w;
            if constexpr (SPEC == 2 && !(VFX_WG4X_ABL & 64)) {
                const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(it.rrow + (long long)J * a.r_cs), (short)0, it.nrec_l, 0x00020000);
                tres[J] = __builtin_amdgcn_raw_buffer_load_b128(rr, pq4, 0, 0);
            }
        } else {
            float y = tl[J][0];
            y = fmaxf(y, y * ps);
            if constexpr (!(VFX_WG4X_ABL & 32)) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y), it.yrs, pyv[J & 3], soff, 0);
            else if (y == 12345.678f) a.y[1] = y;
            tl[J][0] = it.lds[J * BQ];
        }
    };
    auto trickle_drain = [&]() {                  // whatever is still pending, un-overlapped (short K loops; the end of the work list)
        while (trickle_pending()) {
            const TrickleIter it = trickle_iter();
#pragma unroll
            for (int j = 0; j < NSL; ++j) trickle_slot(it, j);
            ++tm;
        }
    };

    // One chunk: 4 k-pair steps x 6 planes x 2 quad blocks = 48 MFMAs from A set SET, with the staging of the next chunk, the A vectors of
    // the next 8-channel group and TPK trickle slots per step woven in.  An element's staging spans two k-pair steps: transform + six LDS
    // writes, then the six tap loads of the element that takes its registers next.  The workgroup barrier stands in front of the LAST
    // k-pair step (every LDS write of the chunk has been issued by then, and this wave's last B fragments of the buffer are in registers):
    // the first B fragments of the NEXT chunk are read under that step's twelve MFMAs instead of behind the barrier.  `bf` lives across chunks.
    float2 bf[6];
    auto bf_first = [&](const float* xs) {
#pragma unroll
        for (int k = 0; k < 6; ++k) bf[k] = *reinterpret_cast<const float2*>(xs + boffs + k * PLANE);
    };
    auto mma_chunk = [&](auto first_tag, auto set_tag, auto trk_tag, const __amdgpu_buffer_rsrc_t& rsl, const float* xs, float* wdst, int xchunk, int agrp) {
        constexpr bool FIRST = decltype(first_tag)::value;
        constexpr bool TRK = decltype(trk_tag)::value;    // trickle slots compiled in (the chunks in which a finished tile can still owe outputs)
        TrickleIter it;
        if constexpr (TRK) it = trickle_iter();
        constexpr int SET = decltype(set_tag)::value;     // chunk parity: A set SET; the chunk staged here (c + 1) and the one loaded (c + 3) use tap set 1 - SET
        const float* bp = xs + boffs;
        const float* bpn = (xs == smem ? smem + BUF : smem) + boffs;     // the buffer this chunk's staging fills
        const int agn = a_goff(agrp + 1);
        const int xs0 = x_soff(xchunk);
        float V[6];
#pragma unroll
        for (int u = 0; u < NSTEP; ++u) {
            const int el = u / SPAN, ph = u % SPAN;
            if (u == NSTEP - 1 && !(VFX_WG4X_ABL & 4)) __syncthreads();
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                constexpr bool STG = !(VFX_WG4X_ABL & 2);
                if (STG && ph == 0 && k == 0) x_transform(1 - SET, el, V);
                if (STG && ph == 0) wdst[el * CG * BQ + k * PLANE] = V[k];
                if (STG && ph == 1) x_load_part(1 - SET, rsl, el, k, xs0);
                if (u == 0) a_load_one(std::integral_constant<int, 1 - SET>{}, k, agn);
                const float4 av4 = aw[SET][k];
                const float av = u == 0 ? av4.x : (u == 1 ? av4.y : (u == 2 ? av4.z : av4.w));
                if constexpr (FIRST) {
                    if (u == 0) {
                        const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                        acc[k][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[k].x, zero16, 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                        acc[k][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[k].y, zero16, 0, 0, 0);
                    } else {
                        acc[k][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[k].x, acc[k][0], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                        acc[k][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[k].y, acc[k][1], 0, 0, 0);
                    }
                } else {
                    acc[k][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[k].x, acc[k][0], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    acc[k][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[k].y, acc[k][1], 0, 0, 0);
                }
                if (u < NSTEP - 1) bf[k] = *reinterpret_cast<const float2*>(bp + k * PLANE + (u + 1) * 2 * BQ);
                else bf[k] = *reinterpret_cast<const float2*>(bpn + k * PLANE);      // (behind the barrier: the next chunk's k-pair step 0)
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (TRK && TPK == 1) {
                    if (k == 2) trickle_slot(it, u);
                } else if constexpr (TRK) {
                    if (k != 0 && k != 3) trickle_slot(it, u * TPK + (k < 3 ? k - 1 : k - 2));   // (after planes 1, 2, 4, 5)
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        ++tm;
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
                tile_thread(t_Q0, t_Lrow, true);
                if constexpr (D1) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) xin_st[i] = xin[i];
                }
                x_load(0, xrs, 0);
#pragma unroll
                for (int k = 0; k < 6; ++k) a_load_one(A0{}, k, 0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < NSLOT; ++j) {
                    float V[6];
                    x_transform(0, j, V);
#pragma unroll
                    for (int k = 0; k < 6; ++k) wbase[j * CG * BQ + k * PLANE] = V[k];
                }
                x_load(1, xrs, 1);
                x_load(0, xrs, 2);
                __builtin_amdgcn_sched_barrier(0);
                __syncthreads();
                bf_first(smem);
            }
            mma_chunk(Yes{}, A0{}, Yes{}, xrs, smem, wbase + BUF, 3, 0);
            mma_chunk(No{}, A1{}, Yes{}, xrs, smem + BUF, wbase, 4, 1);
            // chunks 2 .. S-1 in pairs.  Chunk c stages chunk c + 1 and loads the taps of chunk c + 3: from chunk S - 3 on the per-thread load
            // state is the NEXT tile's (chunks 0, 1, 2 of it), and chunk S - 1 stages its chunk 0 (with the next tile's xin).  The previous
            // tile's outputs trickle out during chunks 0 .. NIT; the pairs after that are compiled without the slots.
            auto chunk_pair = [&](int s, auto trk_tag) {
                const bool last = s == S - 2;
                mma_chunk(No{}, A0{}, trk_tag, xrs, smem, wbase + BUF, last ? 1 : s + 3, s);
                if (s == S - 4) {
                    tile_thread(u_Q0, u_Lrow, u_valid);
                    xrs = x_rsrc(u_b);
                }
                if (last) {
                    if constexpr (D1) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) xin_st[i] = xin[i];
                    }
                }
                mma_chunk(No{}, A1{}, trk_tag, xrs, smem + BUF, wbase, s >= S - 4 ? s + 4 - S : s + 4, s + 1);
            };
            const int SA = min(S, NIT + 2);       // (NIT even: chunks 0 .. NIT + 1 carry the slots)
#pragma unroll 1
            for (int s = 2; s < SA; s += 2) chunk_pair(s, Yes{});
#pragma unroll 1
            for (int s = SA; s < S; s += 2) chunk_pair(s, No{});

            // ---- the finished tile: the bias product closes plane 1 of both quad blocks (see bias_a), whatever the previous tile still
            // owes goes out (short K loops only), then output transform -> LDS, and the tile becomes the pending one
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(bias_a, 1.0f, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(bias_a, 1.0f, acc[1][1], 0, 0, 0);
            trickle_drain();
            if constexpr ((VFX_WG4X_ABL & 1) == 0) {
#pragma unroll
                for (int qb = 0; qb < 2; ++qb) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float p12 = acc[1][qb][r] + acc[2][qb][r], m12 = acc[1][qb][r] - acc[2][qb][r];
                        const float p34 = acc[3][qb][r] + acc[4][qb][r], m34 = acc[3][qb][r] - acc[4][qb][r];
                        const float y0 = (acc[0][qb][r] + p12) + p34;
                        const float y1 = fmaf(2.f, m34, m12);
                        const float y2 = fmaf(4.f, p34, p12);
                        const float y3 = fmaf(8.f, m34, m12) + acc[5][qb][r];
                        const int rr = (r & 3) + 8 * (r >> 2);            // (+ 4 hi)
                        if constexpr (D1) {
                            *reinterpret_cast<float4*>(obuf + ((rr + 4 * hi) * BQ + qb * 32 + lo) * 4) = make_float4(y0, y1, y2, y3);
                        } else {
                            float* o = obuf + (rr + 4 * hi) * 4 * BQ + qb * 32 + lo;      // [row][output index][quad]
                            o[0 * BQ] = y0; o[1 * BQ] = y1; o[2 * BQ] = y2; o[3 * BQ] = y3;
                        }
                    }
                }
                p_ybase = a.y + (long long)t_b * a.y_bs;
                p_rbase = (a.res ? a.res : a.x) + (long long)t_b * a.r_bs;
                const int ql = quad_q(t_Q0 + lane);
                if constexpr (D1) {
                    pq4 = ql * 4;
                    p_Lrow4 = t_Lrow * 4;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) pyv[i] = ql + i * d < t_Lrow ? (ql + i * d) * 4 : VFX_W_OOB;
                }
                tm = 0;
            } else {                              // (ablation: keep the accumulators alive with one store that never happens)
                float sink = 0.f;
#pragma unroll
                for (int k = 0; k < 6; ++k) sink += acc[k][0][0] + acc[k][1][15];
                if (sink == 12345.678f) a.y[0] = sink;
            }
            restart = !u_valid;                   // (the next tile's chunks 0 / 1 are staged / in flight -- unless there is none)
        } else {
            restart = true;                       // (ragged batches) nothing to compute here: the pipeline restarts at the next valid tile
        }
        t_b = u_b; t_Q0 = u_Q0; t_Lrow = u_Lrow; t_valid = u_valid;
    }
    trickle_drain();                              // the last tile's outputs
}

template <bool D1, bool PRE, int SPEC>
static int launch_wg4x(const ConvArgs& a, int nwg, size_t lds, hipStream_t s) {
    return vfx_launch<convwg4x_kernel<D1, PRE, SPEC>>(dim3(nwg), dim3(256), lds, s, a);
}

// The re-blocked persistent form of a wide (Cout % 128 == 0) convwg4_kernel launch; `a`, d1vec as try_launch_convwg4 prepared them, the tile
// count re-derived for 64 quads per tile.  VFX_ENOTSUP = not this launch.
static int try_launch_convwg4x(ConvArgs a, long long nquads, bool d1vec, hipStream_t stream) {
    const int S = a.Cin / 8;
    if (S < 8 || (S & 1)) return VFX_ENOTSUP;
    if (a.Cout % 128 != 0) return VFX_ENOTSUP;
    if (a.bias && !vfx_aligned16(a.bias)) return VFX_ENOTSUP;
    const bool first = !a.res && a.pre_act == VFX_PRE_LRELU && a.post_act == VFX_POST_LRELU;
    const bool second = d1vec && a.res && a.pre_act == VFX_PRE_NONE && a.post_act == VFX_POST_NONE;
    if (!first && !second) return VFX_ENOTSUP;
    const int gy = a.Cout / 128;
    const int ntiles = (int)((nquads + 63) / 64);
    const long long N = (long long)a.B * ntiles * gy;
    if (N >= (1ll << 30)) return VFX_ENOTSUP;
    int nwg = vfx_cu_count();                     // one workgroup per CU, resident for the whole launch
    nwg -= nwg % (8 * gy);
    if (nwg < 8 * gy || N < 4ll * nwg) return VFX_ENOTSUP;
    long long chunk = (N + 7) / 8;
    chunk = (chunk + gy - 1) / gy * gy;
    a.ntiles_l = ntiles;
    a.nph_fold = gy;
    a.xcd_chunk = (int)chunk;
    const size_t lds = (2ull * 6 * 8 * 64 + 4ull * 32 * 256) * sizeof(float);      // two staging buffers + four output tiles: 152 KB
    if (first) return d1vec ? launch_wg4x<true, true, 1>(a, nwg, lds, stream) : launch_wg4x<false, true, 1>(a, nwg, lds, stream);
    return launch_wg4x<true, false, 2>(a, nwg, lds, stream);
}
