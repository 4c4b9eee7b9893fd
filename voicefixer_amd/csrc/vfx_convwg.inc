// vfx_convwg.inc -- included by vfx_conv.hip after vfx_convw.inc.
//
// The k = 3 dilated / plain Conv1d of a ResStack layer (voicefixer/vocoder/model/modules.py:592-609) as a Winograd tap-GEMM
// along the DILATED axis, in exact-fp32 MFMA arithmetic.  Outputs a dilation apart share their inputs:
//   F(2,3)  y[q], y[q+d]            from x[q-d .. q+2d]:  4 products per (co, ci) instead of 6
//   F(4,3)  y[q], .., y[q+3d]       from x[q-d .. q+4d]:  6 products instead of 12          <- convwg4_kernel below
// Round 2 shipped both as stand-alone kernels (convwg_kernel = F(2,3), convwg4_kernel = F(4,3)); since round 3 every
// stand-alone launch runs F(4,3) (the C = 128 stage and the condnet moved over once the dilation-1 instance existed), and
// so does the dilation-1 half of the fused C = 64 layer on its LDS tile (convw_kernel<.., FUSED = 3>, vfx_convw.inc: 229.0
// -> 223.5 ms per step on one box); F(2,3) survives as that layer's fallback for rows that are not 16-byte aligned and for
// C = 128 (convw_kernel<.., FUSED = 2>).  What the stand-alone F(2,3) kernel established and convwg4_kernel keeps:
//  * pair / quad index space: position q = n*d*blk + i*d + r (i < n, r < d) is output i of group blk*d + r, so a
//    workgroup's consecutive groups are runs of d consecutive positions;
//  * WEIGHTS transformed once on the host in float64 and packed [planes][Cin/8][Cout][8] (packing.pack_wino4 =
//    pack_direct of the transformed slabs), read straight from L2 as 16-byte A-operand vectors, two register sets;
//  * ACTIVATIONS: every thread loads its (channel, group) elements' taps with dword buffer loads (ONE vector offset per
//    tap -- out-of-row taps get an out-of-range offset and read 0, which IS the zero padding: no guard band, nothing masked
//    afterwards, per-row lengths cost nothing), pre-activation, B^T, planes to LDS [plane][channel][group], double buffered;
//  * the staging of chunk s+1 is WOVEN between the MFMAs of chunk s (sched_barrier after every MFMA pins the order);
//  * every accumulator starts at zero; bias and residual are added BEHIND the K loop (convwg4_kernel: see there), and the
//    in-place update of a ResStack pair (res == y) stays exact: a lane reads the residual elements it later writes;
//  * XCD-aware tile order with the Cout / BM channel blocks of a tile folded into the workgroup id.

// channel blocks of a tile adjacent in dispatch order on one XCD (see the kernel); VFX_WINO_MFOLD=0: development
static void convwg_fold_blocks(ConvArgs& a, dim3& grid, int gy) {
    static const bool off = VFX_DEV_ENV("VFX_WINO_MFOLD") && atoi(VFX_DEV_ENV("VFX_WINO_MFOLD")) == 0;
    a.nph_fold = 0;
    if (gy > 1 && a.xcd_chunk > 0 && !off) {
        a.nph_fold = gy;
        grid = dim3(grid.x * gy, 1, grid.z);
    }
}

// ======================================================================================================================
// convwg4_kernel: the same convolution as Winograd F(4,3) -- FOUR outputs a dilation apart share SIX products:
//   inputs d_j = x[q + (j-1)d], j = 0..5; outputs y_i = y[q + i*d], i = 0..3
//   V = B^T d:  V0 = 4d0 - 5d2 + d4, V1 = -4d1 - 4d2 + d3 + d4, V2 = 4d1 - 4d2 - d3 + d4,
//               V3 = -2d1 - d2 + 2d3 + d4, V4 = 2d1 - d2 - 2d3 + d4, V5 = 4d1 - 5d3 + d5
//   U = G w:    U0 = w0/4, U1 = -(w0+w1+w2)/6, U2 = -(w0-w1+w2)/6, U3 = w0/24 + w1/12 + w2/6, U4 = w0/24 - w1/12 + w2/6, U5 = w2
//   m_k = sum_ci U_k V_k;  y0 = m0+m1+m2+m3+m4, y1 = m1-m2+2(m3-m4), y2 = m1+m2+4(m3+m4), y3 = m1-m2+8(m3-m4)+m5
// 1.5 products per output instead of 3 (direct) or 2 (F(2,3)): another 25 % fewer fp32 MFMAs than convwg_kernel, at
// about three times the direct sum's rounding error (transform constants up to 8; fp32 operands and accumulators as everywhere:
// ~1e-6 relative on a 256-channel sum, tests/test_ops_gpu.py::test_conv1d_winograd4).
// Quad index space: position q = 4d*blk + i*d + r (i < 4, r < d) is output i of quad Q = blk*d + r.  A workgroup owns
// 32*WGP consecutive quads x 32*WGM output channels; a wave 32 rows x 32 quads x 6 planes = 6 accumulator tiles (96 VGPRs,
// against 128 for the pair kernel).  Staging, weights (packing.pack_wino4: [6 planes][Cin/8][Cout][8]), the woven loop and
// the dispatch order follow convwg_kernel; A vectors are prefetched one 8-channel group ahead in two register sets.
// Bias and residual never pass through the accumulators' partial sums.  All six planes start at zero (the C operand of the first
// k-step).  The run-time instance (SPEC 0) adds bias, then residual, to the transformed outputs in its epilogue, in torch's
// order; the specialised ones close plane 1 with one extra MFMA  acc[1] += bias (x) 1  behind the last k-step (y_i = m1 + ...
// for all four outputs), exactly as convwg4p_kernel / convwg4x_kernel do, so that the three kernels return the same bits.
// Until tests/test_wg4_gpu.py measured it, planes (0, 1, 3, 5) STARTED at the unique solution of A^T m = r + b with m2 = m4 = 0
// (m3 = (t2-t1)/2, m1 = 2 t1 - t2, m0 = t0 - m1 - m3, m5 = t3 - m1 - 8 m3, t_i = residual_i + bias; SPEC 1 / 2: plane 1 at the
// bias): every one of the Cin partial sums then rounded at several times the residual, and the output transform multiplied
// that by up to 8 -- 14 - 31 x the fp32 statement's error under heavy-tailed weight-norm gains (profiles/wg4_parity.txt).
// (The 3x3 convolutions of the ResUNet ran here in round 2, kernel columns as virtual chunks; now convwg4s_kernel.)
// Occupancy is not what bounds this kernel.  Round 2: three waves per SIMD with ~10 spilled registers, slower.  Round 3: the
// A operands as two sets of 8-BYTE vectors (24 instead of 48 registers: 150-166 VGPRs, three waves per SIMD, no spills)
// ran exactly as fast as this two-wave form (C = 256: 3.10-3.16 ms, C = 512: 1.90 ms) while doubling the L1 line accesses
// of the A stream.  The counters say where the time goes (tools/pmc_diag.sh, profiles/r03_pmc_diag_*.txt): every A vector
// feeds ONE MFMA here (wave tile 32 rows x 32 quads; the round-2 F(2,3) kernel's 64 pairs reused it twice), so the L1 serves
// 0.58 line accesses per CU cycle and the texture addresser's FIFOs are full 5-6 % of the time (8-byte form: 0.81 / 19-22 %;
// F(2,3) on the same layer: 0.42 / 1.6-2 %, matrix pipe 83 % busy against 77 % here) -- and the shader clock under this load
// is 2.24 GHz, not the 2.4 GHz the 157.3 TFLOP/s peak assumes.
//
// D1 (round 3): dilation 1 -- every SECOND convolution of a ResStack layer, the one that carries the in-place residual.  In
// the pipeline those launches ran 0.5-0.6 ms (C = 256) behind their dilated partners (profiles/r03_per_dispatch_before_d1.txt): the
// four outputs of a quad are ADJACENT positions, so with one dword per lane and instruction every tap load, residual load
// and store touches 32 lanes x 4 bytes at a 16-byte stride.  Here a quad is what it is in memory, an aligned float4: one
// 16-byte load for taps 1-4 (+ two dwords for x[4Q-1], x[4Q+4]), one 16-byte residual load and one 16-byte store per
// accumulator row.  Taps past the row's end are zeroed by selects (a vector cannot rely on the out-of-range offset); the one
// quad that straddles the end of a row whose length is not a multiple of 4 takes dword loads / stores under a
// workgroup-uniform branch.
//
// XD (round 4): how many chunks AHEAD of the multiplying one the tap loads of the activations run.  XD = 2 is the round-2/3
// form: one register set, the taps of chunk s+2 are issued during steps 2-3 / 6-7 of chunk s and consumed at steps 0 / 4 of
// chunk s+1 -- 27 MFMAs later, i.e. 0.75 us when the wave has the matrix pipe to itself and 1.5 us when it shares it, which
// is about one HBM round trip under load: the s_waitcnt in front of every chunk's first transform (vmcnt is in order, so
// the A vectors queue behind it) is then where the pipe idles.  XD = 3: two register sets used alternately, the taps of
// chunk s+3 are issued during chunk s -- one whole chunk (48 MFMAs) more distance for 6 * NSLOT more VGPRs.
#ifndef VFX_WG4_OCC
#define VFX_WG4_OCC 2
#endif
// Development ablations of convwg4_kernel's K loop (wrong results, timing only; tools/conv_bench.py on `make dev DEVDEFS=-DVFX_WG4_ABL=n` builds):
//   1 = every A vector from 8-channel group 0 (the weights of one group: L1 hits instead of the L2 stream)
//   2 = no tap loads in the loop (the registers keep chunk 0's taps)      4 = no B-fragment reads from LDS (fragments of k-step 0 reused)
//   8 = no transform / LDS writes in the loop                            16 = no barrier between chunks
#ifndef VFX_WG4_ABL
#define VFX_WG4_ABL 0
#endif
#ifndef VFX_WG4_SPEC2_OCC
#define VFX_WG4_SPEC2_OCC 2   // waves per SIMD the <4,1,..,SPEC = 2> instance is bounded to (174 VGPRs as it compiles; 3 = 168 VGPRs
                              // with 6 spilled, two reloads inside the K loop: measured equal, profiles/r05_convwg4_spec_pk_ab.txt)
#endif
// Packed fp32 staging (round 5, measured and removed): the D1 = false instances staged TWO elements per thread with v_pk_mul / v_pk_fma /
// v_pk_add on register pairs and ran their output transform on pairs of accumulator rows -- a third fewer VALU instructions in the K
// loop and the epilogue, bit-identical results, and no change in launch or step time (profiles/r05_convwg4_spec_pk_ab.txt).
// PRE (round 4): false = the launch has no pre-activation (every SECOND convolution of a ResStack layer: the first one applies the
// leaky ReLU in its epilogue), so the two VALU operations per tap that evaluate max(x, 1.0 * x) are not compiled in.  On this chip
// the fp32 MFMA has the fp32 VALU's peak rate and SQ_VALU_MFMA_COEXEC_CYCLES reads 0 for this kernel: every VALU instruction of
// the staging takes its issue cycles out of the matrix pipe's, so instructions that compute nothing are worth removing.
// SPEC (round 5): what is known about the launch at compile time, so that prologue and epilogue hold no instruction that computes
// nothing (every VALU instruction takes its issue cycles out of the matrix pipe's, see PRE):
//   0  anything (residual / bias / post-activation decided at run time; bias and residual are loaded and added in the epilogue)
//   1  the FIRST convolution of a ResStack layer: no residual, leaky ReLU after
//   2  the SECOND one (D1 only): residual, no activation after.  The residual quads are LOADED IN THE EPILOGUE (four accumulator
//      rows per batch, two batches in flight, into registers the A vectors and taps have left by then) and added to the outputs: 4
//      additions per accumulator row instead of 4 moves + the 12-operation solve.  The load latency is exposed to this workgroup
//      only -- the workgroups it shares the CU with are in their K loops meanwhile (tools/wg4_timeline.py: co-resident workgroups
//      run half a lifetime apart).  First attempt, measured and dropped: the quads loaded in the prologue and KEPT through the K
//      loop (239 VGPRs).
// Static VALU count of the <4,1> instances, prologue / epilogue path: 424 / ~440 (SPEC 0) -> 97 / 329 (SPEC 2), 174 / 300 (SPEC 1).
// Measured: the launch and the step do NOT get faster (profiles/r05_convwg4_spec_pk_ab.txt) -- prologue and epilogue already ran
// under the co-resident workgroups' K loops, and the kernel runs at the chip's power cap (profiles/r05_power_cap.txt): fewer
// instructions per product pay as energy -- a slightly higher clock -- not as issue cycles.
// No accumulator is initialised at all: the first k-step's MFMAs of all six planes take the inline constant 0 as their C operand.
template <int WGM, int WGP, bool D1 = false, int XD = 2, bool PRE = true, int SPEC = 0>
__global__ __launch_bounds__(256, (SPEC == 2 && WGM == 4) ? VFX_WG4_SPEC2_OCC : VFX_WG4_OCC) void convwg4_kernel(const ConvArgs a) {
    static_assert(WGM * WGP == 4, "four waves");
    static_assert(SPEC == 0 || (SPEC == 1 && PRE) || (SPEC == 2 && D1 && !PRE), "specialised instances");
    constexpr bool ZSTART = true;                 // accumulators start from the MFMA's C operand (0), not from registers
    static_assert(XD == 2 || XD == 3, "prefetch distance");
    constexpr int XSETS = XD - 1;
    constexpr int KC = 16, NSTEP = KC / 2;
    constexpr int BM = 32 * WGM, BQ = 32 * WGP;
    constexpr int CG = 256 / BQ;                  // channel groups of the staging map
    constexpr int NSLOT = KC / CG;                // staged (channel, quad) elements per thread per chunk: 2 (<4,1>) or 4 (<2,2>)
    constexpr int SPAN = NSTEP / NSLOT;           // k-pair steps an element's staging is spread over: 4 or 2
    constexpr int PLANE = KC * BQ;
    constexpr int BUF = 6 * PLANE;
    static_assert(CG % 2 == 0 && (SPAN == 2 || SPAN == 4), "staging map");
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
    const int d = D1 ? 1 : a.wg_d;
    const float inv_d = 1.0f / (float)d;
    const int Lrow = a.x_rows ? __builtin_amdgcn_readfirstlane(a.x_rows[b]) : a.Lin;
    const int Q0 = bx * BQ;
    {
        const int nblk = fast_div(Lrow + 4 * d - 1, 4 * d, 0.25f * inv_d);
        if (Q0 >= nblk * d) return;
    }
    if (a.stagger) {
        // development (VFX_WG4_STAGGER, -DVFX_DEV builds): the workgroups of the first residency round that share a SIMD start
        // a.stagger x s_sleep(127) apart (wave slot 0 at once, slot 1 one unit later, ...); equal lifetimes then keep them apart
        const int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        if (lin < a.stagger_wgs) {
            const int slot = __builtin_amdgcn_s_getreg((3 << 11) | 4) & 15;   // HW_ID.WAVE_ID
            for (int i = 0; i < slot * a.stagger; ++i) __builtin_amdgcn_s_sleep(127);
        }
    }
    DBG_T(dbg_t0);                                // (-DVFX_ABL=8 builds: phase timers of wave 0, tools/wg4_phase.py)
#if VFX_ABL & 8
    unsigned long long dbg_bar = 0;
#define WG4_SYNC() do { DBG_T(b0_); __syncthreads(); DBG_T(b1_); dbg_bar += b1_ - b0_; } while (0)
#else
#define WG4_SYNC() do { if (!(VFX_WG4_ABL & 16)) __syncthreads(); } while (0)
#endif
    const int xcs = (int)a.x_cs;
    auto quad_q = [&](int Q) {                    // first output of quad Q
        if constexpr (D1) return 4 * Q;
        const int blk = fast_div(Q, d, inv_d);
        return 4 * d * blk + (Q - blk * d);
    };
    // D1: (uniform) this tile holds the quad that straddles the end of a row whose length is not a multiple of 4
    const bool has_tail = D1 && (Lrow & 3) != 0 && (Lrow >> 2) >= Q0 && (Lrow >> 2) < Q0 + BQ;

    // ---- staging map: quad = tid % BQ, channel group = tid / BQ; element j = channel cg + j*CG (same parity as cg)
    const int sq = tid % BQ, cg = tid / BQ;
    int xvoff[6];                                 // vector offset of tap j, out of range when the tap is padding
    bool xin[4] = {true, true, true, true};       // D1: tap 1 + i (position 4Q + i) lies inside the row
    {
        const int q = quad_q(Q0 + sq);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int p = q + (j - 1) * d;
            xvoff[j] = (p >= 0 && p < Lrow) ? (cg * xcs + p) * 4 : VFX_W_OOB;   // outside the row: reads 0 = the zero padding
        }
        if constexpr (D1) {
            // xvoff[1] addresses the whole aligned vector x[4Q .. 4Q+3] (loaded when its first element is inside the row)
#pragma unroll
            for (int i = 0; i < 4; ++i) xin[i] = q + i < Lrow;
        }
    }
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.x) + (long long)b * a.x_bs, (short)0, 0x7fffffff, 0x00020000);
    const float slope = a.pre_act == VFX_PRE_LRELU ? a.pre_slope : 1.f;
    auto x_soff = [&](int v) { return v * KC * xcs * 4; };
    // LDS [plane][channel][quad].  BQ == 32: lanes 0-31 / 32-63 of a B-fragment read (channels 2kk / 2kk+1) are 32 dwords
    // apart = disjoint banks as they are; BQ == 64: odd channels are rotated by 32 columns as in convwg_kernel
    const int wcol = BQ == 32 ? sq : ((sq & ~63) | ((sq + 32 * (cg & 1)) & 63));
    float* const wbase = smem + cg * BQ + wcol;

    float xv[XSETS][NSLOT][6];
    // the tap loads of element j (into register set SET); D1: part 0 = the 16-byte vector (taps 1-4), parts 1 / 2 = taps 0 / 5; else part t = tap t
    auto x_load_part = [&](auto set_tag, int j, int part, int s0) {
        constexpr int SET = decltype(set_tag)::value;
        const int so = s0 + j * CG * xcs * 4;
        if constexpr (D1) {
            if (part == 0) {
                const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, xvoff[1], so, 0);
                xv[SET][j][1] = __uint_as_float(r.x); xv[SET][j][2] = __uint_as_float(r.y);
                xv[SET][j][3] = __uint_as_float(r.z); xv[SET][j][4] = __uint_as_float(r.w);
            } else if (part == 1) {
                xv[SET][j][0] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xrsrc, xvoff[0], so, 0));
            } else if (part == 2) {
                xv[SET][j][5] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xrsrc, xvoff[5], so, 0));
            }
        } else {
            xv[SET][j][part] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xrsrc, xvoff[part], so, 0));
        }
    };
    auto x_load = [&](auto set_tag, int v) {
        const int s0 = x_soff(v);
#pragma unroll
        for (int j = 0; j < NSLOT; ++j)
#pragma unroll
            for (int t = 0; t < 6; ++t) x_load_part(set_tag, j, t, s0);
    };
    // pre-activation (leaky ReLU keeps the zeros of the padding taps) + B^T of element j
    auto x_transform = [&](auto set_tag, int j, float (&V)[6]) {
        constexpr int SET = decltype(set_tag)::value;
        float e[6];
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            e[t] = PRE ? fmaxf(xv[SET][j][t], xv[SET][j][t] * slope) : xv[SET][j][t];
            if constexpr (D1) {
                if (t >= 1 && t <= 4) e[t] = xin[t - 1] ? e[t] : 0.f;   // (the vector was loaded whole)
            }
        }
        const float s1 = fmaf(-4.f, e[2], e[4]), s2 = fmaf(-4.f, e[1], e[3]);
        const float s3 = e[4] - e[2], s4 = e[3] - e[1];
        V[0] = fmaf(4.f, e[0], fmaf(-5.f, e[2], e[4]));
        V[1] = s1 + s2;
        V[2] = s1 - s2;
        V[3] = fmaf(2.f, s4, s3);                 // (the factor 2 rides on the FMA: 12 VALU operations for the six planes)
        V[4] = fmaf(-2.f, s4, s3);
        V[5] = fmaf(4.f, e[1], fmaf(-5.f, e[3], e[5]));
    };
    auto x_write = [&](auto set_tag, float* dst) {
#pragma unroll
        for (int j = 0; j < NSLOT; ++j) {
            float V[6];
            x_transform(set_tag, j, V);
#pragma unroll
            for (int k = 0; k < 6; ++k) dst[j * CG * BQ + k * PLANE] = V[k];
        }
    };

    // ---- A operands: [6 planes][Cin/8][Cout][8]; two register sets, one 8-channel group each
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wd), (short)0, 0x7fffffff, 0x00020000);
    const int avoff = ((m0 + wm * 32 + lo) * 8 + 4 * hi) * 4;
    const int gstride = a.Cout * 32;
    const int pstride = (a.CinPad >> 3) * gstride;
    float4 aw[2][6];
    auto a_goff = [&](int vg) { return (VFX_WG4_ABL & 1) ? 0 : vg * gstride; };   // scalar byte offset of plane 0 of 8-channel group vg
    auto a_load_one = [&](auto set_tag, int k, int goff) {
        constexpr int SET = decltype(set_tag)::value;
        const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, avoff, k * pstride + goff, 0);
        aw[SET][k] = make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
    };

    // ---- the issue block: every load the prologue needs, in the order in which the results are consumed (vmcnt counts in
    // order): the taps of chunk 0, the first A vectors.  Nothing but loads may stand in this block: any arithmetic on a loaded
    // value costs the precise vmcnt bookkeeping.  (Bias and residual are loaded in the epilogue.)
    const int row0 = m0 + wm * 32;
    f32x16 acc[6];
    const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.res ? a.res : a.x) + (long long)b * a.r_bs, (short)0, 0x7fffffff, 0x00020000);
    using X0 = std::integral_constant<int, 0>;
    using X1 = std::integral_constant<int, XSETS - 1>;   // (the second register set; the first again when there is one)
#if VFX_ABL & 8
    __builtin_amdgcn_sched_barrier(0);
#endif
    DBG_T(dbg_tr);
#if VFX_ABL & 8
    __builtin_amdgcn_sched_barrier(0);
#endif
    x_load(X0{}, 0);
#pragma unroll
    for (int k = 0; k < 6; ++k) a_load_one(std::integral_constant<int, 0>{}, k, a_goff(0));
#if VFX_ABL & 8
    __builtin_amdgcn_sched_barrier(0);
#endif
    DBG_T(dbg_ts);
    __builtin_amdgcn_sched_barrier(0);            // (nothing that consumes a loaded value may be scheduled up into the issue block)
    DBG_T(dbg_ta);
    // SPEC 1 / 2: the bias as the A operand of the MFMA that closes plane 1 (lanes 0-31: k-column 0; see convwg4p_kernel)
    float bias_a = 0.f;
    if constexpr (SPEC != 0) bias_a = (a.bias && hi == 0) ? a.bias[row0 + lo] : 0.f;

    // ---- B fragments: lane (column lo, k-half hi) of k-pair u of plane k reads xs[k*PLANE + (2u + hi)*BQ + column]
    // (BQ == 64: the wave's 32 quads wp*32 .. +31; odd channels are rotated by 32 within the 64-column row)
    const int bcol = BQ == 32 ? lo : ((wp * 32 + lo + 32 * hi) & 63);
    const int boffs = hi * BQ + bcol;

    // One chunk (8 k-pair steps x 6 MFMAs) with the staging of the next chunk and the A vectors of the next group woven in:
    // element s of the thread is handled during steps s*SPAN .. s*SPAN + SPAN - 1 (first half: transform + 6 LDS writes,
    // second half: its 6 tap loads for the chunk after next); the 6 A vectors of the next 8-channel group are loaded in the
    // first step of each group into the register set the previous group used.
    // first_tag (chunk 0 only): the MFMAs of k-step 0 start the accumulators -- C = 0 (inline constant)
    auto mma_chunk = [&](auto set_tag, auto first_tag, const float* xs, float* wdst, int xchunk, int agrp0, int glast) {
        constexpr bool FIRST = decltype(first_tag)::value;
        const float* bp = xs + boffs;
        const int agrp1 = a_goff(min(agrp0 + 1, glast)), agrp2 = a_goff(min(agrp0 + 2, glast));
        float bf[6];                              // single set: the fragment of step u+1 is fetched right after MFMA (u, k) issued
#pragma unroll
        for (int k = 0; k < 6; ++k) bf[k] = bp[k * PLANE];
        const int xs0 = x_soff(xchunk);
        float V[6];
#pragma unroll
        for (int u = 0; u < NSTEP; ++u) {
            const int el = u / SPAN, ph = u % SPAN;   // element and phase of its staging
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                // micro-slot in front of MFMA k of step u
                constexpr bool ST = !(VFX_WG4_ABL & 8), LD = !(VFX_WG4_ABL & 2);   // (development ablations)
                if constexpr (SPAN == 4) {
                    if (ST && ph == 0 && k == 0) x_transform(set_tag, el, V);
                    if (ST && ph == 0 && k < 3) wdst[el * CG * BQ + k * PLANE] = V[k];
                    if (ST && ph == 1 && k < 3) wdst[el * CG * BQ + (k + 3) * PLANE] = V[k + 3];
                    if (LD && ph == 2 && k < 3) x_load_part(set_tag, el, k, xs0);
                    if (LD && ph == 3 && k < 3) x_load_part(set_tag, el, k + 3, xs0);
                } else {
                    if (ST && ph == 0 && k == 0) x_transform(set_tag, el, V);
                    if (ST && ph == 0) wdst[el * CG * BQ + k * PLANE] = V[k];
                    if (LD && ph == 1) x_load_part(set_tag, el, k, xs0);
                }
                // A vectors of the NEXT group, all six in the first step of this one (three steps = 18 MFMAs ahead of their
                // first use): step 0 -> group agrp0 + 1 into set 1, step 4 -> group agrp0 + 2 into set 0
                if (u == 0) a_load_one(std::integral_constant<int, 1>{}, k, agrp1);
                if (u == 4) a_load_one(std::integral_constant<int, 0>{}, k, agrp2);
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

    const int S = a.Cin / KC;                     // chunks (host: Cin % 32 == 0, so S is even)
    const int glast = 2 * S - 1;                  // last virtual 8-channel group
    x_write(X0{}, wbase);
    DBG_T(dbg_tb);
    x_load(X0{}, S > 1 ? 1 : 0);
    if constexpr (XSETS == 2) x_load(X1{}, min(2, S - 1));
    __builtin_amdgcn_sched_barrier(0);
    DBG_T(dbg_tc);
    WG4_SYNC();
    DBG_T(dbg_t1);
    using NotFirst = std::false_type;
    int s_begin = 0;
    if constexpr (ZSTART) {                       // chunks 0 and 1 peeled: chunk 0's first k-step starts the accumulators at zero
        mma_chunk(X0{}, std::true_type{}, smem, wbase + BUF, min(XD, S - 1), 0, glast);
        WG4_SYNC();
        mma_chunk(X1{}, NotFirst{}, smem + BUF, wbase, min(1 + XD, S - 1), 2, glast);
        WG4_SYNC();
        s_begin = 2;
    }
#pragma unroll 1
    for (int s = s_begin; s < S; s += 2) {
        // chunk s (LDS buffer 0): stages chunk s+1 (register set 0) into buffer 1, reloads the set with the taps of chunk
        // s+2 (XD = 2) / s+3 (XD = 3); A groups 2s+1, 2s+2
        mma_chunk(X0{}, NotFirst{}, smem, wbase + BUF, min(s + XD, S - 1), 2 * s, glast);
        WG4_SYNC();
        // chunk s+1 (buffer 1): stages chunk s+2 (set 0 / 1) into buffer 0, reloads with chunk s+3 / s+4; A groups 2s+3, 2s+4 (clamped)
        mma_chunk(X1{}, NotFirst{}, smem + BUF, wbase, min(s + 1 + XD, S - 1), 2 * s + 2, glast);
        WG4_SYNC();
    }
    DBG_T(dbg_t2);
    if constexpr (SPEC != 0) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(bias_a, 1.0f, acc[1], 0, 0, 0);   // + bias, rounded once

    // ---- output transform, activation, stores
    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(
        a.y + (long long)b * a.y_bs, (short)0, 0x7fffffff, 0x00020000);
    const int ycs4 = (int)a.y_cs * 4;
    const int post = a.post_act;
    const float ps = a.post_slope;
    int yv[4];
    int yvq = VFX_W_OOB;
    {
        const int q = quad_q(Q0 + wp * 32 + lo);
#pragma unroll
        for (int i = 0; i < 4; ++i) yv[i] = q + i * d < Lrow ? (4 * hi * (int)a.y_cs + q + i * d) * 4 : VFX_W_OOB;
        if constexpr (D1) {
            const bool full = q + 3 < Lrow;
            yvq = full ? yv[0] : VFX_W_OOB;
#pragma unroll
            for (int i = 0; i < 4; ++i) yv[i] = full ? VFX_W_OOB : yv[i];
        }
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
    if constexpr (SPEC == 0) {
        // The run-time instance: bias and residual are loaded here -- the A vectors and taps have left their registers -- and added
        // to the transformed outputs, bias first, in torch's order.  The sums go back into the registers of planes 0 .. 3 (dead after
        // the transform), so that the post-activation loops below find them there.  In place (res == y): every lane loads exactly the
        // residual elements it stores afterwards, and no other lane or workgroup touches them.
        const __amdgpu_buffer_rsrc_t brsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(a.bias ? a.bias : a.x), (short)0, 0x7fffffff, 0x00020000);
        u32x4 bq[4];                              // bias of rows row0 + 4 hi + 8 g + (0..3); no bias: out of range = zeros
        const int bvoff = a.bias ? (row0 + 4 * hi) * 4 : VFX_W_OOB;
#pragma unroll
        for (int g = 0; g < 4; ++g) bq[g] = __builtin_amdgcn_raw_buffer_load_b128(brsrc, bvoff, g * 32, 0);
        const int cs4 = (int)a.r_cs * 4;
        const int qe = quad_q(Q0 + wp * 32 + lo);
        int rv[4];                                // single residual elements (D1: the straddling quad's only); no residual: out of range = zeros
        int rvq = VFX_W_OOB;                      // D1: the whole quad as one 16-byte vector (all four outputs inside the row)
#pragma unroll
        for (int i = 0; i < 4; ++i) rv[i] = (a.res && qe + i * d < Lrow) ? (4 * hi * (int)a.r_cs + qe + i * d) * 4 : VFX_W_OOB;
        if constexpr (D1) {
            const bool full = qe + 3 < Lrow;
            rvq = full ? rv[0] : VFX_W_OOB;
#pragma unroll
            for (int i = 0; i < 4; ++i) rv[i] = full ? VFX_W_OOB : rv[i];
        }
        u32x4 rq[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int soff = (row0 + (r & 3) + 8 * (r >> 2)) * cs4;
            if constexpr (D1) {
                rq[r] = __builtin_amdgcn_raw_buffer_load_b128(rrsrc, rvq, soff, 0);
            } else {
                rq[r].x = __builtin_amdgcn_raw_buffer_load_b32(rrsrc, rv[0], soff, 0);
                rq[r].y = __builtin_amdgcn_raw_buffer_load_b32(rrsrc, rv[1], soff, 0);
                rq[r].z = __builtin_amdgcn_raw_buffer_load_b32(rrsrc, rv[2], soff, 0);
                rq[r].w = __builtin_amdgcn_raw_buffer_load_b32(rrsrc, rv[3], soff, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const u32x4 bg = bq[r >> 2];
            const float bb = __uint_as_float((r & 3) == 0 ? bg.x : ((r & 3) == 1 ? bg.y : ((r & 3) == 2 ? bg.z : bg.w)));
            float y[4];
            outs(r, y);
            float t[4] = {__uint_as_float(rq[r].x), __uint_as_float(rq[r].y), __uint_as_float(rq[r].z), __uint_as_float(rq[r].w)};
            if (D1 && has_tail && a.res) {        // (workgroup-uniform, one tile per row at most; every other lane's offsets read 0,
                                                  // this quad's vector load returned zeros)
                const int soff = (row0 + (r & 3) + 8 * (r >> 2)) * cs4;
#pragma unroll
                for (int i = 0; i < 4; ++i) t[i] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, rv[i], soff, 0));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][r] = (y[i] + bb) + t[i];
        }
    }
    auto sums = [&](int r, float (&y)[4]) {       // SPEC 0: transformed output + bias + residual of accumulator row r (see above)
        y[0] = acc[0][r]; y[1] = acc[1][r]; y[2] = acc[2][r]; y[3] = acc[3][r];
    };
    if constexpr (SPEC == 1) {                    // first convolution of a ResStack layer: leaky ReLU, nothing else
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int soff = (row0 + (r & 3) + 8 * (r >> 2)) * ycs4;
            float y[4];
            outs(r, y);
#pragma unroll
            for (int i = 0; i < 4; ++i) y[i] = fmaxf(y[i], y[i] * ps);   // (0 <= slope <= 1, checked on the host)
            store4(y, soff);
        }
    } else if constexpr (SPEC == 2) {             // second convolution: + residual (loaded here), no activation
        // four accumulator rows per batch, two batches in flight (32 registers -- the A vectors and taps have left 70)
        const int cs4 = (int)a.r_cs * 4;
        const int qe = quad_q(Q0 + wp * 32 + lo);
        const bool full = qe + 3 < Lrow;
        const int rvq2 = full ? (4 * hi * (int)a.r_cs + qe) * 4 : VFX_W_OOB;
        int tv[4];                                // the straddling quad's single elements (has_tail only)
#pragma unroll
        for (int i = 0; i < 4; ++i) tv[i] = (qe + i < Lrow && !full) ? (4 * hi * (int)a.r_cs + qe + i) * 4 : VFX_W_OOB;
        u32x4 rl[2][4];
        auto res_load = [&](int bt, u32x4 (&dst)[4]) {
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[e] = __builtin_amdgcn_raw_buffer_load_b128(rrsrc, rvq2, (row0 + e + 8 * bt) * cs4, 0);
        };
        res_load(0, rl[0]);
        res_load(1, rl[1]);
        __builtin_amdgcn_sched_barrier(0);
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
                if (has_tail) {                   // (workgroup-uniform, one tile per row at most; every other lane's offsets read 0,
                                                  // this quad's vector load returned zeros)
#pragma unroll
                    for (int i = 0; i < 4; ++i) y[i] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, tv[i], srow * cs4, 0));
                }
                store4(y, srow * ycs4);
            }
            if (bt + 2 < 4) res_load(bt + 2, rl[bt & 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
    } else if (post == VFX_POST_NONE) {                  // (the residual-carrying convolutions of a ResStack: nothing to evaluate per output)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int soff = (row0 + (r & 3) + 8 * (r >> 2)) * ycs4;
            float y[4];
            sums(r, y);
            store4(y, soff);
        }
    } else if (post == VFX_POST_LRELU) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int soff = (row0 + (r & 3) + 8 * (r >> 2)) * ycs4;
            float y[4];
            sums(r, y);
#pragma unroll
            for (int i = 0; i < 4; ++i) y[i] = fmaxf(y[i], y[i] * ps);   // (0 <= slope <= 1, checked on the host)
            store4(y, soff);
        }
    } else {
#pragma unroll 1
        for (int r = 0; r < 16; ++r) {
            const int soff = (row0 + (r & 3) + 8 * (r >> 2)) * ycs4;
            float y[4];
            sums(r, y);
#pragma unroll
            for (int i = 0; i < 4; ++i) y[i] = vfx_post(y[i], post, ps);
            store4(y, soff);
        }
    }
#undef WG4_SYNC
#if VFX_ABL & 8
    DBG_T(dbg_t3);
    if (tid == 0 && g_trace_buf) {                // per-workgroup timeline (tools/wg4_timeline.py): one record per workgroup, indexed by its
                                                  // linear id -- no atomics (the phase totals below serialise 14 atomics per workgroup on one line)
        const unsigned long long lin = blockIdx.x + (unsigned long long)gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        if (lin < g_trace_cap) {
            unsigned long long* t = g_trace_buf + 6ull * lin;
            t[0] = (unsigned long long)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
                   ((unsigned long long)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);   // HW_ID | XCC_ID << 32
            t[1] = lin + 1;                       // (0 = no record)
            t[2] = dbg_t0; t[3] = dbg_t1; t[4] = dbg_t2; t[5] = dbg_t3;
        }
    } else if (tid == 0) {
        atomicAdd(&g_dbg[8], dbg_t1 - dbg_t0);   // prologue (incl. the first barrier)
        atomicAdd(&g_dbg[0], dbg_ta - dbg_t0);   //   of which: set-up + issue of the first loads
        atomicAdd(&g_dbgx[0], dbg_tr - dbg_t0);  //     set-up (index math, descriptors, bias loads)
        atomicAdd(&g_dbgx[1], dbg_ta - dbg_ts);  //     residual loads issued
        atomicAdd(&g_dbgx[2], dbg_ts - dbg_tr);  //     first tap loads and A vectors issued
        atomicAdd(&g_dbg[1], dbg_tb - dbg_ta);   //   chunk 0 arrived, transformed, written to LDS
        atomicAdd(&g_dbg[2], dbg_tc - dbg_tb);   //   next tap loads issued, residual arrived, start values
        atomicAdd(&g_dbg[9], dbg_t1 - dbg_tc - (dbg_bar ? 0 : 0));   //   first barrier
        atomicAdd(&g_dbg[4], dbg_t2 - dbg_t1);   // K loop
        atomicAdd(&g_dbg[5], dbg_t3 - dbg_t2);   // epilogue (issue of the stores, not their drain)
        atomicAdd(&g_dbg[3], dbg_bar);           // of which: waiting at the barriers
        atomicAdd(&g_dbg[6], 1ull);
        atomicAdd(&g_dbg[7], (unsigned long long)S);
    }
#endif
}

template <int WGM, int WGP, bool D1 = false, int XD = 2, bool PRE = true, int SPEC = 0>
static int launch_wg4_xd(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t s) {
    return vfx_launch<convwg4_kernel<WGM, WGP, D1, XD, PRE, SPEC>>(grid, dim3(256), lds, s, a);
}

template <int WGM, int WGP, bool D1 = false>
static int launch_wg4_one(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t s) {
#ifdef VFX_DEV
    // development: VFX_WG4_XD=3 = tap loads three chunks ahead (measured: no gain, profiles/r04_convwg4_prologue_ab.txt);
    // VFX_WG4_SPEC=0 = the run-time instance everywhere (round-5 A/B)
    static const int xd = VFX_DEV_ENV("VFX_WG4_XD") ? atoi(VFX_DEV_ENV("VFX_WG4_XD")) : 2;
    if (xd == 3) return launch_wg4_xd<WGM, WGP, D1, 3, true>(a, grid, lds, s);
    static const int spec_mask = VFX_DEV_ENV("VFX_WG4_SPEC") ? atoi(VFX_DEV_ENV("VFX_WG4_SPEC")) : 3;
#else
    constexpr int spec_mask = 3;
#endif
    // the two launches a ResStack layer consists of have instances of their own (SPEC, see the kernel)
    if ((spec_mask & 1) && !a.res && a.pre_act == VFX_PRE_LRELU && a.post_act == VFX_POST_LRELU && (!a.bias || vfx_aligned16(a.bias)))
        return launch_wg4_xd<WGM, WGP, D1, 2, true, 1>(a, grid, lds, s);
    if constexpr (D1) {
        if ((spec_mask & 2) && a.res && a.pre_act == VFX_PRE_NONE && a.post_act == VFX_POST_NONE && (!a.bias || vfx_aligned16(a.bias)))
            return launch_wg4_xd<WGM, WGP, true, 2, false, 2>(a, grid, lds, s);
    }
    return a.pre_act == VFX_PRE_NONE ? launch_wg4_xd<WGM, WGP, D1, 2, false>(a, grid, lds, s)
                                     : launch_wg4_xd<WGM, WGP, D1, 2, true>(a, grid, lds, s);
}

static int try_launch_convwg4p(ConvArgs a, int ntiles, int gy, bool wide, bool d1vec, hipStream_t stream);   // vfx_convwg4p.inc
static int try_launch_convwg4x(ConvArgs a, long long nquads, bool d1vec, hipStream_t stream);                // vfx_convwg4x.inc
#ifndef VFX_WG4X_DEFAULT
#define VFX_WG4X_DEFAULT 1    // 1: the wide ResStack launches run on the re-blocked wave tile (convwg4x_kernel); A/B in profiles/r06_convwg4x_ab.txt
#endif

// k = 3 convolution on convwg4_kernel (Winograd F(4,3), weights packing.pack_wino4); same contract as try_launch_convwg
static int try_launch_convwg4(ConvArgs a, const vfx_tensor* x, int nphase, const PhaseSpec* phs, const float* wg4,
                              hipStream_t stream) {
    static const bool off = (VFX_DEV_ENV("VFX_WINO") && atoi(VFX_DEV_ENV("VFX_WINO")) == 0) ||
                            (VFX_DEV_ENV("VFX_WINO4") && atoi(VFX_DEV_ENV("VFX_WINO4")) == 0);   // development
    if (off || !wg4 || !vfx_aligned16(wg4)) return VFX_ENOTSUP;
    if (nphase != 1 || phs[0].ntaps != 3 || phs[0].ooff != 0) return VFX_ENOTSUP;
    const int d = phs[0].taps[2].off;
    if (d < 1 || phs[0].taps[0].off != -d || phs[0].taps[1].off != 0) return VFX_ENOTSUP;
    for (int t = 0; t < 3; ++t)
        if (phs[0].taps[t].slab != t) return VFX_ENOTSUP;
    if (a.pad_mode != VFX_PAD_ZERO || a.in_mask || a.out_mask) return VFX_ENOTSUP;
    if (a.pre_act != VFX_PRE_NONE && a.pre_act != VFX_PRE_LRELU) return VFX_ENOTSUP;
    // leaky ReLU is evaluated as max(v, slope * v): slopes outside [0, 1] take the direct kernels
    if (a.pre_act == VFX_PRE_LRELU && !(a.pre_slope >= 0.f && a.pre_slope <= 1.f)) return VFX_ENOTSUP;
    if (a.post_act == VFX_POST_LRELU && !(a.post_slope >= 0.f && a.post_slope <= 1.f)) return VFX_ENOTSUP;
    if (!plain_output_map(a, nphase, phs[0].ooff) || a.y_ls != 1 || a.Lq != a.Lin) return VFX_ENOTSUP;
    if (a.res && a.r_ls != 1) return VFX_ENOTSUP;
    if (a.Cin % 32 != 0 || a.Cout % 64 != 0 || a.Cin != a.CinPad) return VFX_ENOTSUP;
    static const bool square = VFX_DEV_ENV("VFX_WINO4_SQUARE") && atoi(VFX_DEV_ENV("VFX_WINO4_SQUARE")) != 0;   // development: 64 x 64 tiles everywhere
    const bool wide = a.Cout % 128 == 0 && !square;
    if (!offsets_fit31(((long long)a.Cin * a.x_cs + a.Lin) * 4) || !offsets_fit31(((long long)a.Cout * a.y_cs + a.Lout) * 4) ||
        (a.res && !offsets_fit31(((long long)a.Cout * a.r_cs + a.Lout) * 4)))
        return VFX_ENOTSUP;
    if (!offsets_fit31(6ll * (a.CinPad >> 3) * a.Cout * 32)) return VFX_ENOTSUP;   // (the transformed weights)
    const long long nquads = ((long long)a.Lin + 4 * d - 1) / (4 * d) * d;
    const int BQ = wide ? 32 : 64;
    const int ntiles = (int)((nquads + BQ - 1) / BQ);
    const int gy = a.Cout / (wide ? 128 : 64);
    if ((long long)ntiles * gy * a.B < 512) return VFX_ENOTSUP;
    a.wd = wg4;
    a.wg_d = d;
    a.x_guard = 0;
    a.tab = nullptr;
    a.stagger = 0; a.stagger_wgs = 0;
    if (VFX_DEV_ENV("VFX_WG4_STAGGER")) {         // development: start stagger of the first residency round (see the kernel)
        a.stagger = atoi(VFX_DEV_ENV("VFX_WG4_STAGGER"));
        a.stagger_wgs = 256 * 3;
    }
    if (!a.res) { a.r_bs = a.x_bs; a.r_cs = a.x_cs; }   // (the kernel builds a residual descriptor unconditionally)
    size_t lds = 2ull * 6 * 16 * BQ * sizeof(float);
    if (VFX_DEV_ENV("VFX_WG4_LDS_PAD_KB"))        // development: fewer workgroups per CU (e.g. 90 -> one)
        lds += (size_t)atoi(VFX_DEV_ENV("VFX_WG4_LDS_PAD_KB")) * 1024;
    dim3 grid(convw_grid_x(a, ntiles), gy, a.B);
    convwg_fold_blocks(a, grid, gy);
    set_last_tile(wide ? 128 : 64, 4 * BQ, TILE_WG4);
    // dilation 1 (the residual-carrying second convolution of a ResStack layer): quads as aligned 16-byte vectors
    static const bool d1_off = VFX_DEV_ENV("VFX_WINO4_D1") && atoi(VFX_DEV_ENV("VFX_WINO4_D1")) == 0;   // development
    const bool vec_ok = ((a.x_cs | a.x_bs | a.y_cs | a.y_bs) & 3) == 0 && vfx_aligned16(a.x) && vfx_aligned16(a.y) &&
                        (!a.res || (((a.r_cs | a.r_bs) & 3) == 0 && vfx_aligned16(a.res)));
    const bool d1vec = d == 1 && vec_ok && !d1_off;
    static const int wg4x = VFX_DEV_ENV("VFX_WG4X") ? atoi(VFX_DEV_ENV("VFX_WG4X")) : VFX_WG4X_DEFAULT;   // development: A/B of the re-blocked tile
    // (2: only where the A/B shows a gain -- dilation-1 launches and the C = 128 stage; the dilated first convolutions of the C >= 256 stages measure equal)
    if (wide && wg4x && (wg4x != 2 || d1vec || a.Cout == 128)) {
        const int rc = try_launch_convwg4x(a, nquads, d1vec, stream);
        if (rc != VFX_ENOTSUP) {
            if (rc == VFX_OK) set_last_tile(128, 256, TILE_WG4X);
            return rc;
        }
    }
    {
        // the two launches of a ResStack layer, when long enough: persistent workgroups, pipeline across tiles (vfx_convwg4p.inc)
        const int rc = try_launch_convwg4p(a, ntiles, gy, wide, d1vec, stream);
        if (rc != VFX_ENOTSUP) {
            if (rc == VFX_OK) set_last_tile(wide ? 128 : 64, 4 * BQ, TILE_WG4P);
            return rc;
        }
    }
    if (d1vec)
        return wide ? launch_wg4_one<4, 1, true>(a, grid, lds, stream) : launch_wg4_one<2, 2, true>(a, grid, lds, stream);
    return wide ? launch_wg4_one<4, 1>(a, grid, lds, stream) : launch_wg4_one<2, 2>(a, grid, lds, stream);
}
