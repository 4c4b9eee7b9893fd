// vfx_convw.inc -- included by vfx_conv.hip (after the tap-table helpers, before launch_conv).
//
// convw_kernel: second-generation fp32 tap-GEMM for the 1-D convolutions of the vocoder, and its FUSED form for
// one whole ResStack layer  x <- x + conv_d1(lrelu(conv_d(lrelu(x))))  (voicefixer/vocoder/model/modules.py:592-609)
// with the intermediate tile in LDS instead of HBM.
//
// What changed against conv_taps_kernel (same MFMA, v_mfma_f32_32x32x2_f32, same tap tables / output maps / epilogue):
//  * WEIGHTS NEVER TOUCH LDS.  They are pre-packed as [slab][Cin/8][Cout][8] with the 8 channels of a group stored
//    in the order (0,2,4,6,1,3,5,7) (packing.pack_direct): lane (m = lane&31, hi = lane>>5) reads ONE 16-byte vector =
//    its A operand of four consecutive MFMA k-steps (k = 2*kk + hi), straight from L2 into VGPRs, 32 rows x 32 B = 1 KB
//    contiguous per wave-instruction, prefetched two (8-channel, tap) steps ahead.  In the first kernel the weight tile
//    was 4 of the 5 staging slots of a chunk (and of its LDS writes and barriers).
//  * LDS holds ONLY activations, so a K-chunk is 16-32 channels deep instead of 8: one barrier per 96-192 MFMAs per
//    wave instead of one per 48; between barriers every wave runs on its own (B fragments: ds_read_b32, prefetched
//    one k-step ahead, A fragments: registers).
//  * FUSED: conv-1 accumulators (tile of BL columns starting one position left of the output tile) -> bias, lrelu,
//    zero outside [0, L) -> LDS tile Y[C][BL+] (aliases the staging buffers) -> conv-2 runs barrier-free with its B
//    fragments read from Y at column shifts 0,1,2 and its A fragments from L2; accumulators start at bias2 + x (the
//    residual, loaded while Y is written).  A tile yields BL-2 outputs.  Per layer this removes one write and one
//    read of the (B, C, L) intermediate and one prologue/epilogue pair per tile.
// Interior tiles only (the caller's guard bands make every tile interior); anything else stays on conv_taps_kernel.

#define VFX_W_MAXNT 3
#ifndef VFX_W_MULTITILE
#define VFX_W_MULTITILE 0  // development: 1 = a fused workgroup walks a.tpw consecutive tiles with cross-tile prefetch of the
                           // first activation chunk / weight vectors (measured on MI355X: no gain, +66 VGPRs; kept for study)
#endif

template <int RM>
struct WStream {                       // A-operand prefetch chain over the flat (8-channel group, tap) step sequence
    int voff[RM];                      // per-lane byte offset: ((m * 8) + 4 * hi) * 4
    int gstride;                       // bytes per 8-channel group: Cout * 32
    int cin8;                          // groups per slab
    int slab0, slab_step;              // weight slab of tap t = slab0 + t * slab_step (affine: conv1d t, convtr r + t*stride;
                                       // a table indexed by the runtime t would pull the whole struct into scratch memory)
    int nt;
    int t, c8, c8_last;                // position of the NEXT load (clamped at the last step: re-loads valid data)
    float4 cur[RM], nxt[RM];

    // (the buffer resource is passed in, not stored: a struct holding a __amdgpu_buffer_rsrc_t is not scalar-replaced
    // by the compiler and would live in scratch memory)
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rsrc, float4 (&dst)[RM]) {
        const int soff = ((slab0 + t * slab_step) * cin8 + c8) * gstride;
#pragma unroll
        for (int i = 0; i < RM; ++i) {
            const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff[i], soff, 0);
            dst[i] = make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
        }
        // advance; past the end stay on the last (group, tap): the extra loads are never used
        int tn = t + 1, cn = c8;
        if (tn == nt) { tn = 0; cn = c8 + 1; }
        if (cn > c8_last) { tn = t; cn = c8; }
        t = tn;
        c8 = cn;
    }
    __device__ __forceinline__ void start(__amdgpu_buffer_rsrc_t rsrc, int m_lane, int hi, int Cout, int cin8_,
                                          int slab0_, int slab_step_, int nt_) {
#pragma unroll
        for (int i = 0; i < RM; ++i) voff[i] = ((m_lane + i * 32) * 8 + 4 * hi) * 4;
        gstride = Cout * 32;
        cin8 = cin8_;
        nt = nt_;
        slab0 = slab0_;
        slab_step = slab_step_;
        t = 0;
        c8 = 0;
        c8_last = cin8_ - 1;
        load(rsrc, cur);
        load(rsrc, nxt);
    }
};

// nsteps (8-channel group, tap) steps over an activation image in LDS: rowp = &img[hi][column of this lane],
// pitch = floats per channel row, tapoff[t] = column (float) offset of tap t.  bf0 must hold the B fragments of
// the first k-step on entry; on exit it holds garbage.
template <int RM, int RL, int NT>
__device__ __forceinline__ void mma_steps(f32x16 (&acc)[RM][RL], WStream<RM>& ws, __amdgpu_buffer_rsrc_t wrsrc,
                                          const float* rowp, int pitch, int tap0, int tapstep, int nsteps) {
    // column offset of tap t = tap0 + t * tapstep (halo tiles: t*dilation; one segment per tap: t*kcx*pitch; ...)
    float bf[2][RL];
    {
        const float* xt = rowp + tap0;
#pragma unroll
        for (int j = 0; j < RL; ++j) bf[0][j] = xt[j * 32];
    }
    const int p2 = 2 * pitch;
    int t = 0, goff = 0;
#pragma unroll 1
    for (int u = 0; u < nsteps; ++u) {
        float4 a[RM];
#pragma unroll
        for (int i = 0; i < RM; ++i) { a[i] = ws.cur[i]; ws.cur[i] = ws.nxt[i]; }
        ws.load(wrsrc, ws.nxt);
        int tn = t + 1, gn = goff;
        if (tn == NT) { tn = 0; gn = goff + 8 * pitch; }
        const int to = tap0 + t * tapstep;
        const int tno = tap0 + tn * tapstep;
        const float* xt = rowp + (goff + to);
        // first fragments of the NEXT step (the last step re-reads its own: no branch around the LDS reads)
        const float* xn = (u + 1 < nsteps) ? rowp + (gn + tno) : xt;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            if (kk < 3) {
#pragma unroll
                for (int j = 0; j < RL; ++j) bf[(kk + 1) & 1][j] = xt[(kk + 1) * p2 + j * 32];
            } else {
#pragma unroll
                for (int j = 0; j < RL; ++j) bf[0][j] = xn[j * 32];
            }
            __builtin_amdgcn_sched_barrier(0);  // keep the next k-step's LDS reads ahead of these MFMAs
#pragma unroll
            for (int i = 0; i < RM; ++i) {
                const float av = kk == 0 ? a[i].x : (kk == 1 ? a[i].y : (kk == 2 ? a[i].z : a[i].w));
#pragma unroll
                for (int j = 0; j < RL; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[kk & 1][j], acc[i][j], 0, 0, 0);
            }
        }
        t = tn;
        goff = gn;
    }
}

// The same for three taps with the step loop unrolled over the taps of one 8-channel group and THREE A-operand
// register sets (ring indexed by the tap): the vectors of step w+2 are loaded while step w multiplies, into the set
// step w-1 just released -- no register rotation (a rotation by v_mov has to wait for the load issued one step
// earlier; measured with tools/probe/mfma_probe.hip: 133 -> 142 TFLOP/s for the whole loop at 3 workgroups per CU).
template <int RM, int NTT = 3>
struct WStream3 {
    int voff[RM];
    int gstride, cin8, slab0, slab_step;
    int t, c8, c8_last;                // position of the NEXT load (clamped at the last step)
    float4 a[3][RM];

    template <int SET>
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rsrc) {
        const int soff = ((slab0 + t * slab_step) * cin8 + c8) * gstride;
#pragma unroll
        for (int i = 0; i < RM; ++i) {
            const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff[i], soff, 0);
            a[SET][i] = make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
        }
        int tn = t + 1, cn = c8;
        if (tn == NTT) { tn = 0; cn = c8 + 1; }
        if (cn > c8_last) { tn = t; cn = c8; }
        t = tn;
        c8 = cn;
    }
    __device__ __forceinline__ void start(__amdgpu_buffer_rsrc_t rsrc, int m_lane, int hi, int Cout, int cin8_, int slab0_,
                                          int slab_step_) {
#pragma unroll
        for (int i = 0; i < RM; ++i) voff[i] = ((m_lane + i * 32) * 8 + 4 * hi) * 4;
        gstride = Cout * 32;
        cin8 = cin8_;
        slab0 = slab0_;
        slab_step = slab_step_;
        t = 0;
        c8 = 0;
        c8_last = cin8_ - 1;
        load<0>(rsrc);   // (group 0, tap 0)
        load<1>(rsrc);   // (group 0, tap 1)
    }
};

// NR = 3: a 3x3 convolution on a pitch map -- the activation image holds three row segments (map rows -1, 0, +1,
// rowstep floats apart) and a group is 3 rows x 3 taps = 9 steps; the A ring is indexed by the tap within the row.
template <int RM, int RL, int NR = 1>
__device__ __forceinline__ void mma_groups3(f32x16 (&acc)[RM][RL], WStream3<RM, 3 * NR>& ws, __amdgpu_buffer_rsrc_t wrsrc,
                                            const float* rowp, int pitch, int tap0, int tapstep, int ngroups,
                                            int rowstep = 0) {
    float bf[2][RL];
    {
        const float* xt = rowp + tap0;
#pragma unroll
        for (int j = 0; j < RL; ++j) bf[0][j] = xt[j * 32];
    }
    const int p2 = 2 * pitch;
    // one ROLLED loop over (group, kernel row) with three unrolled tap steps in its body (the A ring repeats every three
    // steps): unrolling the rows as well made the compiler keep 36 fragment addresses live and spill
    const int nrg = ngroups * NR;
    int off = tap0, dy = 0;                       // LDS offset of (group, row): g*8*pitch + dy*rowstep + tap0
#pragma unroll 1
    for (int rg = 0; rg < nrg; ++rg) {
        int offn = off + rowstep, dyn = dy + 1;   // the (group, row) after this one
        if (dyn == NR) { dyn = 0; offn = off + 8 * pitch - (NR - 1) * rowstep; }
        const bool last = rg + 1 == nrg;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            // A vectors of the step after next, into the set the previous step used
            if (t == 0) ws.template load<2>(wrsrc);
            else if (t == 1) ws.template load<0>(wrsrc);
            else ws.template load<1>(wrsrc);
            const float* xt = rowp + (off + t * tapstep);
            // first fragments of the next step (the last step of the image re-reads its own: no branch around LDS reads)
            const float* xn = t < 2 ? rowp + (off + (t + 1) * tapstep) : (last ? xt : rowp + offn);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                if (kk < 3) {
#pragma unroll
                    for (int j = 0; j < RL; ++j) bf[(kk + 1) & 1][j] = xt[(kk + 1) * p2 + j * 32];
                } else {
#pragma unroll
                    for (int j = 0; j < RL; ++j) bf[0][j] = xn[j * 32];
                }
                __builtin_amdgcn_sched_barrier(0);  // keep the next k-step's LDS reads ahead of these MFMAs
#pragma unroll
                for (int i = 0; i < RM; ++i) {
                    const float4 av4 = ws.a[t][i];
                    const float av = kk == 0 ? av4.x : (kk == 1 ? av4.y : (kk == 2 ? av4.z : av4.w));
#pragma unroll
                    for (int j = 0; j < RL; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[kk & 1][j], acc[i][j], 0, 0, 0);
                }
            }
        }
        off = offn;
        dy = dyn;
    }
}

// ---- lean prologue / epilogue for plain output maps (out = q, unit position stride): one SALU add + one buffer
// instruction per accumulator register.  The generic conv_epilogue spends ~35 instructions per store on index maps,
// bounds and 64-bit addressing; with every workgroup of a launch reaching its epilogue at about the same time (equal
// work, simultaneous start) those instructions are matrix-pipe idle time.  Rows: register r of accumulator tile i
// holds row  m0 + wm*WMT + i*32 + (r&3) + 8*(r>>2) + 4*hi; the lane-dependent part (4*hi rows, column q) sits in the
// vector offset, the rest in the scalar offset.  Columns >= qend get an out-of-range VECTOR offset (the range check
// of a raw buffer compares the vector offset alone with num_records = 2^31-1; the scalar offset is added after the
// check): the buffer unit drops such stores and returns 0 for such loads.
#define VFX_W_OOB ((int)0x80000000)

template <int RM, int RL>
__device__ __forceinline__ void acc_add_rows(f32x16 (&acc)[RM][RL], __amdgpu_buffer_rsrc_t rsrc, int row0, int cs4,
                                             const int (&voff)[RL]) {
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int soff = (row0 + i * 32 + (r & 3) + 8 * (r >> 2)) * cs4;
#pragma unroll
            for (int j = 0; j < RL; ++j)
                acc[i][j][r] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, voff[j], soff, 0));
        }
}

// SUM_FIRST (the unfused launches): the accumulators hold the bare sum of products; the bias (row `nbase` + ... of this lane)
// and, with `add_res`, the residual are added here, in the order torch adds them -- an accumulator that starts at bias
// (+ residual) rounds every partial sum of the K loop at their magnitude (see conv_epilogue).  The residual of an element is
// loaded by the lane that stores it, before the store: in-place updates stay safe.
template <int RM, int RL, bool SUM_FIRST = false>
__device__ __forceinline__ void acc_store_rows(const ConvArgs& a, f32x16 (&acc)[RM][RL], __amdgpu_buffer_rsrc_t rsrc,
                                               int row0, int cs4, const int (&voff)[RL], const bool (&keep)[RL], int nbase,
                                               bool add_res, __amdgpu_buffer_rsrc_t rrsrc, int rcs4, const int (&rvoff)[RL]) {
    // keep[j]: false for a structural-zero (pad) column of a pitch map, which is written as 0 whatever was accumulated
    const int post = a.post_act;
    const float ps = a.post_slope;
    if (post <= VFX_POST_LRELU) {
        const float slope = post == VFX_POST_LRELU ? ps : 1.f;
        float4 bq[RM][4];                         // the bias of this lane's 16 rows per 32-row block: four 16-byte loads
        if constexpr (SUM_FIRST) {
#pragma unroll
            for (int i = 0; i < RM; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    bq[i][g] = a.bias ? *reinterpret_cast<const float4*>(a.bias + nbase + i * 32 + 8 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int soff = (row0 + i * 32 + (r & 3) + 8 * (r >> 2)) * cs4;
                float bv = 0.f;
                if constexpr (SUM_FIRST) {
                    const float4 q4 = bq[i][r >> 2];
                    bv = (r & 3) == 0 ? q4.x : ((r & 3) == 1 ? q4.y : ((r & 3) == 2 ? q4.z : q4.w));
                }
#pragma unroll
                for (int j = 0; j < RL; ++j) {
                    float v = acc[i][j][r];
                    if constexpr (SUM_FIRST) {
                        v += bv;
                        if (add_res)
                            v += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                                rrsrc, rvoff[j], (row0 + i * 32 + (r & 3) + 8 * (r >> 2)) * rcs4, 0));
                    }
                    v = keep[j] ? (v > 0.f ? v : v * slope) : 0.f;
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsrc, voff[j], soff, 0);
                }
            }
    } else {
        // transcendental activations (one layer per stage): rolled over the registers to keep the code small
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
            for (int j = 0; j < RL; ++j)
#pragma unroll 1
                for (int r = 0; r < 16; ++r) {
                    const int soff = (row0 + i * 32 + (r & 3) + 8 * (r >> 2)) * cs4;
                    float v = acc[i][j][r];
                    if constexpr (SUM_FIRST) {
                        if (a.bias) v += a.bias[nbase + i * 32 + (r & 3) + 8 * (r >> 2)];
                        if (add_res)
                            v += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                                rrsrc, rvoff[j], (row0 + i * 32 + (r & 3) + 8 * (r >> 2)) * rcs4, 0));
                    }
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(keep[j] ? vfx_post(v, post, ps) : 0.f), rsrc, voff[j], soff, 0);
                }
    }
}

// FUSED: 0 = one convolution; 1 = one ResStack layer, both convolutions as direct tap-GEMMs; 2 = the same with the
// second (dilation 1) convolution as Winograd F(2,3) on the LDS tile (see vfx_convwg.inc for the algebra); 3 = the same with
// F(4,3) for the second convolution (C = 64: 64 channels x 63 output quads per tile)
template <int BM, int BL, int WGM, int WGL, int NT, int NXV, int FUSED, bool TWO_LEVEL = false>
__global__ __launch_bounds__(256, FUSED ? 2 : 3) void convw_kernel(const ConvArgs a) {
    constexpr int WMT = BM / WGM, WLT = BL / WGL, RM = WMT / 32, RL = WLT / 32;
    constexpr int NTHR = 256;
    constexpr int HALO = FUSED ? 1 : 0;           // accumulator column 0 of the (first) convolution sits HALO left of q0
    constexpr int NR = NT == 9 ? 3 : 1;           // NT == 9: 3x3 convolution on a pitch map = three kernel rows of three taps
    constexpr bool MAP2D = NT == 9;               // (eval-BatchNorm pre-activation, pad-column masks)
    static_assert(!TWO_LEVEL || MAP2D, "the second accumulator set is the 3x3 instances'");
    static_assert(WGM * WGL == 4 && RM >= 1 && RL >= 1 && (NT == 2 || NT == 3 || NT == 9) && !(FUSED && MAP2D), "tile");
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    // wave index as a SCALAR: everything derived from it (row0, scalar buffer offsets) must be provably wave-uniform,
    // otherwise the compiler wraps each buffer instruction in a waterfall loop with a full wait
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lo = lane & 31, hi = lane >> 5;
    const int wm = wave / WGL, wl = wave % WGL;
    // A workgroup owns the consecutive tiles [tile0, tile1) of one (batch item, phase x m-block): exactly one for the
    // unfused launches, a.tpw for the fused layer (whose tiles are short: 2 x 24..48 steps), where the first
    // activation chunk and the first weight vectors of tile k+1 are fetched while tile k is still multiplying.
    constexpr bool MULTI = FUSED && VFX_W_MULTITILE;
    // XCD-aware tile order: the dispatcher deals consecutive workgroup ids round-robin to the 8 XCDs (id % 8), each
    // with its own L2.  Tile = (id % 8) * xcd_chunk + id / 8 gives every XCD a CONTIGUOUS range of tiles, walked in
    // order: the halo columns of neighbouring tiles and the three tap segments of a widely dilated layer (tiles
    // t, t +- d/BL) are then fetched by workgroups of the same XCD within a few dispatches of each other, i.e. from
    // its L2 instead of three times across the fabric.  Purely a placement choice: any mapping computes the same tiles.
    // Transposed convolutions (nph_fold = number of phases > 1): the phases of one tile write INTERLEAVED columns of the
    // same output lines (out = q*stride + phase).  With the phase in blockIdx.y they ran a whole row of tiles apart and
    // every line went to HBM as `stride` partial writes (WRITE_SIZE 4x the algorithmic bytes).  Folded into the id
    // -- id = (tile-in-chunk * nph + phase) * 8 + xcd -- the phases of a tile are dispatched back to back to the SAME XCD,
    // reach their epilogues together, and the partial writes of a line merge in that XCD's L2.
    int bx = blockIdx.x;
    int ph_fold = 0;
    if (a.xcd_chunk > 0) {
        int k = bx >> 3;
        if (a.nph_fold > 1) {
            const int t = k / a.nph_fold;
            ph_fold = k - t * a.nph_fold;
            k = t;
        }
        bx = (bx & 7) * a.xcd_chunk + k;
        if (bx >= a.ntiles_l) return;             // grid.x was rounded up to 8 * xcd_chunk (* nph_fold)
    }
    const int tile0 = MULTI ? bx * a.tpw : bx;
    const int tile1 = MULTI ? min(a.ntiles_l, tile0 + a.tpw) : tile0 + 1;
    const int m0g = blockIdx.y * BM;
    const int ph = FUSED ? 0 : (a.nph_fold > 1 ? ph_fold : m0g / a.Cout);
    const int m0 = a.nph_fold > 1 ? m0g : m0g - ph * a.Cout;
    const int b = blockIdx.z;
    // ragged batches: valid length of this batch item (positions past it are zero padding of the activated input)
    const int Lin_row = a.x_rows ? __builtin_amdgcn_readfirstlane(a.x_rows[b]) : a.Lin;
    const int Lq_row = a.x_rows ? Lin_row + a.lq_extra : a.Lq;
    if (tile0 * a.bl_step >= Lq_row) return;      // nothing to compute for this row in this tile (and the following)
    if (a.stagger) {
        // development / tuning: workgroups that share a CU start a third of a tile apart
        const int lin = bx + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        if (lin < a.stagger_wgs) {
            const int n = (lin % 3) * a.stagger;
            for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(127);
        }
    }
    // Geometry straight from the kernel arguments (SGPRs), no device table on this path: tap t reads LDS column
    // tap0 + t*tapstep and weight slab slab0 + t*slabstep, segment s starts at seg0 + s*segstep; slab0 and the output
    // offset are affine in the phase (transposed convolutions).  The host checks all of that (convw_setup).
    const int tap0 = a.w_tap0, tapstep = a.w_tapstep;
    const int slab0 = a.w_slab0 + ph * a.w_slab_ph, slabstep = a.w_slabstep;
    const int nseg = a.w_nseg;
    const int ooff = a.w_ooff0 + ph * a.w_ooff_ph;
    const int segw = a.segw, sv = segw >> 2, kcx = a.kcx;
    const int xtotal = nseg * kcx * sv;           // float4 per activation chunk
    const int bufstride = a.xs_floats;
    const int xcs = (int)a.x_cs;

    // ---- per-thread activation staging slots: tile-independent parts (slots past the end are clamped duplicates)
    int x_off[NXV], x_lrel[NXV], x_kc[MAP2D ? NXV : 1];
    float4 xv[NXV];
    const float inv_sv = 1.0f / (float)sv, inv_row = 1.0f / (float)(kcx * sv);
#pragma unroll
    for (int j = 0; j < NXV; ++j) {
        int i = tid + NTHR * j;
        i = i < xtotal ? i : xtotal - 1;
        const int s = fast_div(i, kcx * sv, inv_row);
        const int rem = i - s * (kcx * sv);
        const int kc = fast_div(rem, sv, inv_sv);
        const int v = rem - kc * sv;
        x_lrel[j] = a.w_seg0 + s * a.w_segstep - HALO + 4 * v;   // position of element 0 of the vector relative to q0
        if constexpr (MAP2D) x_kc[j] = kc;
        x_off[j] = (kc * xcs + x_lrel[j] + a.x_guard) * 4;       // >= 0: the buffer base is (row 0 of batch item b) - guard
    }
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.x) + ((long long)b * a.x_bs - a.x_guard), (short)0, 0x7fffffff, 0x00020000);
    const int seg_first = a.w_seg0 - HALO + (a.w_segstep < 0 ? (nseg - 1) * a.w_segstep : 0);   // extreme segment origins
    const int seg_last = a.w_seg0 - HALO + (a.w_segstep > 0 ? (nseg - 1) * a.w_segstep : 0);    // relative to q0
    const float slope = (a.pre_act == VFX_PRE_LRELU || a.pre_act == VFX_PRE_AFFINE_LRELU) ? a.pre_slope : 1.f;

    auto x_load = [&](int q0, int chunk) {
        const int xso = (q0 + chunk * kcx * xcs) * 4;
#pragma unroll
        for (int j = 0; j < NXV; ++j) {
            const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, x_off[j], xso, 0);
            xv[j] = make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
        }
    };
    // per-channel (scale, shift) of the fused eval-BatchNorm pre-activation of the 2-D convolutions: one LDS copy
    float* aff = smem + 2 * bufstride;
    if constexpr (MAP2D) {
        if (a.pre_act == VFX_PRE_AFFINE_LRELU) {
            for (int c = tid; c < a.Cin; c += NTHR) {
                aff[2 * c] = a.pre_scale[c];
                aff[2 * c + 1] = a.pre_shift[c];
            }
            __syncthreads();
        }
    }
    auto x_write = [&](float* dst, int q0, bool range_mask, int chunk) {
#pragma unroll
        for (int j = 0; j < NXV; ++j) {
            float e[4] = {xv[j].x, xv[j].y, xv[j].z, xv[j].w};
            const int p = q0 + x_lrel[j];
            if constexpr (MAP2D) {
                if (a.pre_act == VFX_PRE_AFFINE_LRELU) {
                    const int c = chunk * kcx + x_kc[j];
                    const float sc = aff[2 * c], sh = aff[2 * c + 1];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float v = fmaf(e[k], sc, sh);
                        e[k] = v > 0.f ? v : v * slope;
                    }
                }
                // zero padding and the structural-zero pad column apply to the ACTIVATED input
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (p + k < 0 || p + k >= Lin_row || (((p + k) & a.in_mask) == a.in_mask)) e[k] = 0.f;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) e[k] = fmaxf(e[k], e[k] * slope);   // (0 <= slope <= 1: convw_setup)
                if (range_mask) {  // whatever was read outside [0, Lin) is zero padding (of the ACTIVATED input; lrelu(0) = 0)
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (p + k < 0 || p + k >= Lin_row) e[k] = 0.f;
                }
            }
            int i = tid + NTHR * j;
            i = i < xtotal ? i : xtotal - 1;
            *reinterpret_cast<float4*>(dst + 4 * i) = make_float4(e[0], e[1], e[2], e[3]);
        }
    };

    const int row0 = m0 + wm * WMT;               // first accumulator row of this wave (lane part: + 4*hi)
    const int nbase = row0 + 4 * hi;              // accumulator row of register 0 of this lane
    const int m_lane = row0 + lo;                 // weight row of this lane's A operand
    const int b_col = wl * WLT + lo;
    // plain output map (out = q, unit stride): lean residual pre-load and store path
    const bool plain_out = a.q_shift == 31 && a.o_rs == 0 && a.o_cs == 1 && ooff == 0 && a.y_ls == 1 && a.Lq <= a.Lout;
    // affine output maps without residual (transposed 1-D convolutions: out = q*stride + phase offset) take the same lean
    // store path, with the output position instead of q in the vector offset
    const bool lean_out = plain_out || (a.q_shift == 31 && a.o_rs == 0 && a.y_ls == 1 && !a.res && !MAP2D);
    const int S = a.Cin / kcx;                    // K-chunks (host guarantees Cin % kcx == 0)
    const int nsteps = (kcx >> 3) * NT;
    (void)nsteps;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wd), (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(
        a.y + (long long)b * a.y_bs, (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.res ? a.res : a.x) + (long long)b * a.r_bs, (short)0, 0x7fffffff, 0x00020000);

    using WS = typename std::conditional<NT == 2, WStream<RM>, WStream3<RM, NT == 9 ? 9 : 3>>::type;
    WS ws;
    auto ws_start = [&]() {
        if constexpr (NT != 2) ws.start(wrsrc, m_lane, hi, a.Cout, a.CinPad >> 3, slab0, slabstep);
        else ws.start(wrsrc, m_lane, hi, a.Cout, a.CinPad >> 3, slab0, slabstep, NT);
    };
    ws_start();
    x_load(tile0 * a.bl_step, 0);

#pragma unroll 1
    for (int tile = tile0; tile < tile1; ++tile) {
        // (the staging registers hold chunk 0 of this tile, the weight stream its first two steps)
        const int q0 = tile * a.bl_step;          // first OUTPUT position of this tile
        const int qend = min(Lq_row, q0 + a.bl_step);
        const bool has_next = MULTI && tile + 1 < tile1;
        const int nq0 = q0 + a.bl_step;
        const bool range_mask = (q0 + seg_first < 0) || (q0 + seg_last + segw > Lin_row);  // tile reaches past the row
        int rvoff[RL], yvoff[RL];
        bool keep[RL];
#pragma unroll
        for (int j = 0; j < RL; ++j) {
            const int q = q0 + b_col + j * 32;
            rvoff[j] = q < qend ? (4 * hi * (int)a.r_cs + q) * 4 : VFX_W_OOB;
            const int out = plain_out ? q : q * a.o_cs + ooff;
            yvoff[j] = (q < qend && out >= 0 && out < a.Lout) ? (4 * hi * (int)a.y_cs + out) * 4 : VFX_W_OOB;
            keep[j] = !(MAP2D && ((q & a.out_mask) == a.out_mask));
        }
        // unfused launches: the accumulators start at zero, bias and residual are added to the finished sum (acc_store_rows /
        // conv_epilogue); the fused layer's first half starts at its bias b1
        f32x16 acc[RM][RL];
        if constexpr (FUSED) acc_init_bias<RM, RL>(acc, a.bias, nbase);
        else acc_zero<RM, RL>(acc);
        // 3x3 on a map: K = 9 Cin products in one chain.  A strictly sequential fp32 chain of 576 ... 4608 terms is up to 1.13 x the
        // bound of tests/test_convw_gpu.py (4 x the CPU operator's blocked sum); the TWO_LEVEL instances (a.two_level) add the
        // accumulators into a second set every 32 input channels (288 terms), as conv_taps_kernel's small tiles do every 64.  The
        // set costs 32 registers on the small tiles; on the 128 x 128 tile it costs 64 and spills (the host asks for it there from
        // 256 input channels on only)
        f32x16 acc2[TWO_LEVEL ? RM : 1][TWO_LEVEL ? RL : 1];
        if constexpr (TWO_LEVEL) acc_zero<RM, RL>(acc2);

        x_write(smem, q0, range_mask, 0);
        if (S > 1) x_load(q0, 1);
        else if (has_next) x_load(nq0, 0);
        __syncthreads();
        for (int s = 0; s < S; ++s) {
            if (s + 1 < S) {
                x_write(smem + ((s + 1) & 1) * bufstride, q0, range_mask, s + 1);
                if (s + 2 < S) x_load(q0, s + 2);
                else if (has_next) x_load(nq0, 0);
            }
            const float* xs = smem + (s & 1) * bufstride;
            if constexpr (NT != 2)
                mma_groups3<RM, RL, NR>(acc, ws, wrsrc, xs + hi * segw + b_col, segw, tap0, tapstep, kcx >> 3, kcx * segw);
            else mma_steps<RM, RL, NT>(acc, ws, wrsrc, xs + hi * segw + b_col, segw, tap0, tapstep, nsteps);
            __syncthreads();
            if constexpr (TWO_LEVEL) {
                if (((s + 1) & 3) == 0 && s + 1 < S) {
#pragma unroll
                    for (int i = 0; i < RM; ++i)
#pragma unroll
                        for (int j = 0; j < RL; ++j) {
                            acc2[i][j] += acc[i][j];
#pragma unroll
                            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
                        }
                }
            }
        }
        if constexpr (TWO_LEVEL) {
#pragma unroll
            for (int i = 0; i < RM; ++i)
#pragma unroll
                for (int j = 0; j < RL; ++j) acc[i][j] += acc2[i][j];
        }

        if constexpr (!FUSED) {
            if (lean_out && !(a.res && !a.res_init))
                acc_store_rows<RM, RL, true>(a, acc, yrsrc, row0, (int)a.y_cs * 4, yvoff, keep, nbase, a.res != nullptr, rrsrc,
                                             (int)a.r_cs * 4, rvoff);
            else conv_epilogue<BM, BL, WGM, WGL>(a, acc, q0, m0, b, wm, wl, lo, hi, ooff, qend);
        } else if constexpr (FUSED == 3) {
            // ---- second convolution (k3, dilation 1) as Winograd F(4,3) on y = lrelu(conv1 + b1) kept in LDS: the output
            // quad 4Q .. 4Q+3 of the tile shares Y[4Q .. 4Q+5] (one 16-byte + one 8-byte LDS read per (channel, quad)), V = B^T d
            // is formed right before the MFMAs, six planes accumulate U_k V_k (weights packing.pack_wino4, 16-byte A vectors
            // from L2; algebra, start values and output transform as in convwg4_kernel): 6 products per 4 outputs instead
            // of 12 for this half of the layer.  The 64 channels x 256 columns of the tile are re-dealt for this phase: wave
            // = 32 channels x 32 quads (the first phase's 64 x 64 columns per wave would be 16 quads: half an MFMA tile).
            // 63 quads per tile are outputs (bl_step = 252: quad 63 would need columns 256, 257); quads are aligned
            // float4 in memory (q0 = 252 * tile), so residual and stores move as 16-byte vectors, the one quad that straddles
            // the end of a row of odd length as single elements under a workgroup-uniform branch.
            static_assert(BM == 64 && BL == 256 && WGM == 1 && WGL == 4, "F(4,3) second half: 64 channels x 64 quads");
            const int wm2 = wave & 1, wq2 = wave >> 1;
            const int row2 = m0 + 32 * wm2;
            const __amdgpu_buffer_rsrc_t w2rsrc =
                __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wd2), (short)0, 0x7fffffff, 0x00020000);
            const int a2voff = ((row2 + lo) * 8 + 4 * hi) * 4;
            const int g2s = a.Cout * 32;          // bytes per (plane, 8-channel group)
            const int p2s = (a.Cout >> 3) * g2s;  // bytes per plane
            float4 aw2[2][6];
            auto a2_load = [&](auto set_tag, int grp) {
                constexpr int SET = decltype(set_tag)::value;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(w2rsrc, a2voff, k * p2s + grp * g2s, 0);
                    aw2[SET][k] = make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
                }
            };
            const int Qi = 32 * wq2 + lo;         // quad of this lane within the tile
            const int qq = q0 + 4 * Qi;           // its first output position
            const bool full = qq + 3 < qend;
            const bool has_tail = (qend & 3) != 0;   // (uniform; q0 is a multiple of 4) the tile ends inside a quad
            const int rvq = full ? (4 * hi * (int)a.r_cs + qq) * 4 : VFX_W_OOB;
            const int yvq = full ? (4 * hi * (int)a.y_cs + qq) * 4 : VFX_W_OOB;
            int rv1[4], yv1[4];                   // single elements: the straddling quad only
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool one = !full && qq + i < qend;
                rv1[i] = one ? (4 * hi * (int)a.r_cs + qq + i) * 4 : VFX_W_OOB;
                yv1[i] = one ? (4 * hi * (int)a.y_cs + qq + i) * 4 : VFX_W_OOB;
            }
            // residual quads (x itself) and the first A vectors: in flight while y is written and the barrier waits
            u32x4 rq[16];
            {
                const int cs4 = (int)a.r_cs * 4;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    rq[r] = __builtin_amdgcn_raw_buffer_load_b128(rrsrc, rvq, (row2 + (r & 3) + 8 * (r >> 2)) * cs4, 0);
            }
            a2_load(std::integral_constant<int, 0>{}, 0);
            float* Y = smem;                      // aliases the staging buffers (every wave is past its last x read)
            const int yp = a.yp;
            const float ms = a.mid_slope;
            // (round 4: the fp32 MFMA and the VALU share their issue cycles on this chip -- profiles/r04_convwg4_prologue_ab.txt --
            // so the activation is mul + max (0 <= slope <= 1, checked on the host) and the zero-outside-the-row select is only
            // compiled into the path of the tiles that reach past a row end)
            if (q0 - HALO >= 0 && q0 - HALO + BL <= Lin_row) {   // (workgroup-uniform) every column of Y lies inside the row
#pragma unroll
                for (int j = 0; j < RL; ++j) {
                    float* yrow = Y + (wm * WMT + 4 * hi) * yp + wl * WLT + j * 32 + lo;
#pragma unroll
                    for (int i = 0; i < RM; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float v = acc[i][j][r];
                            yrow[(i * 32 + (r & 3) + 8 * (r >> 2)) * yp] = fmaxf(v, v * ms);
                        }
                }
            } else {
#pragma unroll
                for (int j = 0; j < RL; ++j) {
                    const int u = wl * WLT + j * 32 + lo;
                    const int p = q0 - HALO + u;
                    const bool ok = p >= 0 && p < Lin_row;  // conv-2's zero padding: y is zero outside the sequence
                    float* yrow = Y + (wm * WMT + 4 * hi) * yp + u;
#pragma unroll
                    for (int i = 0; i < RM; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float v = acc[i][j][r];
                            yrow[(i * 32 + (r & 3) + 8 * (r >> 2)) * yp] = ok ? fmaxf(v, v * ms) : 0.f;
                        }
                }
            }
            __syncthreads();
            // start values: planes (0, 1, 3, 5) = the solution of A^T m = residual + bias2 with m2 = m4 = 0
            f32x16 accq[6];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                accq[0][r] = __uint_as_float(rq[r].x); accq[1][r] = __uint_as_float(rq[r].y);
                accq[3][r] = __uint_as_float(rq[r].z); accq[5][r] = __uint_as_float(rq[r].w);
            }
            if (has_tail) {
                const int cs4 = (int)a.r_cs * 4;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int soff = (row2 + (r & 3) + 8 * (r >> 2)) * cs4;
                    accq[0][r] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, rv1[0], soff, 0));
                    accq[1][r] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, rv1[1], soff, 0));
                    accq[3][r] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, rv1[2], soff, 0));
                    accq[5][r] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, rv1[3], soff, 0));
                }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 bq = a.bias2 ? *reinterpret_cast<const float4*>(a.bias2 + row2 + 4 * hi + 8 * g)
                                          : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * g + e;
                    const float bb = e == 0 ? bq.x : (e == 1 ? bq.y : (e == 2 ? bq.z : bq.w));
                    const float t0 = accq[0][r] + bb, t1 = accq[1][r] + bb, t2 = accq[3][r] + bb, t3 = accq[5][r] + bb;
                    const float m3 = 0.5f * (t2 - t1);
                    const float m1 = 2.f * t1 - t2;
                    accq[0][r] = t0 - m1 - m3;
                    accq[1][r] = m1;
                    accq[2][r] = 0.f;
                    accq[3][r] = m3;
                    accq[4][r] = 0.f;
                    accq[5][r] = t3 - m1 - 8.f * m3;
                }
            }
            // K loop over the C/8 channel groups of Y, two per iteration (A register sets 0 / 1)
            const float* yb = Y + hi * yp + 4 * Qi;
            const int ngrp = a.Cout >> 3;
            auto group = [&](auto set_tag, int grp, int nxt) {
                constexpr int SET = decltype(set_tag)::value;
                const float* yg = yb + grp * 8 * yp;
                float4 dl = *reinterpret_cast<const float4*>(yg);
                float2 dh = *reinterpret_cast<const float2*>(yg + 4);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    float V[6];
                    {
                        const float s1 = fmaf(-4.f, dl.z, dh.x), s2 = fmaf(-4.f, dl.y, dl.w);
                        const float s3 = dh.x - dl.z, s4 = dl.w - dl.y;
                        V[0] = fmaf(4.f, dl.x, fmaf(-5.f, dl.z, dh.x));
                        V[1] = s1 + s2;
                        V[2] = s1 - s2;
                        V[3] = fmaf(2.f, s4, s3);
                        V[4] = fmaf(-2.f, s4, s3);
                        V[5] = fmaf(4.f, dl.y, fmaf(-5.f, dl.w, dh.y));
                    }
                    if (kk < 3) {
                        dl = *reinterpret_cast<const float4*>(yg + (kk + 1) * 2 * yp);
                        dh = *reinterpret_cast<const float2*>(yg + (kk + 1) * 2 * yp + 4);
                    }
                    if (kk == 0) {
                        if constexpr (SET == 0) a2_load(std::integral_constant<int, 1>{}, nxt);
                        else a2_load(std::integral_constant<int, 0>{}, nxt);
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int k = 0; k < 6; ++k) {
                        const float4 av4 = aw2[SET][k];
                        const float av = kk == 0 ? av4.x : (kk == 1 ? av4.y : (kk == 2 ? av4.z : av4.w));
                        accq[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, V[k], accq[k], 0, 0, 0);
                    }
                }
            };
#pragma unroll 1
            for (int grp = 0; grp < ngrp; grp += 2) {
                group(std::integral_constant<int, 0>{}, grp, grp + 1);
                group(std::integral_constant<int, 1>{}, grp + 1, min(grp + 2, ngrp - 1));
            }
            // output transform, activation, stores
            {
                const int post = a.post_act;
                const float ps = a.post_slope;
                const int cs4 = (int)a.y_cs * 4;
                auto outs = [&](int r, float (&y)[4]) {
                    const float p12 = accq[1][r] + accq[2][r], m12 = accq[1][r] - accq[2][r];
                    const float p34 = accq[3][r] + accq[4][r], m34 = accq[3][r] - accq[4][r];
                    y[0] = (accq[0][r] + p12) + p34;
                    y[1] = fmaf(2.f, m34, m12);
                    y[2] = fmaf(4.f, p34, p12);
                    y[3] = fmaf(8.f, m34, m12) + accq[5][r];
                };
                auto store4 = [&](const float (&v)[4], int soff) {
                    u32x4 u;
                    u.x = __float_as_uint(v[0]); u.y = __float_as_uint(v[1]); u.z = __float_as_uint(v[2]); u.w = __float_as_uint(v[3]);
                    __builtin_amdgcn_raw_buffer_store_b128(u, yrsrc, yvq, soff, 0);
                    if (has_tail) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[i]), yrsrc, yv1[i], soff, 0);
                    }
                };
                if (post == VFX_POST_NONE) {          // (seven of a stage's eight layers: nothing to evaluate per output)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int soff = (row2 + (r & 3) + 8 * (r >> 2)) * cs4;
                        float y[4];
                        outs(r, y);
                        store4(y, soff);
                    }
                } else if (post == VFX_POST_LRELU) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int soff = (row2 + (r & 3) + 8 * (r >> 2)) * cs4;
                        float y[4];
                        outs(r, y);
#pragma unroll
                        for (int i = 0; i < 4; ++i) y[i] = fmaxf(y[i], y[i] * ps);
                        store4(y, soff);
                    }
                } else {
                    // transcendental activations (one layer per stage): rolled over the registers to keep the code small
#pragma unroll 1
                    for (int r = 0; r < 16; ++r) {
                        const int soff = (row2 + (r & 3) + 8 * (r >> 2)) * cs4;
                        float y[4];
                        outs(r, y);
#pragma unroll
                        for (int i = 0; i < 4; ++i) y[i] = vfx_post(y[i], post, ps);
                        store4(y, soff);
                    }
                }
            }
            if (has_next) __syncthreads();
        } else if constexpr (FUSED == 2) {
            // ---- second convolution (k3, dilation 1) as Winograd F(2,3) on y = lrelu(conv1 + b1) kept in LDS: output
            // columns 2p, 2p+1 of the tile share Y[2p .. 2p+3]; V = (d0-d2, d1+d2, d2-d1, d1-d3) is formed from two 8-byte
            // LDS reads per (channel, pair) right before the MFMAs, the four planes accumulate U_k V_k (weights
            // packing.pack_wino, 16-byte A vectors from L2), y[2p] = m0+m1+m2, y[2p+1] = m1-m2-m3: 4 products per output
            // pair instead of 6 for this half of the layer.
            static_assert(RL % 2 == 0, "pairs per wave");
            constexpr int RP = RL / 2;            // 32-pair column blocks per wave
            const __amdgpu_buffer_rsrc_t w2rsrc =
                __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wd2), (short)0, 0x7fffffff, 0x00020000);
            int a2voff[RM];
#pragma unroll
            for (int i = 0; i < RM; ++i) a2voff[i] = ((m_lane + i * 32) * 8 + 4 * hi) * 4;
            const int g2s = a.Cout * 32;          // bytes per (plane, 8-channel group)
            const int p2s = (a.Cout >> 3) * g2s;  // bytes per plane
            float4 aw2[2][4][RM];
            auto a2_load = [&](auto set_tag, int grp) {
                constexpr int SET = decltype(set_tag)::value;
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int i = 0; i < RM; ++i) {
                        const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(w2rsrc, a2voff[i], k * p2s + grp * g2s, 0);
                        aw2[SET][k][i] = make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
                    }
            };
            a2_load(std::integral_constant<int, 0>{}, 0);
            // accumulator planes: 1 starts at bias2, 0 at the residual of the first output, 3 at minus the residual of
            // the second, 2 at zero
            int y0v[RP], y1v[RP], r0v[RP], r1v[RP];
#pragma unroll
            for (int jp = 0; jp < RP; ++jp) {
                const int q = q0 + 2 * (wl * (WLT / 2) + jp * 32 + lo);
                y0v[jp] = q < qend ? (4 * hi * (int)a.y_cs + q) * 4 : VFX_W_OOB;
                y1v[jp] = q + 1 < qend ? (4 * hi * (int)a.y_cs + q + 1) * 4 : VFX_W_OOB;
                r0v[jp] = q < qend ? (4 * hi * (int)a.r_cs + q) * 4 : VFX_W_OOB;
                r1v[jp] = q + 1 < qend ? (4 * hi * (int)a.r_cs + q + 1) * 4 : VFX_W_OOB;
            }
            f32x16 accw[4][RM][RP];
#pragma unroll
            for (int i = 0; i < RM; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 bq = a.bias2 ? *reinterpret_cast<const float4*>(a.bias2 + nbase + i * 32 + 8 * g)
                                              : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int jp = 0; jp < RP; ++jp) {
                        accw[1][i][jp][4 * g + 0] = bq.x; accw[1][i][jp][4 * g + 1] = bq.y;
                        accw[1][i][jp][4 * g + 2] = bq.z; accw[1][i][jp][4 * g + 3] = bq.w;
#pragma unroll
                        for (int e = 0; e < 4; ++e) accw[2][i][jp][4 * g + e] = 0.f;
                    }
                }
            {
                const int cs4 = (int)a.r_cs * 4;
#pragma unroll
                for (int i = 0; i < RM; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int soff = (row0 + i * 32 + (r & 3) + 8 * (r >> 2)) * cs4;
#pragma unroll
                        for (int jp = 0; jp < RP; ++jp) {
                            accw[0][i][jp][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, r0v[jp], soff, 0));
                            accw[3][i][jp][r] = -__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, r1v[jp], soff, 0));
                        }
                    }
            }
            float* Y = smem;                      // aliases the staging buffers (every wave is past its last x read)
            const int yp = a.yp;
            const float ms = a.mid_slope;
#pragma unroll
            for (int j = 0; j < RL; ++j) {
                const int u = wl * WLT + j * 32 + lo;
                const int p = q0 - HALO + u;
                const bool ok = p >= 0 && p < Lin_row;  // conv-2's zero padding: y is zero outside the sequence
                float* yrow = Y + (wm * WMT + 4 * hi) * yp + u;
#pragma unroll
                for (int i = 0; i < RM; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = acc[i][j][r];
                        v = v > 0.f ? v : v * ms;
                        yrow[(i * 32 + (r & 3) + 8 * (r >> 2)) * yp] = ok ? v : 0.f;
                    }
            }
            __syncthreads();
            // K loop over the C/8 channel groups of Y, two per iteration (A register sets 0 / 1)
            const float* yb = Y + hi * yp + 2 * (wl * (WLT / 2) + lo);
            const int ngrp = a.Cout >> 3;
            auto group = [&](auto set_tag, int grp, int nxt) {
                constexpr int SET = decltype(set_tag)::value;
                const float* yg = yb + grp * 8 * yp;
                float2 dlo[RP], dhi[RP];
#pragma unroll
                for (int jp = 0; jp < RP; ++jp) {
                    dlo[jp] = *reinterpret_cast<const float2*>(yg + jp * 64);
                    dhi[jp] = *reinterpret_cast<const float2*>(yg + jp * 64 + 2);
                }
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    float V[4][RP];
#pragma unroll
                    for (int jp = 0; jp < RP; ++jp) {
                        V[0][jp] = dlo[jp].x - dhi[jp].x;
                        V[1][jp] = dlo[jp].y + dhi[jp].x;
                        V[2][jp] = dhi[jp].x - dlo[jp].y;
                        V[3][jp] = dlo[jp].y - dhi[jp].y;
                    }
                    if (kk < 3) {
#pragma unroll
                        for (int jp = 0; jp < RP; ++jp) {
                            dlo[jp] = *reinterpret_cast<const float2*>(yg + (kk + 1) * 2 * yp + jp * 64);
                            dhi[jp] = *reinterpret_cast<const float2*>(yg + (kk + 1) * 2 * yp + jp * 64 + 2);
                        }
                    }
                    if (kk == 0) {
                        if constexpr (SET == 0) a2_load(std::integral_constant<int, 1>{}, nxt);
                        else a2_load(std::integral_constant<int, 0>{}, nxt);
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
#pragma unroll
                        for (int i = 0; i < RM; ++i) {
                            const float4 av4 = aw2[SET][k][i];
                            const float av = kk == 0 ? av4.x : (kk == 1 ? av4.y : (kk == 2 ? av4.z : av4.w));
#pragma unroll
                            for (int jp = 0; jp < RP; ++jp)
                                accw[k][i][jp] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, V[k][jp], accw[k][i][jp], 0, 0, 0);
                        }
                }
            };
#pragma unroll 1
            for (int grp = 0; grp < ngrp; grp += 2) {
                group(std::integral_constant<int, 0>{}, grp, grp + 1);
                group(std::integral_constant<int, 1>{}, grp + 1, min(grp + 2, ngrp - 1));
            }
            // output transform, activation, stores
            {
                const int post = a.post_act;
                const float ps = a.post_slope;
                const int cs4 = (int)a.y_cs * 4;
                if (post <= VFX_POST_LRELU) {
                    const float sl = post == VFX_POST_LRELU ? ps : 1.f;
#pragma unroll
                    for (int i = 0; i < RM; ++i)
#pragma unroll
                        for (int jp = 0; jp < RP; ++jp)
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const int soff = (row0 + i * 32 + (r & 3) + 8 * (r >> 2)) * cs4;
                                float v0 = (accw[0][i][jp][r] + accw[1][i][jp][r]) + accw[2][i][jp][r];
                                float v1 = (accw[1][i][jp][r] - accw[2][i][jp][r]) - accw[3][i][jp][r];
                                v0 = v0 > 0.f ? v0 : v0 * sl;
                                v1 = v1 > 0.f ? v1 : v1 * sl;
                                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v0), yrsrc, y0v[jp], soff, 0);
                                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v1), yrsrc, y1v[jp], soff, 0);
                            }
                } else {
                    // transcendental activations (one layer per stage): rolled over the registers to keep the code small
#pragma unroll
                    for (int i = 0; i < RM; ++i)
#pragma unroll
                        for (int jp = 0; jp < RP; ++jp)
#pragma unroll 1
                            for (int r = 0; r < 16; ++r) {
                                const int soff = (row0 + i * 32 + (r & 3) + 8 * (r >> 2)) * cs4;
                                const float v0 = (accw[0][i][jp][r] + accw[1][i][jp][r]) + accw[2][i][jp][r];
                                const float v1 = (accw[1][i][jp][r] - accw[2][i][jp][r]) - accw[3][i][jp][r];
                                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vfx_post(v0, post, ps)), yrsrc, y0v[jp], soff, 0);
                                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vfx_post(v1, post, ps)), yrsrc, y1v[jp], soff, 0);
                            }
                }
            }
            if (has_next) __syncthreads();
        } else {
            // ---- second convolution of the ResStack layer: k3, dilation 1, on y = lrelu(conv1 + b1) kept in LDS
            WStream3<RM> w2;
            const __amdgpu_buffer_rsrc_t w2rsrc =
                __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wd2), (short)0, 0x7fffffff, 0x00020000);
            w2.start(w2rsrc, m_lane, hi, a.Cout, a.Cout >> 3, 0, 1);
            // conv-2 accumulators start at bias2 + x (the residual): the loads fly while y is written and the barrier waits
            f32x16 acc2[RM][RL];
            acc_init_bias<RM, RL>(acc2, a.bias2, nbase);
            acc_add_rows<RM, RL>(acc2, rrsrc, row0, (int)a.r_cs * 4, rvoff);
            float* Y = smem;                      // aliases the staging buffers (every wave is past its last x read)
            const int yp = a.yp;
            const float ms = a.mid_slope;
#pragma unroll
            for (int j = 0; j < RL; ++j) {
                const int u = wl * WLT + j * 32 + lo;
                const int p = q0 - HALO + u;
                const bool ok = p >= 0 && p < Lin_row;  // conv-2's zero padding: y is zero outside the sequence
                float* yrow = Y + (wm * WMT + 4 * hi) * yp + u;
#pragma unroll
                for (int i = 0; i < RM; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = acc[i][j][r];
                        v = v > 0.f ? v : v * ms;
                        yrow[(i * 32 + (r & 3) + 8 * (r >> 2)) * yp] = ok ? v : 0.f;
                    }
            }
            __syncthreads();
            mma_groups3<RM, RL>(acc2, w2, w2rsrc, Y + hi * yp + b_col, yp, 0, 1, a.Cout >> 3);
            if (has_next) ws_start();             // conv-1 weight vectors of the next tile: in flight during the stores
            acc_store_rows<RM, RL>(a, acc2, yrsrc, row0, (int)a.y_cs * 4, yvoff, keep, nbase, false, rrsrc, 0, rvoff);
            if (has_next) __syncthreads();        // Y is dead before the next tile's chunk 0 overwrites it
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------
template <int BM, int BL, int WGM, int WGL, int NT, int NXV, int FUSED, bool TWO_LEVEL = false>
static int launch_w_one(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t s) {
    return vfx_launch<convw_kernel<BM, BL, WGM, WGL, NT, NXV, FUSED, TWO_LEVEL>>(grid, dim3(256), lds, s, a);
}

template <int BM, int BL, int WGM, int WGL, int NT, int FUSED, bool TWO_LEVEL = false>
static int launch_w_nxv(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t s) {
    if constexpr (FUSED) {
        return a.nxv <= 5 ? launch_w_one<BM, BL, WGM, WGL, NT, 5, FUSED>(a, grid, lds, s)
                          : launch_w_one<BM, BL, WGM, WGL, NT, 6, FUSED>(a, grid, lds, s);
    } else if constexpr (NT == 9) {
        return a.nxv <= 4 ? launch_w_one<BM, BL, WGM, WGL, NT, 4, false, TWO_LEVEL>(a, grid, lds, s)
                          : launch_w_one<BM, BL, WGM, WGL, NT, 7, false, TWO_LEVEL>(a, grid, lds, s);
    } else {
        return a.nxv <= 4   ? launch_w_one<BM, BL, WGM, WGL, NT, 4, false>(a, grid, lds, s)
               : a.nxv == 5 ? launch_w_one<BM, BL, WGM, WGL, NT, 5, false>(a, grid, lds, s)
                            : launch_w_one<BM, BL, WGM, WGL, NT, 6, false>(a, grid, lds, s);
    }
}

#define VFX_W_MAXNXV 6
#define VFX_W_LDS_BUDGET (52 * 1024)  // activation double buffer per workgroup: keeps three workgroups per CU

// Shared geometry set-up of the convw launches: tables, chunk depth, interior check.  ``halo_extra`` = positions the
// accumulator tile starts left of the output tile (1 for the fused layer), ``bl_out`` = outputs per tile.
// Returns VFX_ENOTSUP when the launch has to stay on conv_taps_kernel.
static int convw_setup(ConvArgs& a, const vfx_tensor* x, int nphase, const PhaseSpec* phs, int BL, int halo_extra,
                       int bl_out_fixed, size_t lds_floor, size_t* lds_out, int* ntiles_out) {
    const int Cin = a.Cin, Lin = a.Lin, Lq = a.Lq;
    if (Cin % 8 != 0 || x->guard <= 0) return VFX_ENOTSUP;
    // the kernel evaluates leaky ReLU as max(v, slope * v): other slopes stay on the first-generation kernel
    if ((a.pre_act == VFX_PRE_LRELU || a.pre_act == VFX_PRE_AFFINE_LRELU) && !(a.pre_slope >= 0.f && a.pre_slope <= 1.f))
        return VFX_ENOTSUP;
    const int nt = phs[0].ntaps;
    for (int p = 1; p < nphase; ++p)
        if (phs[p].ntaps != nt) return VFX_ENOTSUP;
    bool all_segments;
    const int maxspan = max_tap_span(nphase, phs, BL, &all_segments);
    // unaligned ("exact") origins everywhere: every tile is interior and staged with buffer loads.  Small spans of
    // an unfused launch stage exactly BL columns and produce BL - span outputs; wide dilations stage BL columns per tap.
    const bool shrink = bl_out_fixed == 0 && maxspan > 0 && maxspan <= 8;
    const bool exact_layout = shrink || all_segments;
    ConvTables tb;
    int kcx = 32;
    for (;; kcx >>= 1) {
        if (kcx < 8) return VFX_ENOTSUP;
        if (Cin % kcx != 0) continue;
        std::memset(&tb, 0, sizeof(tb));
        fill_segments(a, tb, nphase, phs, BL, kcx, exact_layout);
        if (!exact_layout) {
            // fill_segments aligned the origins down to a multiple of 4; buffer loads need no alignment: re-base every phase on
            // its exact tap offsets, so that the staged width is BL + span rounded up to 4 (per-tap segments: BL rounded up)
            a.segw = (BL + maxspan + 3) & ~3;
            for (int p = 0; p < nphase; ++p)
                if (tb.ph[p].nseg != 1) a.segw = a.segw > ((BL + 3) & ~3) ? a.segw : ((BL + 3) & ~3);
            for (int p = 0; p < nphase; ++p) fill_phase(tb.ph[p], phs[p], tb.ph[p].nseg == 1, true, kcx * a.segw);
        }
        const int maxseg = max_segments(tb, nphase);
        a.xs_floats = maxseg * kcx * a.segw;
        a.nxv = (int)(((long long)maxseg * kcx * (a.segw / 4) + 255) / 256);
        if (a.nxv <= VFX_W_MAXNXV && 2ull * a.xs_floats * sizeof(float) <= VFX_W_LDS_BUDGET) break;
    }
    a.kcx = kcx;
    a.bl_step = bl_out_fixed ? bl_out_fixed : (shrink ? BL - maxspan : BL);
    const int ntiles = (Lq + a.bl_step - 1) / a.bl_step;
    // interior check: every staged vector inside [-guard, Lin + guard)
    const TapSpan seg = segment_range(tb, nphase);
    const long long g = x->guard;
    if (-(long long)seg.mn + halo_extra > g) return VFX_ENOTSUP;
    if ((long long)(ntiles - 1) * a.bl_step - halo_extra + seg.mx + a.segw > (long long)Lin + g) return VFX_ENOTSUP;
    // the kernel takes the staging layout from phase 0: every phase must stage the same segments / tap columns
    for (int p = 1; p < nphase; ++p) {
        if (tb.ph[p].nseg != tb.ph[0].nseg) return VFX_ENOTSUP;
        for (int sg = 0; sg < tb.ph[0].nseg; ++sg)
            if (tb.ph[p].seg_org[sg] != tb.ph[0].seg_org[sg]) return VFX_ENOTSUP;
        for (int t = 0; t < nt; ++t)
            if (tb.ph[p].tap_lds[t] != tb.ph[0].tap_lds[t]) return VFX_ENOTSUP;
    }
    // the kernel evaluates tap t as (tap_lds[0] + t*step, tap_w[0] + t*step): both must be affine in t
    for (int p = 0; p < nphase; ++p)
        for (int t = 2; t < nt; ++t) {
            const PhaseTab& T = tb.ph[p];
            if (T.tap_lds[t] - T.tap_lds[0] != t * (T.tap_lds[1] - T.tap_lds[0])) return VFX_ENOTSUP;
            if (T.tap_w[t] - T.tap_w[0] != t * (T.tap_w[1] - T.tap_w[0])) return VFX_ENOTSUP;
        }
    {
        const PhaseTab& T0 = tb.ph[0];
        for (int sg = 2; sg < T0.nseg; ++sg)
            if (T0.seg_org[sg] - T0.seg_org[0] != sg * (T0.seg_org[1] - T0.seg_org[0])) return VFX_ENOTSUP;
        for (int p = 2; p < nphase; ++p) {
            if (tb.ph[p].tap_w[0] - T0.tap_w[0] != p * (tb.ph[1].tap_w[0] - T0.tap_w[0])) return VFX_ENOTSUP;
            if (tb.ph[p].ooff - T0.ooff != p * (tb.ph[1].ooff - T0.ooff)) return VFX_ENOTSUP;
        }
        for (int p = 1; p < nphase; ++p)
            if (nt > 1 && tb.ph[p].tap_w[1] - tb.ph[p].tap_w[0] != T0.tap_w[1] - T0.tap_w[0]) return VFX_ENOTSUP;
        a.w_tap0 = T0.tap_lds[0];
        a.w_tapstep = nt > 1 ? T0.tap_lds[1] - T0.tap_lds[0] : 0;
        a.w_slab0 = T0.tap_w[0];
        a.w_slabstep = nt > 1 ? T0.tap_w[1] - T0.tap_w[0] : 0;
        a.w_slab_ph = nphase > 1 ? tb.ph[1].tap_w[0] - T0.tap_w[0] : 0;
        a.w_ooff0 = T0.ooff;
        a.w_ooff_ph = nphase > 1 ? tb.ph[1].ooff - T0.ooff : 0;
        a.w_nseg = T0.nseg;
        a.w_seg0 = T0.seg_org[0];
        a.w_segstep = T0.nseg > 1 ? T0.seg_org[1] - T0.seg_org[0] : 0;
    }
    a.tab = nullptr;  // (convw_kernel reads no device table)
    size_t lds = 2ull * a.xs_floats * sizeof(float) + 64;  // + slack: exact-width tiles read a few columns past the last row
    if (lds < lds_floor) lds = lds_floor;
    *lds_out = lds;
    *ntiles_out = ntiles;
    return VFX_OK;
}

// grid.x for ``ntiles`` tiles under the XCD-aware order (see the kernel): rounded up to a multiple of 8
static unsigned convw_grid_x(ConvArgs& a, int ntiles) {
    static const bool off = VFX_DEV_ENV("VFX_CONVW_XCD") && atoi(VFX_DEV_ENV("VFX_CONVW_XCD")) == 0;  // development: linear order
    a.ntiles_l = ntiles;
    if (off || ntiles < 64) { a.xcd_chunk = 0; return (unsigned)ntiles; }
    a.xcd_chunk = (ntiles + 7) / 8;
    return (unsigned)(8 * a.xcd_chunk);
}

// Optional start stagger (VFX_CONVW_STAGGER=1): the workgroups of the first residency round sleep (lin % 3) thirds of
// one tile's MFMA time, so that the workgroups sharing a CU stay a third of a tile out of phase for the whole launch.
static void convw_stagger(ConvArgs& a, long long nwg, size_t lds, int waves_per_simd) {
    static const int on = VFX_DEV_ENV("VFX_CONVW_STAGGER") ? atoi(VFX_DEV_ENV("VFX_CONVW_STAGGER")) : 0;
    a.stagger = 0;
    a.stagger_wgs = 0;
    if (!on) return;
    int per_cu = (int)((160 * 1024) / (lds ? lds : 1));
    if (per_cu > waves_per_simd) per_cu = waves_per_simd;
    if (per_cu < 2 || nwg < 256ll * per_cu * 4) return;   // short launches: the stagger would cost more than it hides
    // one tile: (Cin/8) * NT steps (x2 when fused) of 16 MFMAs x 64 cycles per wave, per_cu waves share a SIMD;
    // a third of that, in s_sleep(127) units of ~8128 cycles
    const long long steps = (long long)(a.Cin / 8) * 3 * (a.wd2 ? 2 : 1);
    const long long cycles = steps * 16 * 64 * per_cu;
    a.stagger = (int)(cycles / 3 / 8128) * on;
    if (a.stagger < 1) a.stagger = 1;
    a.stagger_wgs = 256 * per_cu;
}

// convw_kernel addresses every row of one batch item with 32-bit BYTE offsets from a per-item buffer base
static bool convw_offsets_fit(const ConvArgs& a) {
    const long long xin = ((long long)a.CinPad * a.x_cs + a.Lin + 2ll * a.x_guard) * 4;
    const long long yout = ((long long)a.Cout * a.y_cs + (long long)a.Lout * (a.y_ls > 0 ? a.y_ls : 1)) * 4;
    const long long rin = a.res ? ((long long)a.Cout * a.r_cs + a.Lout) * 4 : 0;
    return offsets_fit31(xin) && offsets_fit31(yout) && offsets_fit31(rin);
}

// unfused launch on convw_kernel; VFX_ENOTSUP -> the caller runs conv_taps_kernel
static int try_launch_convw(ConvArgs a, const vfx_tensor* x, int nphase, const PhaseSpec* phs, const float* wd,
                            hipStream_t stream) {
    static const bool off = VFX_DEV_ENV("VFX_CONVW") && atoi(VFX_DEV_ENV("VFX_CONVW")) == 0;  // development: force the first kernel
    if (off || !wd || !vfx_aligned16(wd)) return VFX_ENOTSUP;
    if (a.pad_mode != VFX_PAD_ZERO || a.in_mask || a.out_mask || a.pre_act == VFX_PRE_AFFINE_LRELU) return VFX_ENOTSUP;
    const int nt = phs[0].ntaps;
    if (nt < 2 || nt > VFX_W_MAXNT) return VFX_ENOTSUP;
    int BM, BL;
    if (a.Cout % 128 == 0) { BM = 128; BL = 128; }
    else if (a.Cout % 64 == 0) { BM = 64; BL = 256; }
    else return VFX_ENOTSUP;
    if (!convw_offsets_fit(a)) return VFX_ENOTSUP;
    size_t lds;
    int ntiles;
    a.wd = wd;
    int rc = convw_setup(a, x, nphase, phs, BL, 0, 0, 0, &lds, &ntiles);
    if (rc != VFX_OK) return rc;
    int gy = nphase * a.Cout / BM;
    // small launches (batch 1, first stages) keep the first kernel's small tiles / split-K
    if ((long long)ntiles * gy * a.B < 384) return VFX_ENOTSUP;
    dim3 grid(convw_grid_x(a, ntiles), gy, a.B);
    static const bool fold_off = VFX_DEV_ENV("VFX_CONVW_PHFOLD") && atoi(VFX_DEV_ENV("VFX_CONVW_PHFOLD")) == 0;  // development
    a.nph_fold = 0;
    if (nphase > 1 && a.xcd_chunk > 0 && !fold_off) {
        // phases of a tile adjacent in dispatch order, on one XCD (see the kernel)
        a.nph_fold = nphase;
        gy = a.Cout / BM;
        grid = dim3(grid.x * nphase, gy, a.B);
    }
    convw_stagger(a, ntiles * (long long)gy * a.B, lds, 3);
    set_last_tile(BM, BL, TILE_CONVW + a.kcx / 8);
    if (BM == 128) {
        return nt == 3 ? launch_w_nxv<128, 128, 2, 2, 3, false>(a, grid, lds, stream)
                       : launch_w_nxv<128, 128, 2, 2, 2, false>(a, grid, lds, stream);
    }
    return nt == 3 ? launch_w_nxv<64, 256, 1, 4, 3, false>(a, grid, lds, stream)
                   : launch_w_nxv<64, 256, 1, 4, 2, false>(a, grid, lds, stream);
}

// 3x3 convolution on a pitch map (vfx_conv2d_f32, ksize 3) on convw_kernel: three row segments (map rows -1, 0, +1,
// each BL + 2 columns from one position left of the tile) per 8-channel chunk, 9 weight slabs per channel group.
// VFX_ENOTSUP -> conv_taps_kernel (small launches keep its small tiles / split-K).
static int try_launch_convw_2d(ConvArgs a, const vfx_tensor* x, int P, const float* wd, hipStream_t stream) {
    static const bool off = VFX_DEV_ENV("VFX_CONVW") && atoi(VFX_DEV_ENV("VFX_CONVW")) == 0;
    static const bool off2d = VFX_DEV_ENV("VFX_CONVW2D") && atoi(VFX_DEV_ENV("VFX_CONVW2D")) == 0;  // development
    if (off || off2d || !wd || !vfx_aligned16(wd)) return VFX_ENOTSUP;
    if (a.pad_mode != VFX_PAD_ZERO || a.in_mask != P - 1 || a.out_mask != P - 1 || a.Cin % 8 != 0 || x->guard <= 0)
        return VFX_ENOTSUP;
    if (a.pre_act != VFX_PRE_NONE && a.pre_act != VFX_PRE_AFFINE_LRELU) return VFX_ENOTSUP;
    if (!convw_offsets_fit(a)) return VFX_ENOTSUP;
    int BM, BL;
    if (a.Cout % 128 == 0) {
        // the deepest UNet levels are short launches: when 128-wide tiles do not even fill one residency round (768
        // workgroups) 128 x 64 tiles double the workgroup count (measured: 384 -> 768 workgroups 78 -> 92 TFLOP/s;
        // between one and two rounds the wider tile wins, the half-empty second round runs on idle CUs)
        BM = 128;
        const long long nwg128 = (long long)((a.Lq + 127) / 128) * (a.Cout / 128) * a.B;
        BL = nwg128 < 768 ? 64 : 128;
    }
    else if (a.Cout % 64 == 0) { BM = 64; BL = 128; }
    else if (a.Cout % 32 == 0) { BM = 32; BL = 256; }
    else return VFX_ENOTSUP;
    const int ntiles = (a.Lq + BL - 1) / BL;
    const int gy = a.Cout / BM;
    if ((long long)ntiles * gy * a.B < 384) return VFX_ENOTSUP;
    a.wd = wd;
    a.kcx = 8;
    a.segw = (BL + 2 + 3) & ~3;
    a.xs_floats = 3 * a.kcx * a.segw;
    a.nxv = (3 * a.kcx * (a.segw / 4) + 255) / 256;
    a.bl_step = BL;
    a.w_tap0 = 0; a.w_tapstep = 1;
    a.w_slab0 = 0; a.w_slabstep = 1; a.w_slab_ph = 0;
    a.w_ooff0 = 0; a.w_ooff_ph = 0;
    a.w_nseg = 3; a.w_seg0 = -P - 1; a.w_segstep = P;
    a.tab = nullptr;
    a.stagger = 0; a.stagger_wgs = 0;
    a.two_level = a.Cin >= (BM == 128 && BL == 128 ? 256 : 64);   // K = 9 Cin >= 576 (2304 on the 128 x 128 tile: see the kernel)
    // interior check: every staged vector inside [-guard, Lin + guard)
    const long long g = x->guard;
    if ((long long)P + 1 > g) return VFX_ENOTSUP;
    if ((long long)(ntiles - 1) * BL + (P - 1) + a.segw > (long long)a.Lin + g) return VFX_ENOTSUP;
    const size_t lds = (2ull * a.xs_floats + 2ull * a.Cin) * sizeof(float) + 64;
    const dim3 grid(convw_grid_x(a, ntiles), gy, a.B);
    set_last_tile(BM, BL, TILE_CONVW_2D);
    if (a.two_level) {
        if (BM == 128 && BL == 64) return launch_w_one<128, 64, 2, 2, 9, 4, false, true>(a, grid, lds, stream);
        if (BM == 128) return launch_w_nxv<128, 128, 2, 2, 9, false, true>(a, grid, lds, stream);
        if (BM == 64) return launch_w_nxv<64, 128, 1, 4, 9, false, true>(a, grid, lds, stream);
        return launch_w_nxv<32, 256, 1, 4, 9, false, true>(a, grid, lds, stream);
    }
    if (BM == 128 && BL == 64) return launch_w_one<128, 64, 2, 2, 9, 4, false>(a, grid, lds, stream);
    if (BM == 128) return launch_w_nxv<128, 128, 2, 2, 9, false>(a, grid, lds, stream);
    if (BM == 64) return launch_w_nxv<64, 128, 1, 4, 9, false>(a, grid, lds, stream);
    return launch_w_nxv<32, 256, 1, 4, 9, false>(a, grid, lds, stream);
}

// One ResStack layer, fused (C = 64 or 128):  y = post( x + b2 + conv_k3_d1( lrelu_s( b1 + conv_k3_dil( lrelu_s(x) ) ) ) ) on
// convw_kernel<.., FUSED>: the intermediate tile in LDS, the dilated half a direct sum; the dilation-1 half
//  * w2_wino (optional; packing.pack_wino): 4 products per output pair instead of 6 (FUSED = 2),
//  * w2_wino4 (optional, C = 64; packing.pack_wino4): 6 products per output QUAD instead of 12 (FUSED = 3) when the tensors
//    allow 16-byte residual loads and stores; otherwise w2_wino / the direct weights decide.
// (vfx_resblock_f32 in vfx_resblk4.inc is the entry point: resblk4_kernel first, then this.)
static int resblock_convw(const vfx_tensor* x, const vfx_tensor* y, const float* w1_direct, const float* bias1,
                          const float* w2_direct, const float* bias2, const float* w2_wino, const float* w2_wino4,
                          int B, int C, int L, int dilation, float slope, int post_act, float post_slope,
                          vfx_stream_t stream) {
    if (!x || !y || !x->ptr || !y->ptr || !w1_direct || !w2_direct || B <= 0 || L <= 0 || dilation < 1 || B > 65535)
        return VFX_EINVAL;
    static const bool w2off = VFX_DEV_ENV("VFX_FUSE_WINO") && atoi(VFX_DEV_ENV("VFX_FUSE_WINO")) == 0;  // development
    if (w2off || !vfx_aligned16(w2_wino)) w2_wino = nullptr;
    static const bool w4off = VFX_DEV_ENV("VFX_FUSE_WINO4") && atoi(VFX_DEV_ENV("VFX_FUSE_WINO4")) == 0;  // development
    if (w2off || w4off || !vfx_aligned16(w2_wino4) || C != 64 || y->lstride != 1 || (y->cstride & 3) || (y->bstride & 3) ||
        !vfx_aligned16(y->ptr))
        w2_wino4 = nullptr;
    if (C != 64 && C != 128) return VFX_ERANGE;
    if (x->lstride != 1 || (x->cstride & 3) || (x->bstride & 3) || !vfx_aligned16(x->ptr) || !vfx_aligned16(w1_direct) ||
        !vfx_aligned16(w2_direct))
        return VFX_EALIGN;
    if (x->ptr == y->ptr) return VFX_EINVAL;  // tiles read their neighbours' input columns: not an in-place update
    if (!offsets_fit31(((long long)C * x->cstride + L + 2 * x->guard) * 4) || !offsets_fit31(((long long)C * y->cstride + L) * 4))
        return VFX_ERANGE;  // 32-bit byte offsets within one batch item
    ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x = (const float*)x->ptr;
    a.wd = w1_direct;
    a.wd2 = w2_wino4 ? w2_wino4 : (w2_wino ? w2_wino : w2_direct);
    a.bias = bias1;
    a.bias2 = bias2;
    a.res = a.x;
    a.res_init = 1;
    a.y = (float*)y->ptr;
    a.B = B; a.Cin = C; a.CinPad = C; a.Cout = C;
    a.Lin = L; a.Lq = L; a.Lout = L;
    a.x_bs = x->bstride; a.x_cs = x->cstride;
    a.x_guard = (int)x->guard;
    a.x_rows = x->rows;
    a.lq_extra = 0;
    a.r_bs = x->bstride; a.r_cs = x->cstride; a.r_ls = 1;
    a.y_bs = y->bstride; a.y_cs = y->cstride; a.y_ls = y->lstride;
    a.q_shift = 31; a.q_mask = 0x7fffffff; a.o_rs = 0; a.o_cs = 1;
    a.pad_mode = VFX_PAD_ZERO;
    if (!(slope >= 0.f && slope <= 1.f) || (post_act == VFX_POST_LRELU && !(post_slope >= 0.f && post_slope <= 1.f)))
        return VFX_EINVAL;      // (leaky ReLU is evaluated as max(v, slope * v))
    a.pre_act = VFX_PRE_LRELU;
    a.pre_slope = slope;
    a.mid_slope = slope;
    a.post_act = post_act;
    a.post_slope = post_slope;
    PhaseSpec ph;
    ph.ntaps = 3;
    ph.ooff = 0;
    for (int t = 0; t < 3; ++t) { ph.taps[t].off = (t - 1) * dilation; ph.taps[t].slab = t; }
    // tile: accumulator columns BL, outputs BL - 2
    static const int bl_env = VFX_DEV_ENV("VFX_FUSE_BL") ? atoi(VFX_DEV_ENV("VFX_FUSE_BL")) : 0;  // development: 64 / 128 / 256
    int BL = C == 64 ? 256 : 128;
    if (bl_env == 128 && C == 64) BL = 128;
    if (bl_env == 64 && C == 128) BL = 64;
    a.yp = BL + 4;
    size_t lds;
    int ntiles;
    if (w2_wino4 && BL != 256) w2_wino4 = nullptr, a.wd2 = w2_wino ? w2_wino : w2_direct;
    // outputs per tile: BL - 2 (conv-2 needs one column either side); F(4,3): whole quads, 63 of them
    int rc = convw_setup(a, x, 1, &ph, BL, 1, w2_wino4 ? BL - 4 : BL - 2, (size_t)C * a.yp * sizeof(float), &lds, &ntiles);
    if (rc != VFX_OK) return rc == VFX_ENOTSUP ? VFX_ERANGE : rc;
    // consecutive tiles per workgroup: enough to amortise the cross-tile prefetch, few enough that the launch still
    // fills the chip several times over (tail) -- VFX_FUSE_TPW overrides (development)
    static const int tpw_env = VFX_DEV_ENV("VFX_FUSE_TPW") ? atoi(VFX_DEV_ENV("VFX_FUSE_TPW")) : 0;
    int tpw = VFX_W_MULTITILE ? (tpw_env > 0 ? tpw_env : 8) : 1;
    while (tpw > 1 && (long long)((ntiles + tpw - 1) / tpw) * B < 4096) tpw >>= 1;
    a.tpw = tpw;
    const dim3 grid(tpw == 1 ? convw_grid_x(a, ntiles) : (unsigned)((ntiles + tpw - 1) / tpw), 1, B);
    if (tpw != 1) { a.xcd_chunk = 0; a.ntiles_l = ntiles; }
    convw_stagger(a, (long long)grid.x * B, lds, (C == 64 && BL == 128) || (C == 128 && BL == 64) ? 3 : 2);
    hipStream_t s = (hipStream_t)stream;
    if (w2_wino4) {
        set_last_tile(C, BL, TILE_FUSED_F43 + a.kcx / 8);
        return launch_w_nxv<64, 256, 1, 4, 3, 3>(a, grid, lds, s);
    }
    if (w2_wino && C == 64 && BL == 256) {
        set_last_tile(C, BL, TILE_FUSED_F23 + a.kcx / 8);
        return launch_w_nxv<64, 256, 1, 4, 3, 2>(a, grid, lds, s);
    }
    if (w2_wino && C == 128 && BL == 128) {
        set_last_tile(C, BL, TILE_FUSED_F23 + a.kcx / 8);
        return launch_w_nxv<128, 128, 2, 2, 3, 2>(a, grid, lds, s);
    }
    set_last_tile(C, BL, TILE_FUSED + a.kcx / 8);
    if (C == 64) {
        return BL == 256 ? launch_w_nxv<64, 256, 1, 4, 3, 1>(a, grid, lds, s)
                         : launch_w_nxv<64, 128, 1, 4, 3, 1>(a, grid, lds, s);
    }
    return BL == 128 ? launch_w_nxv<128, 128, 2, 2, 3, 1>(a, grid, lds, s)
                     : launch_w_nxv<128, 64, 2, 2, 3, 1>(a, grid, lds, s);
}
