// vfx_resblk4.inc -- included by vfx_conv.hip after vfx_convwg2d.inc.
//
// resblk4_kernel (round 4): one whole ResStack layer of the C = 64 stage
//     x <- post( x + b2 + conv_k3_d1( lrelu( b1 + conv_k3_dil( lrelu(x) ) ) ) )      (voicefixer/vocoder/model/modules.py:592-609)
// with BOTH convolutions as Winograd F(4,3) and the intermediate tile in LDS, for the dilations whose blocks of 4d positions fit
// a 256-column tile (d = 1, 3, 9, 27: four of the stage's eight layers).  convw_kernel<.., FUSED = 3> (vfx_convw.inc) runs the
// dilated half as the direct sum -- 384 of its 576 MFMAs per wave and tile; here that half forms 6 products per four outputs
// a dilation apart (192 MFMAs), exactly as convwg4_kernel does, but writes its output transform into the natural-order tile
// Y[64][W] in LDS instead of to HBM, and the second half (F(4,3) along adjacent positions, residual and stores as 16-byte
// vectors) is the code of FUSED = 3.
//
// Tile geometry.  A workgroup owns the Y columns [y0, y0 + W), y0 = q0 - 1, W = 4 d NB (NB whole blocks of 4d positions:
// 256 / 252 / 252 / 216 columns for d = 1 / 3 / 9 / 27), i.e. the NB d <= 64 quads  u0 = 4 d blk + r  (outputs at columns u0 + i d).
// The block grid is LOCAL to the tile (nothing requires blocks to start at position 0), so q0 can be any multiple of 4 and the
// second half's output quads stay aligned float4 in memory.  Of the W columns the second half turns 4 nq2 = 4 floor((W - 2) / 4)
// into outputs (q0 .. q0 + 4 nq2 - 1: it needs one column either side, and whole quads), which is the tile step -- 252 / 248 /
// 248 / 212: 1.6 % .. 1.9 % of the first half is recomputed by the neighbour tile, as in FUSED = 3.
// First half: wave = 32 channels x 32 quads x 6 planes (waves: 2 channel blocks x 2 quad blocks), K = 64 = four chunks of 16
// channels staged as in convwg4_kernel<2,2> (dword tap loads with out-of-range offsets as the zero padding, leaky ReLU, B^T, six
// planes to LDS, double buffered, woven between the MFMAs), A vectors (packing.pack_wino4 of the FIRST convolution) from L2.
// Between the halves: output transform (+ b1 came in through the first k-step's C operand), leaky ReLU, zero outside [0, L) (the second
// convolution's zero padding), scattered into Y (which aliases the staging buffers: every wave is past its last fragment read).
// Second half: see convw_kernel<.., FUSED = 3>; all six planes start at zero, and b2 and the residual are added after the output
// transform, element by element.
// Rounding (DESIGN.md 3.3, tests/test_resblk4_gpu.py): nothing but products enters the second half's accumulators.  While A^T m =
// x + b2 was solved for the start values of planes 0, 1, 3, 5, every partial sum was rounded at several times the residual (start
// values up to 5 |x| of the quad's largest element, then 8 m34 in the output transform): with weight-norm gains below one, where
// the residual is most of the answer, the layer measured 30 - 400 x the fp32 F(4,3) statement's maximum error and 10 - 36 x its RMS.
// Per-row lengths (ragged batches) as everywhere: taps and Y columns past the row's own end are zero, tiles past it return.
// The body is shared with resblk4s_kernel (vfx_resblk4s.inc, STRIP = true): the two differ in the tile geometry only -- which
// quads the first half computes (quad_p / quad_ok), where their outputs go in Y (quad_col, ystep), and which output quads the second
// half owns (qq, nown, yc2).  Staging, MFMAs, the transform between the halves, the second half and the epilogue are one code.
template <bool STRIP>
__device__ __forceinline__ void resblk4_body(const ConvArgs& a) {
    constexpr int C = 64, KC = 16, NSTEP = KC / 2, S = C / KC;
    constexpr int BQ = 64, CG = 256 / BQ, NSLOT = KC / CG;      // 4 channel groups, 4 staged elements per thread and chunk
    constexpr int PLANE = KC * BQ, BUF = 6 * PLANE;
    static_assert(NSTEP / NSLOT == 2, "two k-pair steps per staged element");
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lo = lane & 31, hi = lane >> 5;
    const int wm = wave & 1, wq = wave >> 1;      // channel block (32 rows), quad block (32 quads) -- both halves
    int bx = blockIdx.x;
    if (a.xcd_chunk > 0) {                        // XCD-aware tile order (see convw_kernel)
        bx = (bx & 7) * a.xcd_chunk + (bx >> 3);
        if (bx >= a.ntiles_l) return;
    }
    const int b = blockIdx.z;
    const int d = a.wg_d;
    const float inv_d = 1.0f / (float)d;
    const int Lrow = a.x_rows ? __builtin_amdgcn_readfirstlane(a.x_rows[b]) : a.Lin;
    const int xcs = (int)a.x_cs;
    // ---- tile geometry
    // block tile (resblk4_kernel): Y columns [q0 - 1, q0 - 1 + W), NB whole blocks of 4d columns, outputs [q0, q0 + bl_step)
    const int q0 = STRIP ? 0 : bx * a.bl_step;    // first OUTPUT position of this tile (a multiple of 4)
    const int nq1 = a.rb_nq1;                     // quads of the first half: NB * d
    // strip tile (resblk4s_kernel): G = 64 / P segments, segment n = G bx + g of the row covers r in [r0, r0 + W) of block blk
    const int pshift = STRIP ? a.rs_pshift : 6, P = 1 << pshift, W = P - 4;
    int sstart[2] = {0, 0}, sr0[2] = {0, 0};      // per segment of the tile: first output position of strip 0, r0
    if constexpr (STRIP) {
        const int nseg = a.rs_nseg;
        const float inv_nseg = 1.0f / (float)nseg;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int n = (bx << (6 - pshift)) + g;
            const int blk = fast_div(n, nseg, inv_nseg);
            sr0[g] = (n - blk * nseg) * W;
            sstart[g] = 4 * d * blk + sr0[g];
        }
    }
    if ((STRIP ? sstart[0] : q0) >= Lrow) return;
    auto quad_u0 = [&](int Q) {                   // block tile: Y column of output 0 of first-half quad Q (blocks of 4d columns)
        const int blk = fast_div(Q, d, inv_d);
        return 4 * d * blk + (Q - blk * d);
    };
    auto quad_p = [&](int Q) {                    // position of output 0 of first-half quad Q
        if constexpr (STRIP) return (Q >> pshift ? sstart[1] : sstart[0]) - 1 + (Q & (P - 1));   // segment Q >> pshift, column Q & (P - 1)
        else return q0 - 1 + quad_u0(Q);
    };
    auto quad_ok = [&](int Q) {                   // (strip: W + 2 quads per segment)
        if constexpr (STRIP) return (Q & (P - 1)) < P - 2;
        else return Q < nq1;
    };
    auto quad_col = [&](int Q) {                  // Y column of its output 0; output i lies ystep columns further (strip: Y strip 4 g + i)
        if constexpr (STRIP) return ((Q >> pshift) << (pshift + 2)) + (Q & (P - 1));
        else return quad_u0(Q);
    };
    const int ystep = STRIP ? P : d;

    // ================================================================ first half: conv_k3_dil as F(4,3) along the dilated axis
    const int sq = tid % BQ, cg = tid / BQ;
    int xvoff[6];
    {
        const int p0 = quad_p(sq);
        const bool qok = quad_ok(sq);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int p = p0 + (j - 1) * d;
            xvoff[j] = (qok && p >= 0 && p < Lrow) ? (cg * xcs + p) * 4 : VFX_W_OOB;   // outside the row: reads 0 = the zero padding
        }
    }
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.x) + (long long)b * a.x_bs, (short)0, 0x7fffffff, 0x00020000);
    const float slope = a.pre_slope;
    const int wcol = (sq + 32 * (cg & 1)) & 63;   // odd channels rotated by 32 columns (B-fragment reads: disjoint banks)
    float* const wbase = smem + cg * BQ + wcol;
    float xv[NSLOT][6];
    auto x_load_part = [&](int j, int t, int s0) {
        xv[j][t] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xrsrc, xvoff[t], s0 + j * CG * xcs * 4, 0));
    };
    auto x_load = [&](int chunk) {
        const int s0 = chunk * KC * xcs * 4;
#pragma unroll
        for (int j = 0; j < NSLOT; ++j)
#pragma unroll
            for (int t = 0; t < 6; ++t) x_load_part(j, t, s0);
    };
    auto x_transform = [&](int j, float (&V)[6]) {
        float e[6];
#pragma unroll
        for (int t = 0; t < 6; ++t) e[t] = fmaxf(xv[j][t], xv[j][t] * slope);
        const float s1 = fmaf(-4.f, e[2], e[4]), s2 = fmaf(-4.f, e[1], e[3]);
        const float s3 = e[4] - e[2], s4 = e[3] - e[1];
        V[0] = fmaf(4.f, e[0], fmaf(-5.f, e[2], e[4]));
        V[1] = s1 + s2;
        V[2] = s1 - s2;
        V[3] = fmaf(2.f, s4, s3);
        V[4] = fmaf(-2.f, s4, s3);
        V[5] = fmaf(4.f, e[1], fmaf(-5.f, e[3], e[5]));
    };
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wd), (short)0, 0x7fffffff, 0x00020000);
    const int row1 = 32 * wm;
    const int avoff = ((row1 + lo) * 8 + 4 * hi) * 4;
    constexpr int gstride = C * 32;               // bytes per (plane, 8-channel group)
    constexpr int pstride = (C >> 3) * gstride;   // bytes per plane
    float4 aw[2][6];
    auto a_load_one = [&](auto set_tag, int k, int grp) {
        constexpr int SET = decltype(set_tag)::value;
        const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, avoff, k * pstride + grp * gstride, 0);
        aw[SET][k] = make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;

    // the issue block: bias 1, taps of chunk 0, first A vectors (nothing but loads)
    const __amdgpu_buffer_rsrc_t b1rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.bias ? a.bias : a.x), (short)0, 0x7fffffff, 0x00020000);
    u32x4 bq[4];
    {
        const int bvoff = a.bias ? (row1 + 4 * hi) * 4 : VFX_W_OOB;
#pragma unroll
        for (int g = 0; g < 4; ++g) bq[g] = __builtin_amdgcn_raw_buffer_load_b128(b1rsrc, bvoff, g * 32, 0);
    }
    x_load(0);
#pragma unroll
    for (int k = 0; k < 6; ++k) a_load_one(S0{}, k, 0);
    __builtin_amdgcn_sched_barrier(0);

    f32x16 acc[6];
    const int bcol = (32 * wq + lo + 32 * hi) & 63;
    const int boffs = hi * BQ + bcol;
    // one chunk: 8 k-pair steps x 6 MFMAs; element el of the thread is staged during steps 2 el (transform + six LDS writes) and
    // 2 el + 1 (its six tap loads for the chunk after next); A vectors of the next 8-channel group in the first step of each group
    // (round 5) no accumulator is initialised by moves: the MFMAs of the first k-step take C = 0 (inline constant), plane 1 takes
    // C = the bias vector as loaded -- y_i = m1 + ..., so a start value of b1 in plane 1 IS "+ b1" on all four outputs.  (Every later
    // partial sum of plane 1 is then rounded at the size of b1.  Measured, tests/test_resblk4_gpu.py: with unit-scale biases and
    // heavy-tailed gains the layer is at 0.35 - 1.5 x the fp32 F(4,3) statement's error either way -- what is lost here is scaled
    // by the second convolution's weights, and the figure's magnitude holds sum |w2| |b1|.  So it stays: it costs no VALU.)
    f32x16 biasv;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        biasv[4 * g + 0] = __uint_as_float(bq[g].x); biasv[4 * g + 1] = __uint_as_float(bq[g].y);
        biasv[4 * g + 2] = __uint_as_float(bq[g].z); biasv[4 * g + 3] = __uint_as_float(bq[g].w);
    }
    auto mma_chunk = [&](auto first_tag, const float* xs, float* wdst, int xchunk, int agrp0) {
        constexpr bool FIRST = decltype(first_tag)::value;
        const float* bp = xs + boffs;
        const int agrp1 = min(agrp0 + 1, 2 * S - 1), agrp2 = min(agrp0 + 2, 2 * S - 1);
        float bf[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) bf[k] = bp[k * PLANE];
        const int xs0 = xchunk * KC * xcs * 4;
        float V[6];
#pragma unroll
        for (int u = 0; u < NSTEP; ++u) {
            const int el = u >> 1, ph = u & 1;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                if (ph == 0 && k == 0) x_transform(el, V);
                if (ph == 0) wdst[el * CG * BQ + k * PLANE] = V[k];
                if (ph == 1) x_load_part(el, k, xs0);
                if (u == 0) a_load_one(S1{}, k, agrp1);
                if (u == 4) a_load_one(S0{}, k, agrp2);
                const float4 av4 = (u < 4) ? aw[0][k] : aw[1][k];
                const int kk = u & 3;
                const float av = kk == 0 ? av4.x : (kk == 1 ? av4.y : (kk == 2 ? av4.z : av4.w));
                if (FIRST && u == 0) {
                    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[k], k == 1 ? biasv : zero16, 0, 0, 0);
                } else {
                    acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[k], acc[k], 0, 0, 0);
                }
                if (u < NSTEP - 1) bf[k] = bp[k * PLANE + (u + 1) * 2 * BQ];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    {   // chunk 0 to LDS, chunk 1 in flight
#pragma unroll
        for (int j = 0; j < NSLOT; ++j) {
            float V[6];
            x_transform(j, V);
#pragma unroll
            for (int k = 0; k < 6; ++k) wbase[j * CG * BQ + k * PLANE] = V[k];
        }
        x_load(1);
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    mma_chunk(std::true_type{}, smem, wbase + BUF, 2, 0);   // (the first pair of chunks peeled: chunk 0 starts the accumulators)
    __syncthreads();
    mma_chunk(std::false_type{}, smem + BUF, wbase, 3, 2);
    __syncthreads();
#pragma unroll 1
    for (int s = 2; s < S; s += 2) {
        mma_chunk(std::false_type{}, smem, wbase + BUF, min(s + 2, S - 1), 2 * s);
        __syncthreads();
        mma_chunk(std::false_type{}, smem + BUF, wbase, min(s + 3, S - 1), 2 * s + 2);
        __syncthreads();
    }

    // ================================================================ between the halves: Y = lrelu(conv1 + b1), zero outside the row
    // (second-half loads first: the first A vectors are in flight while Y is written and the barrier waits)
    const int row2 = 32 * wm;
    const __amdgpu_buffer_rsrc_t w2rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wd2), (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.x) + (long long)b * a.x_bs, (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(
        a.y + (long long)b * a.y_bs, (short)0, 0x7fffffff, 0x00020000);
    float4 aw2[2][6];
    auto a2_load = [&](auto set_tag, int grp) {
        constexpr int SET = decltype(set_tag)::value;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(w2rsrc, avoff, k * pstride + grp * gstride, 0);
            aw2[SET][k] = make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
        }
    };
    const int Qi = 32 * wq + lo;                  // second half: output quad of this lane within the tile
    int qq, nown, yc2;                            // its first output position, how many of its 4 outputs the tile owns, its Y column
    bool has_tail;                                // (wave-uniform) some quad is partly owned
    if constexpr (STRIP) {
        // quad jq of strip t (strip i = t & 3 of segment g = t >> 2), W / 4 quads per strip.  Its four positions are consecutive
        // but not 16-byte aligned (d is odd): residual and stores are unaligned dwordx4 accesses.  An output belongs to this tile
        // when its r = r0 + 4 jq + e < d (r >= d is the next strip's, computed by another tile) and it lies inside the row.
        const int nq2s = W >> 2;
        int t = fast_div(Qi, nq2s, 1.0f / (float)nq2s);
        const int jq = Qi - t * nq2s;
        const bool sok = t < (4 << (6 - pshift));
        t = sok ? t : 0;
        const int rr = ((t >> 2) ? sr0[1] : sr0[0]) + 4 * jq;
        qq = ((t >> 2) ? sstart[1] : sstart[0]) + (t & 3) * d + 4 * jq;
        nown = sok ? min(Lrow - qq, d - rr) : 0;
        has_tail = __any(nown > 0 && nown < 4);
        yc2 = (t << pshift) + 4 * jq;
    } else {
        const int qend = min(Lrow, q0 + a.bl_step);
        qq = q0 + 4 * Qi;
        nown = qend - qq;
        has_tail = (qend & 3) != 0;               // (uniform) the tile ends inside a quad
        yc2 = 4 * Qi;
    }
    const bool full = nown >= 4;
    const int rvq = full ? (4 * hi * xcs + qq) * 4 : VFX_W_OOB;
    const int yvq = full ? (4 * hi * (int)a.y_cs + qq) * 4 : VFX_W_OOB;
    int rv1[4], yv1[4];                           // single elements: the partly owned quads only
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool one = !full && i < nown;
        rv1[i] = one ? (4 * hi * xcs + qq + i) * 4 : VFX_W_OOB;
        yv1[i] = one ? (4 * hi * (int)a.y_cs + qq + i) * 4 : VFX_W_OOB;
    }
    a2_load(S0{}, 0);
    // residual quads and b2: wanted by the epilogue only, issued before the last pair of channel groups (the tile's own columns were
    // read by the first half: L2 holds them)
    u32x4 rq[16], bq2[4];
    auto res_load = [&]() {
        const int cs4 = xcs * 4;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            rq[r] = __builtin_amdgcn_raw_buffer_load_b128(rrsrc, rvq, (row2 + (r & 3) + 8 * (r >> 2)) * cs4, 0);
        const __amdgpu_buffer_rsrc_t b2rsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(a.bias2 ? a.bias2 : a.x), (short)0, 0x7fffffff, 0x00020000);
        const int bvoff = a.bias2 ? (row2 + 4 * hi) * 4 : VFX_W_OOB;
#pragma unroll
        for (int g = 0; g < 4; ++g) bq2[g] = __builtin_amdgcn_raw_buffer_load_b128(b2rsrc, bvoff, g * 32, 0);
    };
    float* const Y = smem;                        // aliases the staging buffers
    const int yp = a.yp;
    {
        const float ms = a.mid_slope;
        const int Q1 = 32 * wq + lo;              // first-half quad of this lane's accumulator column
        const int p1 = quad_p(Q1);
        bool ok[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = p1 + i * d;
            ok[i] = p >= 0 && p < Lrow;           // conv-2's zero padding: Y is zero outside the sequence
        }
        if (quad_ok(Q1)) {
            float* ycol = Y + (row1 + 4 * hi) * yp + quad_col(Q1);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p12 = acc[1][r] + acc[2][r], m12 = acc[1][r] - acc[2][r];
                const float p34 = acc[3][r] + acc[4][r], m34 = acc[3][r] - acc[4][r];
                float v[4];
                v[0] = (acc[0][r] + p12) + p34;
                v[1] = fmaf(2.f, m34, m12);
                v[2] = fmaf(4.f, p34, p12);
                v[3] = fmaf(8.f, m34, m12) + acc[5][r];
                float* yr = ycol + ((r & 3) + 8 * (r >> 2)) * yp;
#pragma unroll
                for (int i = 0; i < 4; ++i) yr[i * ystep] = ok[i] ? fmaxf(v[i], v[i] * ms) : 0.f;
            }
        }
    }
    __syncthreads();

    // ================================================================ second half: conv_k3_d1 as F(4,3) on Y (as convw_kernel<.., FUSED = 3>)
    // all six planes start at zero (keeping the 64 residual registers through this whole half instead spills: the A vectors of two
    // groups and the Y fragments are live as well -- so they are loaded for the epilogue, late)
    f32x16 accq[6];
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) accq[k][r] = 0.f;
    const float* yb = Y + hi * yp + yc2;
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
                if constexpr (SET == 0) a2_load(S1{}, nxt);
                else a2_load(S0{}, nxt);
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
    constexpr int ngrp = C >> 3;
#pragma unroll 1
    for (int grp = 0; grp < ngrp; grp += 2) {
        if (grp == ngrp - 2) res_load();
        group(S0{}, grp, grp + 1);
        group(S1{}, grp + 1, min(grp + 2, ngrp - 1));
    }
    // output transform, activation, stores
    {
        const int post = a.post_act;
        const float ps = a.post_slope;
        const int cs4 = (int)a.y_cs * 4;
        if (has_tail) {                           // the partly owned quads' residual, element by element (their b128 offset is out of range: 0)
            const int xcs4 = xcs * 4;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int soff = (row2 + (r & 3) + 8 * (r >> 2)) * xcs4;
                rq[r].x |= __builtin_amdgcn_raw_buffer_load_b32(rrsrc, rv1[0], soff, 0);
                rq[r].y |= __builtin_amdgcn_raw_buffer_load_b32(rrsrc, rv1[1], soff, 0);
                rq[r].z |= __builtin_amdgcn_raw_buffer_load_b32(rrsrc, rv1[2], soff, 0);
                rq[r].w |= __builtin_amdgcn_raw_buffer_load_b32(rrsrc, rv1[3], soff, 0);
            }
        }
        // A^T m, then + b2, then + x (nothing but products went through the accumulators), back into planes 0 .. 3: rq and bq2 are
        // indexed by constants only (the post-activation loop below may not be unrolled)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p12 = accq[1][r] + accq[2][r], m12 = accq[1][r] - accq[2][r];
            const float p34 = accq[3][r] + accq[4][r], m34 = accq[3][r] - accq[4][r];
            const u32x4 bg = bq2[r >> 2];
            const float bb = __uint_as_float((r & 3) == 0 ? bg.x : ((r & 3) == 1 ? bg.y : ((r & 3) == 2 ? bg.z : bg.w)));
            const float y3 = ((fmaf(8.f, m34, m12) + accq[5][r]) + bb) + __uint_as_float(rq[r].w);
            accq[0][r] = (((accq[0][r] + p12) + p34) + bb) + __uint_as_float(rq[r].x);
            accq[1][r] = (fmaf(2.f, m34, m12) + bb) + __uint_as_float(rq[r].y);
            accq[2][r] = (fmaf(4.f, p34, p12) + bb) + __uint_as_float(rq[r].z);
            accq[3][r] = y3;
        }
        auto outs = [&](int r, float (&y)[4]) {
            y[0] = accq[0][r]; y[1] = accq[1][r]; y[2] = accq[2][r]; y[3] = accq[3][r];
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
        if (post == VFX_POST_NONE) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float y[4];
                outs(r, y);
                store4(y, (row2 + (r & 3) + 8 * (r >> 2)) * cs4);
            }
        } else if (post == VFX_POST_LRELU) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float y[4];
                outs(r, y);
#pragma unroll
                for (int i = 0; i < 4; ++i) y[i] = fmaxf(y[i], y[i] * ps);
                store4(y, (row2 + (r & 3) + 8 * (r >> 2)) * cs4);
            }
        } else {
#pragma unroll 1
            for (int r = 0; r < 16; ++r) {
                float y[4];
                outs(r, y);
#pragma unroll
                for (int i = 0; i < 4; ++i) y[i] = vfx_post(y[i], post, ps);
                store4(y, (row2 + (r & 3) + 8 * (r >> 2)) * cs4);
            }
        }
    }
}

__global__ __launch_bounds__(256, 2) void resblk4_kernel(const ConvArgs a) { resblk4_body<false>(a); }


// Argument checks and kernel arguments shared by resblk4_kernel and resblk4s_kernel (vfx_resblk4s.inc): C = 64, both F(4,3)
// weight sets, 16-byte aligned rows with unit stride, x and y distinct, every byte offset of a batch item within 32 bits.
static bool resblk4_args_ok(const vfx_tensor* x, const vfx_tensor* y, const vfx_resblock_w* w, int B, int C, int L, int dilation,
                            float slope, int post_act, float post_slope) {
    const float *bias1 = w->bias1, *bias2 = w->bias2, *w2_wino4 = w->w2_wino4, *w1_wino4 = w->w1_wino4;
    bool ok = x && y && x->ptr && y->ptr && w1_wino4 && w2_wino4 && C == 64 && B > 0 && B <= 65535 && L > 0 && dilation >= 1 &&
              x->ptr != y->ptr;
    if (ok) {
        ok = vfx_aligned16(w1_wino4) && vfx_aligned16(w2_wino4) && vfx_aligned16(x->ptr) && vfx_aligned16(y->ptr) && x->lstride == 1 &&
             y->lstride == 1 && ((x->cstride | x->bstride | y->cstride | y->bstride) & 3) == 0 &&
             (!bias1 || vfx_aligned16(bias1)) && (!bias2 || vfx_aligned16(bias2)) && slope >= 0.f && slope <= 1.f &&
             !(post_act == VFX_POST_LRELU && !(post_slope >= 0.f && post_slope <= 1.f)) &&
             offsets_fit31(((long long)C * x->cstride + L) * 4) && offsets_fit31(((long long)C * y->cstride + L) * 4);
    }
    return ok;
}

static void resblk4_fill_args(ConvArgs& a, const vfx_tensor* x, const vfx_tensor* y, const vfx_resblock_w* w, int B, int C, int L,
                              int dilation, float slope, int post_act, float post_slope) {
    std::memset(&a, 0, sizeof(a));
    a.x = (const float*)x->ptr;
    a.wd = w->w1_wino4;
    a.wd2 = w->w2_wino4;
    a.bias = w->bias1;
    a.bias2 = w->bias2;
    a.y = (float*)y->ptr;
    a.B = B; a.Cin = C; a.CinPad = C; a.Cout = C;
    a.Lin = L; a.Lq = L; a.Lout = L;
    a.x_bs = x->bstride; a.x_cs = x->cstride;
    a.x_rows = x->rows;
    a.y_bs = y->bstride; a.y_cs = y->cstride; a.y_ls = 1;
    a.pre_act = VFX_PRE_LRELU;
    a.pre_slope = slope;
    a.mid_slope = slope;
    a.post_act = post_act;
    a.post_slope = post_slope;
    a.wg_d = dilation;
    a.yp = 260;
}

// The 64-column F(4,3) tile takes a dilation whose blocks of 4d positions fill a 256-column tile: d <= 32 with at least 48 of
// the 64 quad columns used (the stage's d = 1, 3, 9, 27).
static bool resblk4_takes(int dilation) {
    const int nb = 256 / (4 * dilation);
    return dilation <= 32 && nb >= 1 && nb * dilation >= 48;
}

static int resblk4_launch(const vfx_tensor* x, const vfx_tensor* y, const vfx_resblock_w* w, int B, int C, int L, int dilation,
                          float slope, int post_act, float post_slope, vfx_stream_t stream) {
    ConvArgs a;
    resblk4_fill_args(a, x, y, w, B, C, L, dilation, slope, post_act, post_slope);
    const int nb = 256 / (4 * dilation);
    const int W = 4 * dilation * nb;              // Y columns a tile computes
    const int nq2 = (W - 2) / 4;                  // output quads of the second half
    a.rb_nq1 = nb * dilation;
    a.bl_step = 4 * nq2;
    const int ntiles = (L + a.bl_step - 1) / a.bl_step;
    const size_t lds = (size_t)C * a.yp * sizeof(float);   // 66 560 bytes (the staging buffers, 49 152, alias it)
    const dim3 grid(convw_grid_x(a, ntiles), 1, B);
    set_last_tile(C, 256, TILE_RESBLK4);
    return vfx_launch<resblk4_kernel>(grid, dim3(256), lds, (hipStream_t)stream, a);
}

// vfx_resblock_f32 (include/vfx_hip.h): one ResStack layer, fused.  With both F(4,3) transforms offered, C = 64, a dilation
// resblk4_takes() and 16-byte aligned rows: resblk4_kernel.  Anything else: resblock_convw (vfx_convw.inc) decides.
extern "C" int vfx_resblock_f32(const vfx_tensor* x, const vfx_tensor* y, const vfx_resblock_w* w, int B, int C, int L,
                                int dilation, float slope, int post_act, float post_slope, vfx_stream_t stream) {
    if (!w) return VFX_EINVAL;
    static const bool off = (VFX_DEV_ENV("VFX_FUSE_WINO44") && atoi(VFX_DEV_ENV("VFX_FUSE_WINO44")) == 0) ||
                            (VFX_DEV_ENV("VFX_FUSE_WINO4") && atoi(VFX_DEV_ENV("VFX_FUSE_WINO4")) == 0) ||
                            (VFX_DEV_ENV("VFX_FUSE_WINO") && atoi(VFX_DEV_ENV("VFX_FUSE_WINO")) == 0);   // development
    if (off || !resblk4_takes(dilation) || !resblk4_args_ok(x, y, w, B, C, L, dilation, slope, post_act, post_slope)) {
        return resblock_convw(x, y, w->w1_direct, w->bias1, w->w2_direct, w->bias2, w->w2_wino, w->w2_wino4, B, C, L, dilation, slope,
                              post_act, post_slope, stream);
    }
    return resblk4_launch(x, y, w, B, C, L, dilation, slope, post_act, post_slope, stream);
}
