// vfx_level_span_rows.inc -- the LINKED streaming loudness leveller of a session of several channels (vfx_level_span_rows_f32;
// definition, resources and measured cost: DESIGN.md 3.18; included by vfx_loudness.hip behind vfx_level_span.inc, whose span
// record, state layout and workspace layout (lv_span, LV_*, lv_layout, lv_chunk) it uses as they are).
//
// The leveller of vfx_level_span.inc with ONE energy per quarter for the C channels of a programme:
//     E_q = sum_c w_c E_{q,c}      (fp64, c ascending from 0.0, every product and every sum rounded on its own),
// E_{q,c} the local quarter energy of channel c as there (same regions, chunks and tree: its bits do not depend on the window),
// w the BS.1770-4 channel weights.  Anchors, hold, clamp, a_q and the fp32 ramp are unchanged; the ramp multiplies every channel.
// Channel ch's window is xw + ch w_stride, its outputs out + ch out_stride; g0, wlen, n_total and the state are the programme's.
//   1. lvr_quarter_kernel: lv_quarter_kernel's body per (new quarter, channel): grid (ne(m1) - ne(m0), C); writes E_{q,c} into
//      channel c's slots of the workspace.
//   2. lvr_anchor_kernel: one workgroup: first the weighted sums of the new quarters in the order above into the slots the mono
//      kernel fills, then lv_anchor_kernel's body on them.
//   3. lvr_apply_kernel: grid (blocks, C); four outputs per lane, 16-byte loads and stores where THIS channel's addresses allow.
// At most three launches per call, whatever C.  C = 1, w = {1}: 0 + 1 E is exact -- the bits and the state of vfx_level_span_f32.
#define LVR_CMAX 8

struct lvr_rows {
    long long w_stride, out_stride;
    long long eslots;             // energy slots per channel
    double* ewc;                  // [C][eslots]
    double w[LVR_CMAX];
    int C;
};

static void lvr_layout(long long n_span, int hop, int C, size_t* total, lv_span* s, lvr_rows* r, char* base) {
    size_t off = 0;
    lv_layout(n_span, hop, &off, s, base);
    const long long slots = n_span / hop + 13;
    const size_t o_c = off; off += lk_round((size_t)C * (size_t)slots * sizeof(double));
    *total = off;
    if (r) {
        r->eslots = slots;
        r->ewc = (double*)(base + o_c);
    }
}

__global__ __launch_bounds__(LK_T) void lvr_quarter_kernel(const float* __restrict__ xw, lk_coef k,
                                                           const double* __restrict__ mpow, lv_span s, lvr_rows rw) {
    __shared__ float tile[LK_T * LK_LDSW];
    __shared__ double sc[LK_T][4];
    __shared__ double rs[LK_T];
    const int c = threadIdx.x, S = s.S;
    const int ch = blockIdx.y;
    const long long q = s.ne0 + blockIdx.x;
    const long long r0 = q > 2 ? (q - 2) * s.hop : 0;
    const long long len = (q + 1) * s.hop - r0;           // <= 3 hop <= LK_T S
    const long long qrel = q * s.hop - r0;                // quarter q is [qrel, len) of the region
    const float* xr = xw + (long long)ch * rw.w_stride + (r0 - s.g0);
    const bool vec = (reinterpret_cast<uintptr_t>(xr) & 15u) == 0;    // (uniform; the values do not depend on it)
    float st[4] = {0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < S / LK_P; ++p) {
        __syncthreads();
        if (vec) lk_stage<true>(xr, 0, S, p, len, tile); else lk_stage<false>(xr, 0, S, p, len, tile);
        __syncthreads();
#pragma unroll 8
        for (int i = 0; i < LK_P; ++i) lk_step(k, tile[c * LK_LDSW + i], st);
    }
    // inclusive scan of the end states: after step i, v_c = sum_{j in (c - 2^(i+1), c]} M^(c-j) e_j
    double v[4] = {st[0], st[1], st[2], st[3]};
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
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) st[e] = c == 0 ? 0.f : (float)sc[c - 1][e];
    const long long cs = (long long)c * S;
    const bool active = cs + S > qrel && cs < len;        // the chunk reaches into quarter q
    double acc = 0.0;
    for (int p = 0; p < S / LK_P; ++p) {
        __syncthreads();
        if (vec) lk_stage<true>(xr, 0, S, p, len, tile); else lk_stage<false>(xr, 0, S, p, len, tile);
        __syncthreads();
        if (active) {
            const long long i0 = cs + p * LK_P;
#pragma unroll 8
            for (int i = 0; i < LK_P; ++i) {
                const double y = lk_step(k, tile[c * LK_LDSW + i], st);
                const long long pos = i0 + i;
                if (pos >= qrel && pos < len) acc = fma(y, y, acc);
            }
        }
    }
    rs[c] = acc;
    __syncthreads();
    for (int h = LK_T / 2; h > 0; h >>= 1) {              // (a fixed order)
        if (c < h) rs[c] += rs[c + h];
        __syncthreads();
    }
    if (c == 0) rw.ewc[(long long)ch * rw.eslots + blockIdx.x] = rs[0];
}

__global__ __launch_bounds__(LK_T) void lvr_anchor_kernel(lv_span s, lvr_rows rw, double T, double max_gain, double gate,
                                                          double* __restrict__ state) {
    __shared__ double Gs[LK_T];
    __shared__ int ok[LK_T];
    const int l = threadIdx.x;
    // the linked energies of the new quarters, before anything else reads them
    for (long long j = l; j < s.ne1 - s.ne0; j += LK_T) {
        double E = 0.0;
#pragma unroll
        for (int ch = 0; ch < LVR_CMAX; ++ch)             // (unrolled: the weights are kernel arguments and stay in scalar registers)
            if (ch < rw.C) E = __dadd_rn(E, __dmul_rn(rw.w[ch], rw.ewc[(long long)ch * rw.eslots + j]));
        s.ews[j] = E;
    }
    __syncthreads();
    const bool fresh = s.m0 == 0;
    // what lane 0 carries
    double Gc = 0.0, gmin = INFINITY, gmax = -INFINITY, cnt = 0.0, gated = 0.0, fault = 0.0;
    if (l == 0 && !fresh) {
        gmin = state[0]; gmax = state[1]; cnt = state[2]; gated = state[3]; Gc = state[4]; fault = state[6];
        if (cnt != (double)s.na0 || state[5] != (double)s.ne0) fault = 1.0;
    }
    // the anchors before na0 that this span's outputs read (at most two)
    for (long long q = s.qa0 + l; q < s.na0; q += LK_T) s.aws[q - s.qa0] = (float)state[8 + (q & 3)];
    __syncthreads();                                      // (the state's anchor slots are read: they may be written)
    for (long long base = s.na0; base < s.na1; base += LK_T) {
        const long long q = base + l;
        if (q < s.na1) {
            const long long j0 = q > LV_BEHIND ? q - LV_BEHIND : 0;
            const long long j1 = s.Q - LV_AHEAD < q ? s.Q : q + LV_AHEAD;
            double sum = 0.0;
            for (long long j = j0; j < j1; ++j) {             // (both indices are valid whichever value is taken)
                const double en = s.ews[j >= s.ne0 ? j - s.ne0 : 0], er = state[16 + (j & (LV_RING - 1))];
                sum += j >= s.ne0 ? en : er;
            }
            double G = 0.0;
            int valid = 0;
            if (j1 > j0 && sum > 0.0) {
                const double lq = -0.691 + 10.0 * log10(sum / ((double)(j1 - j0) * (double)s.hop));
                valid = lq > gate;
                G = fmin(fmax(T - lq, -LV_MAX_CUT), max_gain);
            }
            Gs[l] = G;
            ok[l] = valid;
        }
        __syncthreads();
        if (l == 0) {
            const long long m = s.na1 - base < LK_T ? s.na1 - base : LK_T;
            for (int i = 0; i < (int)m; ++i) {            // the hold, in index order
                if (ok[i]) Gc = Gs[i];
                else { Gs[i] = Gc; gated += 1.0; }
                gmin = fmin(gmin, Gc);
                gmax = fmax(gmax, Gc);
            }
            cnt += (double)m;
        }
        __syncthreads();
        if (q < s.na1) {
            const float a = (float)pow(10.0, Gs[l] / 20.0);
            s.aws[q - s.qa0] = a;
            if (q >= s.na1 - 4) state[8 + (q & 3)] = (double)a;
        }
        __syncthreads();
    }
    // every read of the energy ring is behind us: the last LV_RING energies go in
    for (long long j = (s.ne1 - LV_RING > s.ne0 ? s.ne1 - LV_RING : s.ne0) + l; j < s.ne1; j += LK_T)
        state[16 + (j & (LV_RING - 1))] = s.ews[j - s.ne0];
    if (l == 0) {
        state[0] = gmin; state[1] = gmax; state[2] = cnt; state[3] = gated; state[4] = Gc;
        state[5] = (double)s.ne1; state[6] = fault; state[7] = 0.0;
    }
}

__global__ __launch_bounds__(LK_T) void lvr_apply_kernel(const float* __restrict__ xw, lv_span s, long long w_stride,
                                                         long long out_stride, float* __restrict__ out) {
    const long long t0 = s.m0 + ((long long)blockIdx.x * LK_T + threadIdx.x) * 4;
    if (t0 >= s.m1) return;
    const bool full = t0 + 3 < s.m1;
    const float* xc = xw + (long long)blockIdx.y * w_stride + (s.m0 - s.g0);      // this channel's sample m0
    float* oc = out + (long long)blockIdx.y * out_stride;
    const bool vx = (reinterpret_cast<uintptr_t>(xc) & 15u) == 0, vo = (reinterpret_cast<uintptr_t>(oc) & 15u) == 0;     // (uniform)
    const float* xp = xc + (t0 - s.m0);
    float* op = oc + (t0 - s.m0);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (vx && full) {
        const float4 u = *reinterpret_cast<const float4*>(xp);
        v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (t0 + e < s.m1) v[e] = xp[e];
    }
    long long q = t0 / s.hop;
    int r = (int)(t0 - q * s.hop);
    const float fh = (float)s.hop;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float g;
        if (q >= s.Q) {
            g = s.aws[s.qt];                              // behind the last complete quarter (qt: a host argument, inside aws)
        } else {
            const float a0 = s.aws[q - s.qa0], a1 = s.aws[q + 1 - s.qa0];
            g = __fadd_rn(a0, __fmul_rn(__fsub_rn(a1, a0), __fdiv_rn((float)r, fh)));     // (this order is the definition)
        }
        v[e] = __fmul_rn(v[e], g);
        if (++r == s.hop) { r = 0; ++q; }
    }
    if (vo && full) {
        *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (t0 + e < s.m1) op[e] = v[e];
    }
}

extern "C" size_t vfx_level_span_rows_workspace_bytes(int64_t n_span, int hop, int C) {
    if (n_span < 0 || n_span > LV_SPAN_MAX || hop < 400 || hop > 19200 || C < 1 || C > LVR_CMAX) return 0;
    size_t total = 0;
    lvr_layout(n_span, hop, C, &total, nullptr, nullptr, nullptr);
    return total;
}

extern "C" int vfx_level_span_rows_f32(const float* xw, int64_t w_stride, int C, const double* weight, int64_t g0, int64_t wlen,
                                       int64_t n_total, int64_t m0, int64_t m1, int fs, const double* coef, const double* mpow, int S,
                                       double target, double max_gain_db, double gate, double* state, float* out, int64_t out_stride,
                                       void* ws, size_t ws_bytes, vfx_stream_t stream) {
    if (!xw || !out || !state || !ws || !coef || !mpow || !weight || g0 < 0 || wlen < 0 || n_total < 0 || m0 < 0 || m1 < m0 ||
        m1 > n_total)
        return VFX_EINVAL;
    if (fs < 4000 || fs > 192000 || g0 > INT64_MAX - wlen || m1 - m0 > LV_SPAN_MAX) return VFX_EINVAL;
    if (C < 1 || C > LVR_CMAX || w_stride < wlen || out_stride < m1 - m0 || w_stride > (INT64_MAX >> 6) || out_stride > (INT64_MAX >> 6))
        return VFX_EINVAL;
    const int hop = (fs + 5) / 10;
    if (S != lv_chunk(hop)) return VFX_EINVAL;
    if (!(target >= -70.0 && target < 0.0) || !(max_gain_db >= 0.0 && max_gain_db <= 40.0) || !(gate >= -70.0 && gate < target))
        return VFX_EINVAL;
    for (int i = 0; i < 10; ++i)
        if (!std::isfinite(coef[i])) return VFX_EINVAL;
    lvr_rows rw = {};
    for (int i = 0; i < C; ++i) {
        if (!std::isfinite(weight[i]) || !(weight[i] >= 0.0)) return VFX_EINVAL;
        rw.w[i] = weight[i];
    }
    const bool known = n_total != INT64_MAX;
    const long long nk = g0 + wlen;                       // the samples seen so far
    if (!known) {
        const long long ready = nk / hop > LV_AHEAD ? (nk / hop - LV_AHEAD) * hop : 0;
        if (m1 > ready) return VFX_EINVAL;
    }
    size_t need = 0;
    lv_span s = {};
    lvr_layout(m1 - m0, hop, C, &need, &s, &rw, (char*)ws);
    if (ws_bytes < need || ((uintptr_t)ws & 15u) || ((uintptr_t)state & 7u)) return VFX_EINVAL;
    {   // the block of the outputs may not overlap the block of the windows
        const uintptr_t xb = (uintptr_t)xw, xe = (uintptr_t)(xw + (C - 1) * w_stride + wlen);
        const uintptr_t ob = (uintptr_t)out, oe = (uintptr_t)(out + (C - 1) * out_stride + (m1 - m0));
        if (!(xe <= ob || oe <= xb)) return VFX_EINVAL;
    }
    if (m0 == m1) return VFX_OK;
    const long long Q = known ? n_total / hop : LLONG_MAX;
    auto na = [&](long long m) { return m == 0 ? 0LL : ((m - 1) / hop + 1 < Q ? (m - 1) / hop + 1 : Q) + 1; };
    auto ne = [&](long long m) { return m == 0 ? 0LL : (na(m) + LV_AHEAD - 1 < Q ? na(m) + LV_AHEAD - 1 : Q); };
    s.g0 = g0;
    s.m0 = m0;
    s.m1 = m1;
    s.Q = Q;
    s.hop = hop;
    s.S = S;
    s.ne0 = ne(m0);
    s.ne1 = ne(m1);
    s.na0 = na(m0);
    s.na1 = na(m1);
    s.qa0 = m0 / hop < Q ? m0 / hop : Q;
    s.qt = known && Q < s.na1 ? Q - s.qa0 : 0;            // (Q >= qa0 always; Q < na1: anchor Q is among this span's)
    {   // every channel's window covers what is read: the outputs' own samples and the regions of the new quarters
        long long lo = m0, hi = m1;
        if (s.ne1 > s.ne0) {
            const long long r0 = s.ne0 > 2 ? (s.ne0 - 2) * hop : 0;
            lo = r0 < lo ? r0 : lo;
            hi = s.ne1 * hop > hi ? s.ne1 * hop : hi;
        }
        if (lo < g0 || hi > nk) return VFX_EINVAL;
    }
    rw.w_stride = w_stride;
    rw.out_stride = out_stride;
    rw.C = C;
    lk_coef k;
    k.b0s = (float)coef[0]; k.b1s = (float)coef[1]; k.b2s = (float)coef[2]; k.a1s = (float)coef[3]; k.a2s = (float)coef[4];
    k.b0h = (float)coef[5]; k.b1h = (float)coef[6]; k.b2h = (float)coef[7]; k.a1h = (float)coef[8]; k.a2h = (float)coef[9];
    hipStream_t st = (hipStream_t)stream;
    if (s.ne1 > s.ne0) {
        hipLaunchKernelGGL(lvr_quarter_kernel, dim3((unsigned)(s.ne1 - s.ne0), (unsigned)C), dim3(LK_T), 0, st, xw, k, mpow, s, rw);
        VFX_LAUNCHED();
    }
    hipLaunchKernelGGL(lvr_anchor_kernel, dim3(1), dim3(LK_T), 0, st, s, rw, target, max_gain_db, gate, state);
    VFX_LAUNCHED();
    const long long nblk = (m1 - m0 + 4LL * LK_T - 1) / (4LL * LK_T);
    hipLaunchKernelGGL(lvr_apply_kernel, dim3((unsigned)nblk, (unsigned)C), dim3(LK_T), 0, st, xw, s, (long long)w_stride,
                       (long long)out_stride, out);
    VFX_LAUNCHED();
    return vfx_last_error();
}
