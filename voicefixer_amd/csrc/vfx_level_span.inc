// vfx_level_span.inc -- the streaming loudness leveller of a session, carried across blocks, for one row (vfx_level_span_f32;
// definition, ready rule and measured cost: DESIGN.md 3.17, voicefixer_amd/loudness.py) and LINKED over the C = 1..8 channels of
// a programme (vfx_level_span_rows_f32; DESIGN.md 3.18): one set of kernels, the row being the programme of one channel with the
// weight 1.  Included by vfx_loudness.hip behind vfx_limit_span.inc, whose K-weighting step, staging and matrix-vector product
// (lk_step, lk_stage, lk_mv) it shares.
//
// Per programme x_c[0..N) at fs, hop = (fs + 5) / 10, Q = N / hop complete quarters.  E_{q,c} is the K-weighted energy of quarter q
// of channel c with the filter started from ZERO at sample max(0, (q - 2) hop), and
//     E_q = sum_c w_c E_{q,c}      (fp64, c ascending from 0.0, every product and every sum rounded on its own),
// w the BS.1770-4 channel weights (C = 1, w = {1}: 0 + 1 E is exact).  Anchor q (at sample q hop) has the loudness l_q of the
// quarters [q - 20, q + 9] within [0, Q), the gain G_q = clamp(T - l_q, -40, max_gain) where l_q > gate and G_{q-1} otherwise
// (G_{-1} = 0), a_q = float(10^(G_q / 20)); out_c[t] = x_c[t] (a_q + (a_{q+1} - a_q) (float(t - q hop) / float(hop))) for t in
// quarter q < Q and x_c[t] a_Q behind the last complete quarter: one ramp multiplies every channel.  Channel ch's window is
// xw + ch w_stride, its outputs out + ch out_stride; g0, wlen, n_total and the state are the programme's.  Every value is a
// function of GLOBAL positions, so output t has the bits of one call over the whole row whatever the split.  Calls come in order
// (m0 of a call is m1 of the one before, the first m0 is 0), so what a call finds in the caller's state is a function of m0
// alone: after outputs [0, m) the anchors [0, na(m)) have been evaluated and the energies [0, ne(m)) computed,
//     na(m) = m == 0 ? 0 : min(Q, (m - 1) / hop + 1) + 1,      ne(m) = m == 0 ? 0 : min(Q, na(m) + 9)
// (no clipping against Q while the end is unknown: the ready rule keeps every window inside the complete quarters).
//   1. lv_quarter_kernel: one workgroup per (NEW quarter q in [ne(m0), ne(m1)), channel): grid (ne(m1) - ne(m0), C).  Its region
//      [r0, (q + 1) hop), r0 = max(0, (q - 2) hop), is cut from r0 into 256 chunks of S samples (S a function of fs: 256 S >= 3
//      hop); every lane filters its chunk from zero (fp32, staged through LDS 32 samples of every chunk at a time), a
//      Hillis-Steele scan (fp64, M^(2^i) of THIS S) gives every chunk its true start state, and the chunks that reach into
//      quarter q are filtered again from it: y^2 in fp64 per lane, a fixed tree over the lanes.  Nothing depends on where the
//      window starts or on the other quarters of the launch.  Writes E_{q,c} into channel c's slots of the workspace.
//   2. lv_anchor_kernel: one workgroup: first the weighted sums E_q of the new quarters, in the order above (one channel of
//      weight 1: none, E_q = 0 + 1 E_{q,0} exactly, and the host points the quarter kernel's slots at E_q); then z, l, G of the
//      anchors [na(m0), na(m1)) (a direct ascending fp64 sum per anchor, the energies before ne(m0) from the state's ring), the
//      hold in index order from the carried G, a, the record's folds; then the last 32 energies and the last 4 anchor gains go
//      back into the state.
//   3. lv_apply_kernel: out over [m0, m1), grid (blocks, C): four outputs per lane, 16-byte loads and stores where THIS channel's
//      addresses allow.
// At most three launches per call, whatever C; none of them waits for the host.
//
// state (device float64[VFX_LEVEL_STATE], owned by the caller, one per programme; a call with m0 == 0 initialises it):
//   [0] min G  [1] max G  [2] anchors evaluated  [3] anchors gated  [4] G of the last anchor (what the hold carries)
//   [5] energies computed (the ring holds the quarters [that - 32, that))  [6] 1 once a call came out of order (sticky)
//   [8 + q % 4] a_q of the last four anchors      [16 + j % 32] E_j of the last 32 quarters
#define LV_STATE 64
#define LV_RING 32
#define LV_BEHIND 20
#define LV_AHEAD 10
#define LV_MAX_CUT 40.0
#define LV_SPAN_MAX (1LL << 30)   // outputs per call
#define LV_CMAX 8

struct lv_span {
    long long g0, m0, m1;
    long long Q;                  // complete quarters of the row (LLONG_MAX: the end is unknown)
    long long ne0, ne1;           // new energies
    long long na0, na1;           // new anchors
    long long qa0;                // aws[0] is the gain of anchor qa0 = min(m0 / hop, Q)
    long long qt;                 // aws[qt] is a_Q where this span reaches behind the last complete quarter, else 0: the load is
                                  // uniform, the compiler issues it for every wave, and it has to stay inside aws for all of them
    long long w_stride, out_stride;
    long long eslots;             // energy slots per channel
    int hop, S, C;
    double w[LV_CMAX];            // the channel weights: host doubles, copied into the kernel arguments
    double* ews;                  // [ne1 - ne0]: E_q
    float* aws;                   // [na1 - qa0]
    double* ewc;                  // [C][eslots]: E_{q,c}
};

static void lv_layout(long long n_span, int hop, int C, size_t* total, lv_span* s, char* base) {
    const long long nq = n_span / hop;
    size_t off = 0;
    const size_t o_e = off; off += lk_round((size_t)(nq + 13) * sizeof(double));
    const size_t o_a = off; off += lk_round((size_t)(nq + 4) * sizeof(float));
    const size_t o_c = off; off += lk_round((size_t)C * (size_t)(nq + 13) * sizeof(double));
    *total = off;
    if (s) {
        s->ews = (double*)(base + o_e);
        s->aws = (float*)(base + o_a);
        s->ewc = (double*)(base + o_c);
        s->eslots = nq + 13;
    }
}

static inline int lv_chunk(int hop) { return 32 * (int)((3LL * hop + 32 * LK_T - 1) / (32 * LK_T)); }

__global__ __launch_bounds__(LK_T) void lv_quarter_kernel(const float* __restrict__ xw, lk_coef k,
                                                          const double* __restrict__ mpow, lv_span s) {
    __shared__ float tile[LK_T * LK_LDSW];
    __shared__ double sc[LK_T][4];
    __shared__ double rs[LK_T];
    const int c = threadIdx.x, S = s.S;
    const int ch = blockIdx.y;
    const long long q = s.ne0 + blockIdx.x;
    const long long r0 = q > 2 ? (q - 2) * s.hop : 0;
    const long long len = (q + 1) * s.hop - r0;           // <= 3 hop <= LK_T S
    const long long qrel = q * s.hop - r0;                // quarter q is [qrel, len) of the region
    const float* xr = xw + (long long)ch * s.w_stride + (r0 - s.g0);
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
    if (c == 0) s.ewc[(long long)ch * s.eslots + blockIdx.x] = rs[0];
}

__global__ __launch_bounds__(LK_T) void lv_anchor_kernel(lv_span s, double T, double max_gain, double gate,
                                                         double* __restrict__ state) {
    __shared__ double Gs[LK_T];
    __shared__ int ok[LK_T];
    const int l = threadIdx.x;
    if (s.ewc != s.ews) {         // (uniform) the linked energies of the new quarters, before anything else reads them
        for (long long j = l; j < s.ne1 - s.ne0; j += LK_T) {
            double E = 0.0;
#pragma unroll
            for (int ch = 0; ch < LV_CMAX; ++ch)          // (unrolled: the weights are kernel arguments and stay in scalar registers)
                if (ch < s.C) E = __dadd_rn(E, __dmul_rn(s.w[ch], s.ewc[(long long)ch * s.eslots + j]));
            s.ews[j] = E;
        }
        __syncthreads();
    }
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

__global__ __launch_bounds__(LK_T) void lv_apply_kernel(const float* __restrict__ xw, lv_span s, float* __restrict__ out) {
    const long long t0 = s.m0 + ((long long)blockIdx.x * LK_T + threadIdx.x) * 4;
    if (t0 >= s.m1) return;
    const bool full = t0 + 3 < s.m1;
    const float* xc = xw + (long long)blockIdx.y * s.w_stride + (s.m0 - s.g0);    // this channel's sample m0
    float* oc = out + (long long)blockIdx.y * s.out_stride;
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

// Validation, geometry and the launches of both entry points.  ``rows``: the linked entry, which also checks C and the strides
// and refuses an overlap of the blocks of windows and outputs BEFORE it accepts an empty span; the mono entry accepts the empty
// span first (each keeps the order it had as a file of its own).  Nothing is launched where anything is refused.
static int lv_run(bool rows, const float* xw, int64_t w_stride, int C, const double* weight, int64_t g0, int64_t wlen,
                  int64_t n_total, int64_t m0, int64_t m1, int fs, const double* coef, const double* mpow, int S, double target,
                  double max_gain_db, double gate, double* state, float* out, int64_t out_stride, void* ws, size_t ws_bytes,
                  vfx_stream_t stream) {
    if (!xw || !out || !state || !ws || !coef || !mpow || !weight || g0 < 0 || wlen < 0 || n_total < 0 || m0 < 0 || m1 < m0 ||
        m1 > n_total)
        return VFX_EINVAL;
    if (!rows) out_stride = m1 - m0;                      // (the one row: C = 1, w_stride = wlen, weight {1} from the entry point)
    if (fs < 4000 || fs > 192000 || g0 > INT64_MAX - wlen || m1 - m0 > LV_SPAN_MAX) return VFX_EINVAL;
    if (rows && (C < 1 || C > LV_CMAX || w_stride < wlen || out_stride < m1 - m0 || w_stride > (INT64_MAX >> 6) ||
                 out_stride > (INT64_MAX >> 6)))
        return VFX_EINVAL;
    const int hop = (fs + 5) / 10;
    if (S != lv_chunk(hop)) return VFX_EINVAL;
    if (!(target >= -70.0 && target < 0.0) || !(max_gain_db >= 0.0 && max_gain_db <= 40.0) || !(gate >= -70.0 && gate < target))
        return VFX_EINVAL;
    for (int i = 0; i < 10; ++i)
        if (!std::isfinite(coef[i])) return VFX_EINVAL;
    lv_span s = {};
    for (int i = 0; i < C; ++i) {
        if (!std::isfinite(weight[i]) || !(weight[i] >= 0.0)) return VFX_EINVAL;
        s.w[i] = weight[i];
    }
    const bool known = n_total != INT64_MAX;
    const long long nk = g0 + wlen;                       // the samples seen so far
    if (!known) {
        const long long ready = nk / hop > LV_AHEAD ? (nk / hop - LV_AHEAD) * hop : 0;
        if (m1 > ready) return VFX_EINVAL;
    }
    size_t need = 0;
    lv_layout(m1 - m0, hop, C, &need, &s, (char*)ws);
    if (ws_bytes < need || ((uintptr_t)ws & 15u) || ((uintptr_t)state & 7u)) return VFX_EINVAL;
    if (C == 1 && weight[0] == 1.0) s.ewc = s.ews;        // 0 + 1 E is E: the quarter kernel writes E_q itself, the anchor kernel sums nothing
    // the block of the outputs may not overlap the block of the windows
    const uintptr_t xb = (uintptr_t)xw, xe = (uintptr_t)(xw + (C - 1) * w_stride + wlen);
    const uintptr_t ob = (uintptr_t)out, oe = (uintptr_t)(out + (C - 1) * out_stride + (m1 - m0));
    const bool overlap = !(xe <= ob || oe <= xb);
    if (rows && overlap) return VFX_EINVAL;
    if (m0 == m1) return VFX_OK;
    if (overlap) return VFX_EINVAL;
    const long long Q = known ? n_total / hop : LLONG_MAX;
    auto na = [&](long long m) { return m == 0 ? 0LL : ((m - 1) / hop + 1 < Q ? (m - 1) / hop + 1 : Q) + 1; };
    auto ne = [&](long long m) { return m == 0 ? 0LL : (na(m) + LV_AHEAD - 1 < Q ? na(m) + LV_AHEAD - 1 : Q); };
    s.g0 = g0;
    s.m0 = m0;
    s.m1 = m1;
    s.Q = Q;
    s.hop = hop;
    s.S = S;
    s.C = C;
    s.w_stride = w_stride;
    s.out_stride = out_stride;
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
    lk_coef k;
    k.b0s = (float)coef[0]; k.b1s = (float)coef[1]; k.b2s = (float)coef[2]; k.a1s = (float)coef[3]; k.a2s = (float)coef[4];
    k.b0h = (float)coef[5]; k.b1h = (float)coef[6]; k.b2h = (float)coef[7]; k.a1h = (float)coef[8]; k.a2h = (float)coef[9];
    hipStream_t st = (hipStream_t)stream;
    if (s.ne1 > s.ne0) {
        hipLaunchKernelGGL(lv_quarter_kernel, dim3((unsigned)(s.ne1 - s.ne0), (unsigned)C), dim3(LK_T), 0, st, xw, k, mpow, s);
        VFX_LAUNCHED();
    }
    hipLaunchKernelGGL(lv_anchor_kernel, dim3(1), dim3(LK_T), 0, st, s, target, max_gain_db, gate, state);
    VFX_LAUNCHED();
    const long long nblk = (m1 - m0 + 4LL * LK_T - 1) / (4LL * LK_T);
    hipLaunchKernelGGL(lv_apply_kernel, dim3((unsigned)nblk, (unsigned)C), dim3(LK_T), 0, st, xw, s, out);
    VFX_LAUNCHED();
    return vfx_last_error();
}

extern "C" size_t vfx_level_span_rows_workspace_bytes(int64_t n_span, int hop, int C) {
    if (n_span < 0 || n_span > LV_SPAN_MAX || hop < 400 || hop > 19200 || C < 1 || C > LV_CMAX) return 0;
    size_t total = 0;
    lv_layout(n_span, hop, C, &total, nullptr, nullptr);
    return total;
}

extern "C" size_t vfx_level_span_workspace_bytes(int64_t n_span, int hop) { return vfx_level_span_rows_workspace_bytes(n_span, hop, 1); }

extern "C" int vfx_level_span_f32(const float* xw, int64_t g0, int64_t wlen, int64_t n_total, int64_t m0, int64_t m1, int fs,
                                  const double* coef, const double* mpow, int S, double target, double max_gain_db, double gate,
                                  double* state, float* out, void* ws, size_t ws_bytes, vfx_stream_t stream) {
    static const double one[1] = {1.0};
    return lv_run(false, xw, wlen, 1, one, g0, wlen, n_total, m0, m1, fs, coef, mpow, S, target, max_gain_db, gate, state, out,
                  0, ws, ws_bytes, stream);
}

extern "C" int vfx_level_span_rows_f32(const float* xw, int64_t w_stride, int C, const double* weight, int64_t g0, int64_t wlen,
                                       int64_t n_total, int64_t m0, int64_t m1, int fs, const double* coef, const double* mpow, int S,
                                       double target, double max_gain_db, double gate, double* state, float* out, int64_t out_stride,
                                       void* ws, size_t ws_bytes, vfx_stream_t stream) {
    return lv_run(true, xw, w_stride, C, weight, g0, wlen, n_total, m0, m1, fs, coef, mpow, S, target, max_gain_db, gate, state, out,
                  out_stride, ws, ws_bytes, stream);
}
