// vfx_meter_span.inc -- the streaming loudness meter of a session, carried across blocks (vfx_meter_span_rows_f32,
// vfx_meter_report_f32; definition, ready rule and measured cost: DESIGN.md 3.19, voicefixer_amd/loudness.py).  Included by
// vfx_loudness.hip behind vfx_level_span.inc: the quarter energies are lv_quarter_kernel's, the interpolated values
// tp_tile_sums', the order statistics lk_select's -- the meter adds the span form that carries them, and the report.
//
// Per programme x_c[0..N) at fs, C = 1..8 channels with the weights w, hop = (fs + 5) / 10.  A call folds the samples [m0, m1)
// into the caller's state and log; calls come in order (m0 of a call is m1 of the one before, the first m0 is 0), so what a
// call finds follows from m0 alone: after [0, m) the quarters [0, nq(m)), nq(m) = m / hop, are in qlog,
//     qlog[q] = sum_c w_c E_{q,c}      (fp64, c ascending from 0.0, every product and every sum rounded on its own),
// E_{q,c} the leveller's quarter energy (vfx_level_span.inc), and the state holds the peaks over [0, m):
//     P  = max_c max |x_c[n]|, n < m;      TP = max(P, max |y_c[k]| over the interpolated values k that BELONG to a sample n < m)
// -- value (K, p) of tp_tile_sums belongs to sample n = K - c / R, reads x[n - Bk .. n + Fw], and lies in the row iff
// ls_env_kernel's lo_ok and hi_ok hold; the values of n = N (behind the last sample) are folded by the call with m1 = N once N
// is known.  Every value is a function of GLOBAL positions and every fold is a maximum, so state and log have the bits of one
// call over the whole row whatever the split, the window or g0.  While the end is unknown m1 <= n_known - Fw.
//   1. lv_quarter_kernel (as it is): grid (nq(m1) - nq(m0), C), E_{q,c} into the workspace.
//   2. mt_peak_kernel<R> (R = 2, 4; mt_peak1_kernel at R = 1): a workgroup owns a tile of the whole-row anchoring (K0 = Kal +
//      tile TP_TILE) and walks the channels; |x| and |y| are folded with fmaxf in registers, then over the lanes: one float2
//      {max |x|, max |y|} per tile.  Nothing per sample is stored.
//   3. mt_fold_kernel: one workgroup: the weighted sums of the new quarters into qlog, the partials into the state.
// At most three launches per call, no float atomics, nothing waits for the host.
//
// state (device float64[VFX_METER_STATE], the caller's, one per programme; a call with m0 == 0 initialises it; all zeros is
// the state of a programme nothing of which has been metered):
//   [0] P  [1] TP  [2] quarters logged  [3] samples metered  [4] 1 once a call came out of order (sticky)  [5..16) 0
#define MT_STATE 16
#define MT_SPAN_MAX (1LL << 30)   // samples per call
#define MT_CMAX 8

struct mt_span {
    long long g0, wl, wh;         // the window's origin; window and row intersect in [wl, wh) (global)
    long long n;                  // n_total (INT64_MAX: unknown)
    long long m0, m1;
    long long tlo, nt;            // first peak tile (global index at R > 1; at R = 1 tile t starts at m0 + t TP_TILE), how many
    long long nq0, nq1;           // new quarters
    long long w_stride, eslots;
    int known, tail;              // n is the row's length; this call folds the values behind the last sample (R > 1)
    int C;
    double w[MT_CMAX];            // the channel weights: host doubles, copied into the kernel arguments
    double* ewc;                  // [C][eslots]: E_{q,c} of the new quarters
    float2* part;                 // [nt]: {max |x|, max |y|} of every tile
};

static void mt_layout(long long n_span, int hop, int C, size_t* total, mt_span* s, char* base) {
    const long long nq = n_span / hop + 2;                // (new quarters of a span: at most n_span / hop + 1)
    const long long nt = n_span / TP_TILE + 3;            // (any anchoring of the tiles, and the tail's)
    size_t off = 0;
    const size_t o_e = off; off += lk_round((size_t)C * (size_t)nq * sizeof(double));
    const size_t o_p = off; off += lk_round((size_t)nt * sizeof(float2));
    *total = off;
    if (s) {
        s->ewc = (double*)(base + o_e);
        s->part = (float2*)(base + o_p);
        s->eslots = nq;
    }
}

// max over the workgroup of two values at once (exact: no order to fix); lane 0 holds the result
__device__ __forceinline__ void mt_max2(float& a, float& b, float* ra, float* rb) {
    const int l = threadIdx.x;
    ra[l] = a;
    rb[l] = b;
    __syncthreads();
    for (int h = TP_T / 2; h > 0; h >>= 1) {
        if (l < h) {
            ra[l] = fmaxf(ra[l], ra[l + h]);
            rb[l] = fmaxf(rb[l], rb[l + h]);
        }
        __syncthreads();
    }
    a = ra[0];
    b = rb[0];
}

// Tile blockIdx.x holds K in [K0, K0 + TP_TILE), K0 = Kal + (tlo + blockIdx.x) TP_TILE: the whole-row kernel's anchoring, the row
// pointer and the tile origin both moved by g0 as in ls_env_kernel, so every chain has the order of lk_truepeak_kernel.  Sample
// n = K - c / R collects |x[n]| and its R interpolated values; lo_ok / hi_ok: ls_env_kernel's clipping against [0, n_total).
template <int R>
__global__ __launch_bounds__(TP_T) void mt_peak_kernel(const float* __restrict__ xw, const float* __restrict__ bank, int J, int Jp,
                                                       int c, long long Kal, mt_span s) {
    extern __shared__ float4 tp_lds[];
    const int l = threadIdx.x;
    const int q = c / R, rem = c - q * R;
    const long long K0 = Kal + (s.tlo + (long long)blockIdx.x) * TP_TILE;
    const long long nb = K0 + TP_KPL * l - q;             // the sample of this lane's first K
    float px = 0.f, py = 0.f;
    for (int ch = 0; ch < s.C; ++ch) {
        const float* xc = xw + (long long)ch * s.w_stride;
#pragma unroll
        for (int k = 0; k < TP_KPL; ++k) {
            const long long nn = nb + k;
            if (nn >= s.m0 && nn < s.m1) px = fmaxf(px, fabsf(xc[nn - s.g0]));
        }
        float aa[R][TP_KPL], ab[R][TP_KPL];
        const bool vec = ((((uintptr_t)xc >> 2) - (uintptr_t)s.g0) & 3u) == 0;      // (uniform; the values do not depend on it)
        if (vec) tp_tile_sums<R, true>(xc, s.wh - s.g0, bank, J, Jp, K0 - s.g0, tp_lds, aa, ab);
        else tp_tile_sums<R, false>(xc, s.wh - s.g0, bank, J, Jp, K0 - s.g0, tp_lds, aa, ab);
#pragma unroll
        for (int k = 0; k < TP_KPL; ++k) {
            const long long nn = nb + k;
            const bool mine = (nn >= s.m0 && nn < s.m1) || (s.tail && nn == s.n);
#pragma unroll
            for (int p = 0; p < R; ++p) {
                const bool lo_ok = nn > 0 || (nn == 0 && p >= rem);
                const bool hi_ok = !s.known || nn < s.n || (nn == s.n && p < rem);
                if (mine && lo_ok && hi_ok) py = fmaxf(py, fabsf(aa[p][k] + ab[p][k]));
            }
        }
        __syncthreads();                                  // (the staged tile is read: the next channel, or the tree, may write)
    }
    float* red = reinterpret_cast<float*>(tp_lds);        // [2 TP_T]
    mt_max2(px, py, red, red + TP_T);
    if (l == 0) s.part[blockIdx.x] = make_float2(px, py);
}

// R = 1: nothing is interpolated; tile t holds the samples from m0 + t TP_TILE.
__global__ __launch_bounds__(TP_T) void mt_peak1_kernel(const float* __restrict__ xw, mt_span s) {
    __shared__ float red[2 * TP_T];
    const int l = threadIdx.x;
    const long long n0 = s.m0 + (long long)blockIdx.x * TP_TILE;
    float px = 0.f, py = 0.f;
#pragma unroll
    for (int k = 0; k < TP_KPL; ++k) {
        const long long nn = n0 + l + k * TP_T;
        if (nn < s.m1)
            for (int ch = 0; ch < s.C; ++ch) px = fmaxf(px, fabsf(xw[(long long)ch * s.w_stride + (nn - s.g0)]));
    }
    mt_max2(px, py, red, red + TP_T);
    if (l == 0) s.part[blockIdx.x] = make_float2(px, px);
}

__global__ __launch_bounds__(LK_T) void mt_fold_kernel(mt_span s, double* __restrict__ state, double* __restrict__ qlog) {
    __shared__ float red[2 * LK_T];
    const int l = threadIdx.x;
    for (long long j = l; j < s.nq1 - s.nq0; j += LK_T) {
        double E = 0.0;
#pragma unroll
        for (int ch = 0; ch < MT_CMAX; ++ch)              // (unrolled: the weights are kernel arguments and stay in scalar registers)
            if (ch < s.C) E = __dadd_rn(E, __dmul_rn(s.w[ch], s.ewc[(long long)ch * s.eslots + j]));
        qlog[s.nq0 + j] = E;
    }
    float px = 0.f, py = 0.f;
    for (long long j = l; j < s.nt; j += LK_T) {
        const float2 v = s.part[j];
        px = fmaxf(px, v.x);
        py = fmaxf(py, v.y);
    }
    mt_max2(px, py, red, red + LK_T);
    if (l == 0) {
        double P = 0.0, TP = 0.0, fault = 0.0;
        if (s.m0 != 0) {
            P = state[0]; TP = state[1]; fault = state[4];
            if (state[2] != (double)s.nq0 || state[3] != (double)s.m0) fault = 1.0;
        } else {
            for (int i = 5; i < MT_STATE; ++i) state[i] = 0.0;
        }
        state[0] = fmax(P, (double)px);
        state[1] = fmax(TP, (double)fmaxf(px, py));
        state[2] = (double)s.nq1;
        state[3] = (double)s.m1;
        state[4] = fault;
    }
}

extern "C" size_t vfx_meter_span_workspace_bytes(int64_t n_span, int hop, int C) {
    if (n_span < 0 || n_span > MT_SPAN_MAX || hop < 400 || hop > 19200 || C < 1 || C > MT_CMAX) return 0;
    size_t total = 0;
    mt_layout(n_span, hop, C, &total, nullptr, nullptr);
    return total;
}

extern "C" int vfx_meter_span_rows_f32(const float* xw, int64_t w_stride, int C, const double* weight, int64_t g0, int64_t wlen,
                                       int64_t n_total, int64_t m0, int64_t m1, int fs, const double* coef, const double* mpow, int S,
                                       const float* bank, int J, int R, int c, double* state, double* qlog, int64_t qcap, void* ws,
                                       size_t ws_bytes, vfx_stream_t stream) {
    if (!xw || !state || !qlog || !ws || !coef || !mpow || !weight || g0 < 0 || wlen < 0 || n_total < 0 || m0 < 0 || m1 < m0 ||
        m1 > n_total || qcap < 0)
        return VFX_EINVAL;
    if (fs < 4000 || fs > 192000 || g0 > INT64_MAX - wlen || m1 - m0 > MT_SPAN_MAX) return VFX_EINVAL;
    if (C < 1 || C > MT_CMAX || w_stride < wlen || w_stride > (INT64_MAX >> 6)) return VFX_EINVAL;
    if (R != 1 && R != 2 && R != 4) return VFX_EINVAL;
    if (R > 1 && (!bank || J < 1 || J > TP_JMAX || c < 0 || (long long)c >= (long long)R * J)) return VFX_EINVAL;
    const int hop = (fs + 5) / 10;
    if (S != lv_chunk(hop)) return VFX_EINVAL;
    for (int i = 0; i < 10; ++i)
        if (!std::isfinite(coef[i])) return VFX_EINVAL;
    mt_span s = {};
    for (int i = 0; i < C; ++i) {
        if (!std::isfinite(weight[i]) || !(weight[i] >= 0.0)) return VFX_EINVAL;
        s.w[i] = weight[i];
    }
    const bool known = n_total != INT64_MAX;
    const long long nk = g0 + wlen;                       // the samples seen so far
    const long long q = R > 1 ? c / R : 0;
    const long long Fw = q, Bk = R > 1 ? (long long)J - 1 - q : 0;
    if (!known && m1 > (nk > Fw ? nk - Fw : 0)) return VFX_EINVAL;
    s.nq0 = m0 / hop;
    s.nq1 = m1 / hop;
    if (s.nq1 > qcap) return VFX_EINVAL;
    size_t need = 0;
    mt_layout(m1 - m0, hop, C, &need, &s, (char*)ws);
    if (ws_bytes < need || ((uintptr_t)ws & 15u) || ((uintptr_t)state & 7u) || ((uintptr_t)qlog & 7u)) return VFX_EINVAL;
    if (m0 == m1) return VFX_OK;
    {   // every channel's window covers what is read: what the peaks of [m0, m1) read and the regions of the new quarters
        long long lo = m0 > Bk ? m0 - Bk : 0;
        long long hi = n_total - m1 > Fw ? m1 - 1 + Fw : n_total - 1;
        if (s.nq1 > s.nq0) {
            const long long r0 = s.nq0 > 2 ? (s.nq0 - 2) * hop : 0;
            lo = r0 < lo ? r0 : lo;
            hi = s.nq1 * hop - 1 > hi ? s.nq1 * hop - 1 : hi;
        }
        if (lo < g0 || hi >= nk) return VFX_EINVAL;
    }
    s.g0 = g0;
    s.n = n_total;
    s.m0 = m0;
    s.m1 = m1;
    s.known = known;
    s.C = C;
    s.w_stride = w_stride;
    s.wl = g0;
    s.wh = n_total - g0 < wlen ? n_total : nk;
    s.tail = R > 1 && known && m1 == n_total;
    hipStream_t st = (hipStream_t)stream;
    if (s.nq1 > s.nq0) {
        lv_span v = {};                                   // what lv_quarter_kernel reads of it
        v.g0 = g0;
        v.ne0 = s.nq0;
        v.hop = hop;
        v.S = S;
        v.C = C;
        v.w_stride = w_stride;
        v.eslots = s.eslots;
        v.ewc = s.ewc;
        lk_coef k;
        k.b0s = (float)coef[0]; k.b1s = (float)coef[1]; k.b2s = (float)coef[2]; k.a1s = (float)coef[3]; k.a2s = (float)coef[4];
        k.b0h = (float)coef[5]; k.b1h = (float)coef[6]; k.b2h = (float)coef[7]; k.a1h = (float)coef[8]; k.a2h = (float)coef[9];
        hipLaunchKernelGGL(lv_quarter_kernel, dim3((unsigned)(s.nq1 - s.nq0), (unsigned)C), dim3(LK_T), 0, st, xw, k, mpow, v);
        VFX_LAUNCHED();
    }
    if (R > 1) {
        const long long Kal = tp_kal(c, R);
        const long long off = q - Kal;                    // (>= 0)
        s.tlo = (m0 + off) / TP_TILE;
        s.nt = ((s.tail ? n_total : m1 - 1) + off) / TP_TILE - s.tlo + 1;
        const int Jp = tp_jp(J);
        const size_t tp_bytes = (size_t)(TP_TILE + Jp + R * Jp) * sizeof(float);          // (>= the tree's 2 TP_T floats)
        const dim3 gt((unsigned)s.nt);
        if (R == 4) hipLaunchKernelGGL((mt_peak_kernel<4>), gt, dim3(TP_T), tp_bytes, st, xw, bank, J, Jp, c, Kal, s);
        else hipLaunchKernelGGL((mt_peak_kernel<2>), gt, dim3(TP_T), tp_bytes, st, xw, bank, J, Jp, c, Kal, s);
    } else {
        s.tlo = 0;
        s.nt = (m1 - m0 + TP_TILE - 1) / TP_TILE;
        hipLaunchKernelGGL(mt_peak1_kernel, dim3((unsigned)s.nt), dim3(TP_T), 0, st, xw, s);
    }
    VFX_LAUNCHED();
    hipLaunchKernelGGL(mt_fold_kernel, dim3(1), dim3(LK_T), 0, st, s, state, qlog);
    VFX_LAUNCHED();
    return vfx_last_error();
}

// ---- the report over the carried state ---------------------------------------------------------------------------------------
// One workgroup: report = {L, LRA, Mmax, Smax, P, TP, M_last, S_last, quarters, flag} from qlog[0..quarters), the recipe of
// lk_gate_kernel / lk_report_kernel on these quarter sums: z_j = (q_j + q_{j+1} + q_{j+2} + q_{j+3}) / (4 hop) (left to right),
// both gates over the z_j in fixed-order workgroup sums, the short-term energies e_j = (ascending sum of 30 quarters) / (30 hop)
// into st, the two order statistics of the gated e_j by counting over their bit patterns (lk_select).  The log is read from
// memory: an hour is 36000 quarters, which LDS does not hold.  Reads state and qlog only.  flag: the state's, or 2 where the
// state's quarter count does not fit st (the figures are then those of no quarters).
__device__ __forceinline__ double mt_max(double v, double* rs) {
    const int c = threadIdx.x;
    rs[c] = v;
    __syncthreads();
    for (int h = LK_T / 2; h > 0; h >>= 1) {
        if (c < h) rs[c] = fmax(rs[c], rs[c + h]);
        __syncthreads();
    }
    v = rs[0];
    __syncthreads();
    return v;
}

__global__ __launch_bounds__(LK_T) void mt_report_kernel(const double* __restrict__ state, const double* __restrict__ q, int hop,
                                                         long long cap, double* __restrict__ report, double* __restrict__ e) {
    __shared__ double rs[LK_T];
    __shared__ long long rc[LK_T];
    const int c = threadIdx.x;
    const double vq = state[2];
    const bool fits = vq >= 0.0 && vq <= (double)cap;
    const long long nq = fits ? (long long)vq : 0;
    const long long nblk = nq > 3 ? nq - 3 : 0;
    const long long nst = nq >= LK_ST ? nq - LK_ST + 1 : 0;
    unsigned long long* key = reinterpret_cast<unsigned long long*>(e);
    const double inv4 = 1.0 / (4.0 * hop), inv = 1.0 / ((double)LK_ST * hop);
    double zm = -1.0, s1 = 0.0;                           // (max is exact: any order gives the same bits)
    long long c1 = 0;
    for (long long j = c; j < nblk; j += LK_T) {
        const double zj = (q[j] + q[j + 1] + q[j + 2] + q[j + 3]) * inv4;
        zm = fmax(zm, zj);
        if (-0.691 + 10.0 * log10(zj) > -70.0) { s1 += zj; ++c1; }
    }
    zm = mt_max(zm, rs);
    lk_reduce(s1, c1, rs, rc);
    double L = -INFINITY;
    if (c1 > 0) {
        const double gr = -0.691 + 10.0 * log10(s1 / (double)c1) - 10.0;
        double s2 = 0.0;
        long long c2 = 0;
        for (long long j = c; j < nblk; j += LK_T) {
            const double zj = (q[j] + q[j + 1] + q[j + 2] + q[j + 3]) * inv4;
            const double l = -0.691 + 10.0 * log10(zj);
            if (l > -70.0 && l > gr) { s2 += zj; ++c2; }
        }
        lk_reduce(s2, c2, rs, rc);
        if (c2 > 0) L = -0.691 + 10.0 * log10(s2 / (double)c2);
    }
    double em = -1.0;
    s1 = 0.0;
    c1 = 0;
    for (long long j = c; j < nst; j += LK_T) {
        double a = 0.0;
        for (int i = 0; i < LK_ST; ++i) a += q[j + i];    // (fixed order)
        a *= inv;
        e[j] = a;
        em = fmax(em, a);
        if (-0.691 + 10.0 * log10(a) > -70.0) { s1 += a; ++c1; }
    }
    em = mt_max(em, rs);
    lk_reduce(s1, c1, rs, rc);
    double lra = 0.0;
    if (c1 > 0) {
        const double gr = -0.691 + 10.0 * log10(s1 / (double)c1) - 20.0;
        long long c2 = 0;
        double zero = 0.0;
        for (long long j = c; j < nst; j += LK_T) {      // (each lane rewrites only the entries it wrote itself)
            const double a = e[j];
            const double lj = -0.691 + 10.0 * log10(a);
            const bool keep = lj > -70.0 && lj > gr;
            key[j] = keep ? (unsigned long long)__double_as_longlong(a) : ~0ULL;
            c2 += keep;
        }
        lk_reduce(zero, c2, rs, rc);                      // (also orders the key writes before the counting reads)
        if (c2 > 0) {
            const double lo = __longlong_as_double((long long)lk_select(key, nst, (c2 - 1 + 5) / 10, rc));
            const double hi = __longlong_as_double((long long)lk_select(key, nst, ((c2 - 1) * 95 + 50) / 100, rc));
            lra = (-0.691 + 10.0 * log10(hi)) - (-0.691 + 10.0 * log10(lo));
        }
    }
    if (c == 0) {
        double ml = -INFINITY, sl = -INFINITY;
        if (nq >= 4) ml = -0.691 + 10.0 * log10((q[nq - 4] + q[nq - 3] + q[nq - 2] + q[nq - 1]) * inv4);
        if (nq >= LK_ST) {
            double a = 0.0;
            for (int i = 0; i < LK_ST; ++i) a += q[nq - LK_ST + i];
            sl = -0.691 + 10.0 * log10(a * inv);
        }
        report[0] = L;
        report[1] = lra;
        report[2] = zm >= 0.0 ? -0.691 + 10.0 * log10(zm) : -INFINITY;
        report[3] = em >= 0.0 ? -0.691 + 10.0 * log10(em) : -INFINITY;
        report[4] = state[0];
        report[5] = state[1];
        report[6] = ml;
        report[7] = sl;
        report[8] = (double)nq;
        report[9] = !fits ? 2.0 : (state[4] != 0.0 ? 1.0 : 0.0);
    }
}

extern "C" size_t vfx_meter_report_workspace_bytes(int64_t quarters) {
    if (quarters < 0 || quarters > (INT64_MAX >> 4)) return 0;
    return (size_t)(quarters > 0 ? quarters : 1) * sizeof(double);       // (exact: ws_bytes / 8 is also how far the kernel trusts state[2])
}

extern "C" int vfx_meter_report_f32(const double* state, const double* qlog, int hop, double* report, void* ws, size_t ws_bytes,
                                    vfx_stream_t stream) {
    if (!state || !qlog || !report || !ws || hop < 400 || hop > 19200) return VFX_EINVAL;
    if (((uintptr_t)state & 7u) || ((uintptr_t)qlog & 7u) || ((uintptr_t)report & 7u) || ((uintptr_t)ws & 7u)) return VFX_EINVAL;
    if (!(report + 10 <= state || state + MT_STATE <= report)) return VFX_EINVAL;
    hipLaunchKernelGGL(mt_report_kernel, dim3(1), dim3(LK_T), 0, (hipStream_t)stream, state, qlog, hop,
                       (long long)(ws_bytes / sizeof(double)), report, (double*)ws);
    VFX_LAUNCHED();
    return vfx_last_error();
}
