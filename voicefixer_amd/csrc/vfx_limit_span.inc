// vfx_limit_span.inc -- the fixed-gain look-ahead limiter of a streaming session, carried across blocks, for one row
// (vfx_limit_span_f32; DESIGN.md 3.16) and LINKED over the C = 1..8 channels of a programme (vfx_limit_span_rows_f32; DESIGN.md
// 3.18): one set of kernels, the row being the programme of one channel.  Included by vfx_loudness.hip behind vfx_limit.inc,
// whose tile sizes, reductions and true-peak sums it shares.
//
// F is steps 2-6 of the whole-row limiter (vfx_limit.inc) with a GIVEN gain gL: no measurement, no bound test, no trim.  F_C is
// F with ONE envelope for the C channels: e[n] = max_c e_c[n], then c, m and g from it, and out_c[n] = x_c[n] (float(gL) g[n]).
// The span form writes outputs [m0, m1) of F_C over rows of n_total samples from the windows xw[ch w_stride + k] = x_ch[g0 + k]
// to out[ch out_stride + n - m0]; g0, wlen and n_total are the programme's.  Every value is a function of GLOBAL positions:
// clipping and clamping are done against [0, n_total), never against the window, so output n has the bits the single span
// [0, n_total) gives it.  n_total = INT64_MAX: the end is not known yet, nothing is clipped at the top.
//   1. ls_env_kernel<R> (R = 2, 4; ls_env1_kernel at R = 1): the required gain c[n] = e[n] > thr ? thr / e[n] : 1 over
//      [a, b) = [m0 - 2 H, m1 + 2 H) within the row into the scratch (cbuf[n - a]), one flag per tile.  R > 1: a workgroup owns
//      a tile and walks the channels: tp_tile_sums on the channel's window (row pointer and tile origin both moved by g0, so a
//      sample lands in the LDS slot, and every chain has the order, of the whole-row kernels); positions outside the window
//      are zeros and reach only values nobody asks for (the host check: the window covers [a - Bk, b - 1 + Fw] within the
//      row); e is folded with fmaxf in registers.  There is no measured partial to tell a quiet tile by, so the shortcut is a
//      bound, per channel: no interpolated value exceeds max |x_c| over what the tile reads times the largest l1 norm of a
//      phase (the norms and the channels' maxima are reduced by one tree in LDS); where that (with a margin over the rounding
//      of the sums) stays at or under thr the channel is skipped -- every e_c of it is <= thr, so it changes c nowhere -- and
//      a tile whose channels are all quiet writes ones and clears its flag.
//      One cbuf, one flag per tile (the OR over the channels), one ctail per programme: the interpolated values behind the last
//      sample, only once n_total is known.  16-byte loads are decided per channel: w_stride need not keep the alignment.
//   2. ls_limit_kernel: lk_limit_kernel for global positions: tiles of LM_TILE outputs from m0; no flag over the tile and 2 H
//      around it: out_c = float(gL) x_c; otherwise c over the tile and 2 H around it in LDS, doubling minima, one ascending
//      fp32 chain per output, and g = min(1 - sum, c[n]) -- the exact sum never exceeds c[n], the fp32 one may by its rounding,
//      and nothing behind this kernel would trim it.  g is computed ONCE per output and applied to the C rows in a channel loop
//      (the 2 H + 1 FMAs per output and the doubling minima are the kernel's cost and do not depend on the channel; a second
//      grid dimension would repeat them C times).  Per tile: min g, max |out| over the rows.
//   3. ls_fold_kernel: one workgroup: record = {min g, max |out|} over [m0, m1) (exact folds: no order to fix).
// Three launches per call, whatever the span and whatever C.
struct ls_span {
    long long g0, wl, wh;         // the window's origin; window and row intersect in [wl, wh) (global)
    long long n;                  // n_total (INT64_MAX: unknown)
    long long m0, m1, a, b;       // outputs [m0, m1); c is needed over [a, b)
    long long tlo, nte;           // first envelope tile (global index at R > 1), how many
    long long nto;                // output tiles
    int known, tail;              // n is the row's length; ctail holds a value (R > 1, known, b == n)
    float* cbuf;                  // [b - a]
    float* ctail;                 // [1]
    int* flag;                    // [nte]
    float* gmin;                  // [nto]
    float* vpk;                   // [nto]
};

#define LS_SPAN_MAX (1LL << 30)   // outputs per call
#define LS_CMAX 8

// (one envelope per programme: the layout does not depend on C)
static void ls_layout(long long n_span, int H, size_t* total, ls_span* m, char* base) {
    const long long nc = n_span + 4LL * H;
    const long long nte = nc / TP_TILE + 3;               // (any anchoring of the tiles, and the tail's)
    const long long nto = n_span > 0 ? (n_span + LM_TILE - 1) / LM_TILE : 1;
    size_t off = 0;
    const size_t o_c = off;    off += lk_round((size_t)nc * sizeof(float));
    const size_t o_ct = off;   off += lk_round(sizeof(float));
    const size_t o_flag = off; off += lk_round((size_t)nte * sizeof(int));
    const size_t o_gm = off;   off += lk_round((size_t)nto * sizeof(float));
    const size_t o_vp = off;   off += lk_round((size_t)nto * sizeof(float));
    *total = off;
    if (m) {
        m->cbuf = (float*)(base + o_c);
        m->ctail = (float*)(base + o_ct);
        m->flag = (int*)(base + o_flag);
        m->gmin = (float*)(base + o_gm);
        m->vpk = (float*)(base + o_vp);
    }
}

// Tile blockIdx.x of the envelope at R > 1 holds K in [K0, K0 + TP_TILE), K0 = Kal + (tlo + blockIdx.x) TP_TILE; sample
// n = K - c / R collects the R interpolated values of K and |x[n]|.  q = c / R, rem = c mod R: value (K, p) lies in the row iff
// (n > 0 or n == 0 and p >= rem) and (n < N or n == N and p < rem) -- lk_env_kernel's c <= K R + p < c + R N without the
// product, which does not fit 64 bits when N is unknown.
template <int R>
__global__ __launch_bounds__(TP_T) void ls_env_kernel(const float* __restrict__ xw, long long w_stride, int C,
                                                      const float* __restrict__ bank, int J, int Jp, int c, long long Kal,
                                                      float thr, ls_span s) {
    extern __shared__ float4 tp_lds[];
    float* red = reinterpret_cast<float*>(tp_lds);        // [(R + C) TP_T] before the sums stage their tile over it
    const int l = threadIdx.x;
    const int q = c / R, rem = c - q * R;
    const long long K0 = Kal + (s.tlo + (long long)blockIdx.x) * TP_TILE;
    const long long nb = K0 + TP_KPL * l - q;             // the sample of this lane's first K
#pragma unroll
    for (int p = 0; p < R; ++p) {
        float v = 0.f;
        for (int i = l; i < J; i += TP_T) v += fabsf(bank[p * J + i]);
        red[p * TP_T + l] = v;
    }
    for (int ch = 0; ch < C; ++ch) {
        const float* xc = xw + (long long)ch * w_stride;
        float mx = 0.f;                                   // max |x_c| over what the sums of this tile read
        for (int i = l; i < TP_TILE + Jp; i += TP_T) {
            const long long j = K0 - Jp + 1 + i;
            if (j >= s.wl && j < s.wh) mx = fmaxf(mx, fabsf(xc[j - s.g0]));
        }
        red[(R + ch) * TP_T + l] = mx;
    }
    __syncthreads();
    for (int h = TP_T / 2; h > 0; h >>= 1) {              // one tree: the phases' l1 norms and the channels' maxima
        if (l < h) {
#pragma unroll
            for (int p = 0; p < R; ++p) red[p * TP_T + l] += red[p * TP_T + l + h];
            for (int ch = R; ch < R + C; ++ch) red[ch * TP_T + l] = fmaxf(red[ch * TP_T + l], red[ch * TP_T + l + h]);
        }
        __syncthreads();
    }
    float l1 = 1.f;                                       // (the sample itself counts with weight 1)
#pragma unroll
    for (int p = 0; p < R; ++p) l1 = fmaxf(l1, red[p * TP_T]);
    unsigned hot = 0;                                     // (uniform; 1.001 is far above the rounding of J fp32 FMAs)
    for (int ch = 0; ch < C; ++ch) hot |= (unsigned)(red[(R + ch) * TP_T] * l1 * 1.001f > thr) << ch;
    __syncthreads();                                      // (red is read: the sums may stage)
    float xv[TP_KPL], ev[TP_KPL];                         // max_c |x_c[n]|, max_c of the interpolated values of n
#pragma unroll
    for (int k = 0; k < TP_KPL; ++k) { xv[k] = 0.f; ev[k] = 0.f; }
    const int any = hot != 0;
    for (int ch = 0; ch < C; ++ch) {
        if (!(hot >> ch & 1u)) continue;
        const float* xc = xw + (long long)ch * w_stride;
#pragma unroll
        for (int k = 0; k < TP_KPL; ++k) {
            const long long nn = nb + k;
            if (nn >= s.a && nn < s.b) xv[k] = fmaxf(xv[k], fabsf(xc[nn - s.g0]));
        }
        float aa[R][TP_KPL], ab[R][TP_KPL];
        const bool vec = ((((uintptr_t)xc >> 2) - (uintptr_t)s.g0) & 3u) == 0;      // (uniform; the values do not depend on it)
        if (vec) tp_tile_sums<R, true>(xc, s.wh - s.g0, bank, J, Jp, K0 - s.g0, tp_lds, aa, ab);
        else tp_tile_sums<R, false>(xc, s.wh - s.g0, bank, J, Jp, K0 - s.g0, tp_lds, aa, ab);
#pragma unroll
        for (int k = 0; k < TP_KPL; ++k) {
            const long long nn = nb + k;
#pragma unroll
            for (int p = 0; p < R; ++p) {
                const bool lo_ok = nn > 0 || (nn == 0 && p >= rem);
                const bool hi_ok = !s.known || nn < s.n || (nn == s.n && p < rem);
                if (lo_ok && hi_ok) ev[k] = fmaxf(ev[k], fabsf(aa[p][k] + ab[p][k]));
            }
        }
        __syncthreads();                                  // (the staged tile is read: the next channel may stage its own)
    }
#pragma unroll
    for (int k = 0; k < TP_KPL; ++k) {
        const long long nn = nb + k;
        if (nn >= s.a && nn < s.b) {
            const float e = fmaxf(xv[k], ev[k]);
            s.cbuf[nn - s.a] = any && e > thr ? thr / e : 1.f;
        } else if (s.tail && nn == s.n) {
            *s.ctail = any && ev[k] > thr ? thr / ev[k] : 1.f;
        }
    }
    if (l == 0) s.flag[blockIdx.x] = any;
}

// The envelope at R = 1 (and of the sample-peak mode): e[n] = max_c |x_c[n]|; tile t holds samples from a + t TP_TILE.
__global__ __launch_bounds__(TP_T) void ls_env1_kernel(const float* __restrict__ xw, long long w_stride, int C, float thr,
                                                       ls_span s) {
    const int l = threadIdx.x;
    const long long n0 = s.a + (long long)blockIdx.x * TP_TILE;
    int hot = 0;
#pragma unroll
    for (int k = 0; k < TP_KPL; ++k) {
        const long long nn = n0 + l + k * TP_T;
        if (nn < s.b) {
            float e = 0.f;
            for (int ch = 0; ch < C; ++ch) e = fmaxf(e, fabsf(xw[(long long)ch * w_stride + (nn - s.g0)]));
            s.cbuf[nn - s.a] = e > thr ? thr / e : 1.f;
            hot |= e > thr;
        }
    }
    hot = __syncthreads_or(hot);
    if (l == 0) s.flag[blockIdx.x] = hot != 0;
}

// off: envelope tile of sample j is (j + off) / TP_TILE - tlo (c / R - Kal at R > 1) or (j - a) / TP_TILE (R = 1: off = -a,
// tlo = 0).  lev, the dynamic LDS and the arithmetic: lk_limit_kernel's.
__global__ __launch_bounds__(LM_T) void ls_limit_kernel(const float* __restrict__ xw, long long w_stride, int C, float gL, int H,
                                                        int lev, long long off, ls_span s, float* __restrict__ out,
                                                        long long out_stride) {
    extern __shared__ float lm_lds[];
    float* ra = lm_lds;                                   // (lm_minmax starts with a barrier: cs and ds are done with by then)
    float* rb = lm_lds + LM_T;
    const int l = threadIdx.x;
    const long long n = s.n;
    const long long n0 = s.m0 + (long long)blockIdx.x * LM_TILE;
    int active = 0;
    {
        const long long lo = n0 - 2 * H > s.a ? n0 - 2 * H : s.a;
        const long long hi = n0 + LM_TILE - 1 + 2 * H < s.b - 1 ? n0 + LM_TILE - 1 + 2 * H : s.b - 1;
        const long long tlo = (lo + off) / TP_TILE - s.tlo;
        long long thi = s.tail && hi == n - 1 ? s.nte - 1 : (hi + off) / TP_TILE - s.tlo;       // (the last sample reads ctail's tile)
        thi = thi > s.nte - 1 ? s.nte - 1 : thi;
        for (long long j = tlo + l; j <= thi; j += LM_T) active |= s.flag[j];
        active = lm_any(active, reinterpret_cast<int*>(lm_lds));
    }
    float gm = 1.f, vm = 0.f;
    if (!active) {
        for (int ch = 0; ch < C; ++ch) {
            const float* xc = xw + (long long)ch * w_stride;
            float* oc = out + (long long)ch * out_stride;
#pragma unroll
            for (int e = 0; e < LM_PER; ++e) {
                const long long nn = n0 + l + e * LM_T;
                if (nn < s.m1) {
                    const float v = xc[nn - s.g0] * gL;
                    oc[nn - s.m0] = v;
                    vm = fmaxf(vm, fabsf(v));
                }
            }
        }
    } else {
        const int Lc = LM_TILE + 4 * H, Lm = LM_TILE + 2 * H;
        float* cs = lm_lds;
        float* ds = cs + Lc;
        float* wk = ds + Lm;
        const long long c0 = n0 - 2 * H;
        for (int i = l; i < Lc; i += LM_T) {
            const long long j = c0 + i;
            float v = 1.f;                                // (outside the row, or behind what this span's outputs read: neutral)
            if (j >= s.a && j < s.b) {
                v = s.cbuf[j - s.a];
                if (s.tail && j == n - 1) v = fminf(v, *s.ctail);
            }
            cs[i] = v;
        }
        for (int k = l; k <= H; k += LM_T) wk[k] = (float)((1.0 + cospi((double)k / (double)(H + 1))) / (double)(2 * H + 2));
        __syncthreads();
        for (int lv = 0, st = 1; lv < lev; ++lv, st <<= 1) {
            for (int base = 0; base < Lc; base += LM_T) {
                const int i = base + l;
                float a = 1.f;
                if (i < Lc) {
                    a = cs[i];
                    if (i + st < Lc) a = fminf(a, cs[i + st]);
                }
                __syncthreads();
                if (i < Lc) cs[i] = a;
            }
            __syncthreads();
        }
        const int P = 1 << lev;
        for (int i = l; i < Lm; i += LM_T) {
            long long j = n0 - H + i;
            j = j < 0 ? 0 : (j > n - 1 ? n - 1 : j);      // (the clamped extension, against the ROW)
            const int a = (int)(j - n0) + H;              // cs index of j - H
            ds[i] = 1.f - fminf(cs[a], cs[a + 2 * H + 1 - P]);
        }
        __syncthreads();
        float acc[LM_PER];
#pragma unroll
        for (int e = 0; e < LM_PER; ++e) acc[e] = 0.f;
        for (int kk = 0; kk <= 2 * H; ++kk) {             // (k = kk - H ascending: a fixed order)
            const float w = wk[kk < H ? H - kk : kk - H];
#pragma unroll
            for (int e = 0; e < LM_PER; ++e) acc[e] = fmaf(w, ds[l + e * LM_T + kk], acc[e]);
        }
        float gg[LM_PER];                                 // float(gL) g of this lane's outputs, the same for every channel
#pragma unroll
        for (int e = 0; e < LM_PER; ++e) {
            const long long nn = n0 + l + e * LM_T;
            gg[e] = gL;
            if (nn < s.m1) {
                // g <= c[n] holds for the exact sum (every m under the window covers n); the fp32 chain drifts by up to
                // (2 H + 1) 2^-24, and a session has no trim behind it: the minimum keeps every SAMPLE of every channel under
                // the ceiling
                float cn = s.cbuf[nn - s.a];
                if (s.tail && nn == n - 1) cn = fminf(cn, *s.ctail);
                const float g = fminf(1.f - acc[e], cn);
                gg[e] = gL * g;
                gm = fminf(gm, g);
            }
        }
        for (int ch = 0; ch < C; ++ch) {
            const float* xc = xw + (long long)ch * w_stride;
            float* oc = out + (long long)ch * out_stride;
#pragma unroll
            for (int e = 0; e < LM_PER; ++e) {
                const long long nn = n0 + l + e * LM_T;
                if (nn < s.m1) {
                    const float v = xc[nn - s.g0] * gg[e];
                    oc[nn - s.m0] = v;
                    vm = fmaxf(vm, fabsf(v));
                }
            }
        }
    }
    lm_minmax(gm, vm, ra, rb);
    if (l == 0) {
        s.gmin[blockIdx.x] = gm;
        s.vpk[blockIdx.x] = vm;
    }
}

__global__ __launch_bounds__(LM_T) void ls_fold_kernel(ls_span s, double* __restrict__ record) {
    __shared__ float ra[LM_T], rb[LM_T];
    const int l = threadIdx.x;
    float gm = 1.f, vm = 0.f;
    for (long long j = l; j < s.nto; j += LM_T) {
        gm = fminf(gm, s.gmin[j]);
        vm = fmaxf(vm, s.vpk[j]);
    }
    lm_minmax(gm, vm, ra, rb);
    if (l == 0) {
        record[0] = gm;
        record[1] = vm;
    }
}

// Validation, geometry and the three launches of both entry points.  ``rows``: the linked entry, which also checks C and the
// strides and refuses an overlap of the blocks of windows and outputs BEFORE it accepts an empty span; the mono entry accepts
// the empty span first (each keeps the order it had as a file of its own).  Nothing is launched where anything is refused.
static int ls_run(bool rows, const float* xw, int64_t w_stride, int C, int64_t g0, int64_t wlen, int64_t n_total, int64_t m0,
                  int64_t m1, double gain, double ceiling_db, int H, const float* bank, int J, int R, int c, float* out,
                  int64_t out_stride, double* record, void* ws, size_t ws_bytes, vfx_stream_t stream) {
    if (!xw || !out || !record || !ws || g0 < 0 || wlen < 0 || n_total < 0 || m0 < 0 || m1 < m0 || m1 > n_total) return VFX_EINVAL;
    if (!rows) out_stride = m1 - m0;                      // (the one row: C = 1, w_stride = wlen from the entry point)
    if (H < 1 || H > LM_HMAX || (R != 1 && R != 2 && R != 4) || g0 > INT64_MAX - wlen || m1 - m0 > LS_SPAN_MAX) return VFX_EINVAL;
    if (rows && (C < 1 || C > LS_CMAX || w_stride < wlen || out_stride < m1 - m0 || w_stride > (INT64_MAX >> 6) ||
                 out_stride > (INT64_MAX >> 6)))
        return VFX_EINVAL;
    if (!std::isfinite(gain) || !(gain > 0.0) || !std::isfinite(ceiling_db)) return VFX_EINVAL;
    if (R > 1 && (!bank || J < 1 || J > TP_JMAX || c < 0 || (long long)c >= (long long)R * J)) return VFX_EINVAL;
    const double cl = pow(10.0, ceiling_db / 20.0);
    const float gLf = (float)gain, thr = (float)(cl / gain);
    if (!std::isfinite(gLf) || !(gLf > 0.f) || !std::isfinite(thr) || !(thr > 0.f)) return VFX_EINVAL;
    size_t need = 0;
    ls_span s = {};
    ls_layout(m1 - m0, H, &need, &s, (char*)ws);
    if (ws_bytes < need || ((uintptr_t)ws & 15u)) return VFX_EINVAL;
    // the block of the outputs may not overlap the block of the windows
    const uintptr_t xb = (uintptr_t)xw, xe = (uintptr_t)(xw + (C - 1) * w_stride + wlen);
    const uintptr_t ob = (uintptr_t)out, oe = (uintptr_t)(out + (C - 1) * out_stride + (m1 - m0));
    const bool overlap = !(xe <= ob || oe <= xb);
    if (rows && overlap) return VFX_EINVAL;
    if (m0 == m1) return VFX_OK;
    if (overlap) return VFX_EINVAL;
    const long long q = R > 1 ? c / R : 0;
    const long long Fw = q, Bk = R > 1 ? (long long)J - 1 - q : 0;
    const long long reach = 2LL * H;
    s.g0 = g0;
    s.n = n_total;
    s.m0 = m0;
    s.m1 = m1;
    s.known = n_total != INT64_MAX;
    s.a = m0 > reach ? m0 - reach : 0;
    s.b = n_total - m1 > reach ? m1 + reach : n_total;
    const long long need_lo = s.a > Bk ? s.a - Bk : 0;
    const long long need_hi = n_total - s.b > Fw ? s.b - 1 + Fw : n_total - 1;
    if (need_lo < g0 || need_hi - g0 >= wlen) return VFX_EINVAL;
    s.wl = g0;
    s.wh = n_total - g0 < wlen ? n_total : g0 + wlen;
    s.tail = R > 1 && s.known && s.b == n_total;
    s.nto = (m1 - m0 + LM_TILE - 1) / LM_TILE;
    hipStream_t st = (hipStream_t)stream;
    long long off;
    if (R > 1) {
        const long long Kal = tp_kal(c, R);
        off = q - Kal;
        s.tlo = (s.a + off) / TP_TILE;
        s.nte = ((s.tail ? n_total : s.b - 1) + off) / TP_TILE - s.tlo + 1;
        const int Jp = tp_jp(J);
        size_t tp_bytes = (size_t)(TP_TILE + Jp + R * Jp) * sizeof(float);
        if (tp_bytes < (size_t)(R + C) * TP_T * sizeof(float)) tp_bytes = (size_t)(R + C) * TP_T * sizeof(float);     // (red)
        const dim3 gt((unsigned)s.nte);
        if (R == 4) hipLaunchKernelGGL((ls_env_kernel<4>), gt, dim3(TP_T), tp_bytes, st, xw, (long long)w_stride, C, bank, J, Jp, c, Kal, thr, s);
        else hipLaunchKernelGGL((ls_env_kernel<2>), gt, dim3(TP_T), tp_bytes, st, xw, (long long)w_stride, C, bank, J, Jp, c, Kal, thr, s);
    } else {
        off = -s.a;
        s.tlo = 0;
        s.nte = (s.b - s.a + TP_TILE - 1) / TP_TILE;
        hipLaunchKernelGGL(ls_env1_kernel, dim3((unsigned)s.nte), dim3(TP_T), 0, st, xw, (long long)w_stride, C, thr, s);
    }
    VFX_LAUNCHED();
    int lev = 0;
    while ((2 << lev) <= 2 * H + 1) ++lev;
    const size_t lds = (size_t)(LM_TILE + 4 * H + LM_TILE + 2 * H + H + 1) * sizeof(float);
    int err = vfx_launch<ls_limit_kernel>(dim3((unsigned)s.nto), dim3(LM_T), lds, st, xw, (long long)w_stride, C, gLf, H, lev, off, s,
                                          out, (long long)out_stride);
    if (err != VFX_OK) return err;
    hipLaunchKernelGGL(ls_fold_kernel, dim3(1), dim3(LM_T), 0, st, s, record);
    VFX_LAUNCHED();
    return vfx_last_error();
}

extern "C" size_t vfx_limit_span_workspace_bytes(int64_t n_span, int H) {
    if (n_span < 0 || n_span > LS_SPAN_MAX || H < 1 || H > LM_HMAX) return 0;
    size_t total = 0;
    ls_layout(n_span, H, &total, nullptr, nullptr);
    return total;
}

extern "C" size_t vfx_limit_span_rows_workspace_bytes(int64_t n_span, int H, int C) {
    return C < 1 || C > LS_CMAX ? 0 : vfx_limit_span_workspace_bytes(n_span, H);
}

extern "C" int vfx_limit_span_f32(const float* xw, int64_t g0, int64_t wlen, int64_t n_total, int64_t m0, int64_t m1, double gain,
                                  double ceiling_db, int H, const float* bank, int J, int R, int c, float* out, double* record,
                                  void* ws, size_t ws_bytes, vfx_stream_t stream) {
    return ls_run(false, xw, wlen, 1, g0, wlen, n_total, m0, m1, gain, ceiling_db, H, bank, J, R, c, out, 0, record, ws, ws_bytes,
                  stream);
}

extern "C" int vfx_limit_span_rows_f32(const float* xw, int64_t w_stride, int C, int64_t g0, int64_t wlen, int64_t n_total,
                                       int64_t m0, int64_t m1, double gain, double ceiling_db, int H, const float* bank, int J, int R,
                                       int c, float* out, int64_t out_stride, double* record, void* ws, size_t ws_bytes,
                                       vfx_stream_t stream) {
    return ls_run(true, xw, w_stride, C, g0, wlen, n_total, m0, m1, gain, ceiling_db, H, bank, J, R, c, out, out_stride, record, ws,
                  ws_bytes, stream);
}
