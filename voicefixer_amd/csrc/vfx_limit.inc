// vfx_limit.inc -- the look-ahead peak limiter behind the loudness measurement (vfx_loudness_limit_f32; definition, resources
// and measured cost: DESIGN.md 3.14; included by vfx_loudness.hip, whose tiles and true-peak sums it shares).
//
// After the gate has produced {L, g, P, TP} per programme (a programme is one row unless the call is grouped):
//   1. lk_lim_prep_kernel: one lane per row: gL = 10^((T - L)/20) (1 when L = -inf), bound = Cl / TP < gL -- the comparison the
//      static gain makes, so a row that is not bound gets the bits of that path --, thr = float(Cl / gL), the row's programme.
//   2. lk_env_kernel<R> (R = 2, 4; lk_env1_kernel at R = 1): bound rows only: the required gain c[n] = min(1, thr / e[n]) of
//      every sample into the scratch, one flag per true-peak tile.  A tile whose partial of lk_truepeak_kernel and whose
//      samples stay at or under thr writes ones, clears its flag and forms no sum.  The interpolated values after the last
//      sample (K = c / R + n) belong to another lane than sample n - 1: they go to ctail[row], folded in by the reader.
//   3. lk_limit_kernel: per tile of LM_TILE outputs.  No flag over the tile and 2 H around it (and every row that is not
//      bound): out = float(gL) x.  Otherwise c (the minimum over the programme's rows) over the tile and 2 H around it is
//      staged in LDS, log2-many doubling passes turn it into minima over 2^k samples, two of which cover the 2 H + 1 window
//      (m), and every output sums its 2 H + 1 deficits w[k] (1 - m) in ascending k -- one fp32 chain, the same whatever the
//      batch -- g = 1 - sum, out = (float(gL) g) x.  Per tile: min g and max |out|.
//   4. lk_truepeak_kernel on out, bound rows only (their lengths in n2, 0 elsewhere).
//   5. lk_lim_fold_kernel: one workgroup per programme: TPv, t = min(1, Cl / TPv), min g -> the record, t to the rows.
//   6. lk_trim_kernel: out *= float(t) where t < 1.
// Six launches behind the gate at R > 1, five at R = 1; none depends on B or on a length, none waits for the host.
#define LM_T 256
#define LM_PER 4
#define LM_TILE (LM_T * LM_PER)
#define LM_HMAX 4096

struct lk_lim_row {               // what every kernel behind the gate needs to know of a row
    float gL, thr, t;             // float(gL), float(Cl / gL), the trim (1 until the fold has run)
    int bound, r0, r1;            // the row's programme is rows [r0, r1)
    int pad[2];
};

struct lk_lim {                   // the limiter's slices of the workspace (behind lk_layout's and lk_ext_layout's)
    double* res4;                 // [B][4]       {L, g, P, TP} of the gate, per programme
    lk_lim_row* row;              // [B]
    int* n2;                      // [B]          n of a bound row, 0 of any other
    float* ctail;                 // [B]          required gain of the interpolated values after the last sample
    float* cbuf;                  // [B][cs]      required gain per sample (bound rows only)
    int* flag;                    // [B][ntiles]  true-peak tile holds a c < 1
    float* part2;                 // [B][ntiles]  true-peak partials of the limited row
    float* gmin;                  // [B][nto]     min g of every output tile
    float* vpk;                   // [B][nto]     max |out| of every output tile
    long long cs, ntiles, nto;
};

static void lk_lim_layout(int B, long long n_max, size_t* total, lk_lim* m, char* base) {
    const long long ntiles = tp_ntiles(n_max);
    const long long nto = n_max > 0 ? (n_max + LM_TILE - 1) / LM_TILE : 1;
    const long long cs = (n_max + 3) / 4 * 4;
    size_t off = 0;
    const size_t o_res = off;  off += lk_round((size_t)B * 4 * sizeof(double));
    const size_t o_row = off;  off += lk_round((size_t)B * sizeof(lk_lim_row));
    const size_t o_n2 = off;   off += lk_round((size_t)B * sizeof(int));
    const size_t o_ct = off;   off += lk_round((size_t)B * sizeof(float));
    const size_t o_c = off;    off += lk_round((size_t)B * cs * sizeof(float));
    const size_t o_flag = off; off += lk_round((size_t)B * ntiles * sizeof(int));
    const size_t o_p2 = off;   off += lk_round((size_t)B * ntiles * sizeof(float));
    const size_t o_gm = off;   off += lk_round((size_t)B * nto * sizeof(float));
    const size_t o_vp = off;   off += lk_round((size_t)B * nto * sizeof(float));
    *total = off;
    if (m) {
        m->res4 = (double*)(base + o_res);
        m->row = (lk_lim_row*)(base + o_row);
        m->n2 = (int*)(base + o_n2);
        m->ctail = (float*)(base + o_ct);
        m->cbuf = (float*)(base + o_c);
        m->flag = (int*)(base + o_flag);
        m->part2 = (float*)(base + o_p2);
        m->gmin = (float*)(base + o_gm);
        m->vpk = (float*)(base + o_vp);
        m->cs = cs;
        m->ntiles = ntiles;
        m->nto = nto;
    }
}

// out may be x itself with the same stride (every sample is read and written by one lane, after the envelope is in the
// scratch); any other overlap of the two batches is refused.
static bool lk_lim_alias_ok(const float* x, int64_t x_stride, const float* out, int64_t out_stride, int B, int64_t n_max) {
    if (!x || !out || (out == x && out_stride == x_stride)) return true;
    const uintptr_t xb = (uintptr_t)x, xe = (uintptr_t)(x + (int64_t)(B - 1) * x_stride + n_max);
    const uintptr_t ob = (uintptr_t)out, oe = (uintptr_t)(out + (int64_t)(B - 1) * out_stride + n_max);
    return xe <= ob || oe <= xb;
}

// One lane per row.  G > 0: the row's programme is looked up in group_start (rows in no programme: bound = 0, gL = 1).
__global__ __launch_bounds__(LK_T) void lk_lim_prep_kernel(const int* __restrict__ n_rows, long long n_max, int B, int G,
                                                           double target, double ceiling_db, lk_grp grp, lk_lim lm) {
    const int r = blockIdx.x * LK_T + threadIdx.x;
    if (r >= B) return;
    int o = r, r0 = r, r1 = r + 1;
    if (G > 0) {
        o = -1;
        for (int g = 0; g < G; ++g) {
            int a = grp.start[g], b = grp.start[g + 1];
            a = a < 0 ? 0 : (a > B ? B : a);
            b = b < a ? a : (b > B ? B : b);
            if (r >= a && r < b) { o = g; r0 = a; r1 = b; break; }
        }
    }
    long long n = n_rows[r];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    double gL = 1.0;
    int bound = 0;
    float thr = INFINITY;
    if (o >= 0) {
        const double L = lm.res4[4 * o], tpk = lm.res4[4 * o + 3];
        if (isfinite(L)) gL = pow(10.0, (target - L) / 20.0);
        const double cl = pow(10.0, ceiling_db / 20.0);
        bound = cl / tpk < gL;                            // (the gate's own comparison; TP = 0: inf, not bound)
        thr = (float)(cl / gL);
    }
    lk_lim_row w;
    w.gL = (float)gL; w.thr = thr; w.t = 1.f;
    w.bound = bound; w.r0 = r0; w.r1 = r1;
    w.pad[0] = 0; w.pad[1] = 0;
    lm.row[r] = w;
    lm.n2[r] = bound ? (int)n : 0;
    lm.ctail[r] = 1.f;
}

// The envelope of a bound row at R > 1: lk_truepeak_kernel's tiles and sums, c[n] instead of a maximum.  Sample n = K - c / R
// collects the R interpolated values of K (the times in (n - 1, n]) and |x[n]|.
template <int R, bool VEC>
__global__ __launch_bounds__(TP_T) void lk_env_kernel(const float* __restrict__ x, long long x_stride,
                                                      const int* __restrict__ n_rows, long long n_max,
                                                      const float* __restrict__ bank, int J, int Jp, lk_tp t, lk_lim lm) {
    extern __shared__ float4 tp_lds[];
    const int r = blockIdx.y, l = threadIdx.x;
    long long n = n_rows[r];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    if ((long long)blockIdx.x >= tp_tiles(n, R, t.c, t.Kal)) return;         // (uniform over the workgroup)
    const lk_lim_row info = lm.row[r];
    if (!info.bound) return;
    const float thr = info.thr;
    const long long t_end = (long long)t.c + (long long)R * n;
    const long long K0 = t.Kal + (long long)blockIdx.x * TP_TILE;
    const float* xr = x + (long long)r * x_stride;
    float* cr = lm.cbuf + (long long)r * lm.cs;
    const long long nb = K0 + TP_KPL * l - t.c / R;      // the sample of this lane's first K
    float xv[TP_KPL];
    int hot = l == 0 && t.part[(long long)r * t.ntiles + blockIdx.x] > thr;
#pragma unroll
    for (int k = 0; k < TP_KPL; ++k) {
        const long long nn = nb + k;
        xv[k] = nn >= 0 && nn < n ? fabsf(xr[nn]) : 0.f;
        hot |= xv[k] > thr;
    }
    if (!__syncthreads_or(hot)) {                         // nothing above the threshold in this tile: c = 1, no sums
#pragma unroll
        for (int k = 0; k < TP_KPL; ++k)
            if (nb + k >= 0 && nb + k < n) cr[nb + k] = 1.f;
        if (l == 0) lm.flag[(long long)r * lm.ntiles + blockIdx.x] = 0;
        return;
    }
    float aa[R][TP_KPL], ab[R][TP_KPL];
    tp_tile_sums<R, VEC>(xr, n, bank, J, Jp, K0, tp_lds, aa, ab);
#pragma unroll
    for (int k = 0; k < TP_KPL; ++k) {
        float ev = 0.f;
#pragma unroll
        for (int p = 0; p < R; ++p) {
            const long long tt = (K0 + TP_KPL * l + k) * R + p;
            if (tt >= t.c && tt < t_end) ev = fmaxf(ev, fabsf(aa[p][k] + ab[p][k]));
        }
        const long long nn = nb + k;
        if (nn >= 0 && nn < n) {
            const float e = fmaxf(xv[k], ev);
            cr[nn] = e > thr ? thr / e : 1.f;
        } else if (nn == n) {
            lm.ctail[r] = ev > thr ? thr / ev : 1.f;
        }
    }
    if (l == 0) lm.flag[(long long)r * lm.ntiles + blockIdx.x] = 1;
}

// The envelope of a bound row at R = 1 (and of the sample-peak limiter): e[n] = |x[n]|; tile b holds samples from b TP_TILE.
__global__ __launch_bounds__(TP_T) void lk_env1_kernel(const float* __restrict__ x, long long x_stride,
                                                       const int* __restrict__ n_rows, long long n_max, lk_lim lm) {
    const int r = blockIdx.y, l = threadIdx.x;
    long long n = n_rows[r];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    const long long n0 = (long long)blockIdx.x * TP_TILE;
    if (n0 >= n) return;
    const lk_lim_row info = lm.row[r];
    if (!info.bound) return;
    const float thr = info.thr;
    const float* xr = x + (long long)r * x_stride;
    float* cr = lm.cbuf + (long long)r * lm.cs;
    int hot = 0;
#pragma unroll
    for (int k = 0; k < TP_KPL; ++k) {
        const long long nn = n0 + l + k * TP_T;
        if (nn < n) {
            const float e = fabsf(xr[nn]);
            cr[nn] = e > thr ? thr / e : 1.f;
            hot |= e > thr;
        }
    }
    hot = __syncthreads_or(hot);
    if (l == 0) lm.flag[(long long)r * lm.ntiles + blockIdx.x] = hot != 0;
}

// workgroup minimum of a and maximum of b (every lane gets both)
__device__ __forceinline__ void lm_minmax(float& a, float& b, float* ra, float* rb) {
    const int l = threadIdx.x;
    __syncthreads();
    ra[l] = a;
    rb[l] = b;
    __syncthreads();
    for (int h = LM_T / 2; h > 0; h >>= 1) {
        if (l < h) { ra[l] = fminf(ra[l], ra[l + h]); rb[l] = fmaxf(rb[l], rb[l + h]); }
        __syncthreads();
    }
    a = ra[0];
    b = rb[0];
}

// workgroup OR through one LDS word (lk_limit_kernel keeps ALL its LDS dynamic: vfx_launch raises the dynamic limit to the whole
// 160 KB of a CU, which leaves no room for a static byte, and __syncthreads_or brings static LDS of its own)
__device__ __forceinline__ int lm_any(int v, int* slot) {
    __syncthreads();
    if (threadIdx.x == 0) *slot = 0;
    __syncthreads();
    if (v) *slot = 1;                                     // (every writer writes the same value)
    __syncthreads();
    return *slot;
}

// off: true-peak tile of sample n is (n + off) / TP_TILE (c / R - Kal; 0 at R = 1).  lev: 2^lev <= 2 H + 1 < 2^(lev + 1).
// Dynamic LDS: c over [n0 - 2H, n0 + LM_TILE + 2H), the deficits 1 - m over [n0 - H, n0 + LM_TILE + H), w[0..H]; the
// reductions reuse its first 2 LM_T words.
__global__ __launch_bounds__(LM_T) void lk_limit_kernel(const float* x, long long x_stride,          // (out may be x)
                                                        const int* __restrict__ n_rows, long long n_max, int B, int H, int lev,
                                                        long long off, lk_tp t, lk_lim lm, float* out, long long out_stride) {
    extern __shared__ float lm_lds[];
    float* ra = lm_lds;                                   // (lm_minmax starts with a barrier: cs and ds are done with by then)
    float* rb = lm_lds + LM_T;
    const int r = blockIdx.y, l = threadIdx.x;
    long long n = n_rows[r];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    const long long n0 = (long long)blockIdx.x * LM_TILE;
    if (n0 >= n) return;                                  // (uniform over the workgroup)
    const lk_lim_row info = lm.row[r];
    const float gL = info.gL;
    const float* xr = x + (long long)r * x_stride;
    float* yr = out + (long long)r * out_stride;
    int r0 = info.r0, r1 = info.r1;
    r0 = r0 < 0 ? 0 : (r0 > B ? B : r0);
    r1 = r1 < r0 ? r0 : (r1 > B ? B : r1);
    int active = 0;
    if (info.bound) {
        const long long lo = n0 - 2 * H > 0 ? n0 - 2 * H : 0;
        const long long hi = n0 + LM_TILE - 1 + 2 * H < n - 1 ? n0 + LM_TILE - 1 + 2 * H : n - 1;
        const long long nt = t.R > 1 ? tp_tiles(n, t.R, t.c, t.Kal) : (n + TP_TILE - 1) / TP_TILE;
        const long long tlo = (lo + off) / TP_TILE;
        long long thi = hi == n - 1 ? nt - 1 : (hi + off) / TP_TILE;          // (the last sample also reads ctail's tile)
        thi = thi > nt - 1 ? nt - 1 : thi;
        for (int rr = r0; rr < r1; ++rr)
            for (long long j = tlo + l; j <= thi; j += LM_T) active |= lm.flag[(long long)rr * lm.ntiles + j];
        active = lm_any(active, reinterpret_cast<int*>(lm_lds));
    }
    float gm = 1.f, vm = 0.f;
    if (!active) {
#pragma unroll
        for (int e = 0; e < LM_PER; ++e) {
            const long long nn = n0 + l + e * LM_T;
            if (nn < n) {
                const float v = xr[nn] * gL;
                yr[nn] = v;
                vm = fmaxf(vm, fabsf(v));
            }
        }
        if (!info.bound) return;
    } else {
        const int Lc = LM_TILE + 4 * H, Lm = LM_TILE + 2 * H;
        float* cs = lm_lds;
        float* ds = cs + Lc;
        float* wk = ds + Lm;
        const long long c0 = n0 - 2 * H;
        for (int i = l; i < Lc; i += LM_T) {
            const long long j = c0 + i;
            float v = 1.f;                                // (outside the row: neutral)
            if (j >= 0 && j < n)
                for (int rr = r0; rr < r1; ++rr) {
                    v = fminf(v, lm.cbuf[(long long)rr * lm.cs + j]);
                    if (j == n - 1) v = fminf(v, lm.ctail[rr]);
                }
            cs[i] = v;
        }
        for (int k = l; k <= H; k += LM_T) wk[k] = (float)((1.0 + cospi((double)k / (double)(H + 1))) / (double)(2 * H + 2));
        __syncthreads();
        // cs[i] <- min c[i .. i + 2^lev): one doubling per level, 256 entries at a time in ascending order (an entry reads
        // itself and one further up, which no earlier chunk has rewritten)
        for (int lv = 0, s = 1; lv < lev; ++lv, s <<= 1) {
            for (int base = 0; base < Lc; base += LM_T) {
                const int i = base + l;
                float a = 1.f;
                if (i < Lc) {
                    a = cs[i];
                    if (i + s < Lc) a = fminf(a, cs[i + s]);
                }
                __syncthreads();
                if (i < Lc) cs[i] = a;
            }
            __syncthreads();
        }
        const int P = 1 << lev;
        for (int i = l; i < Lm; i += LM_T) {
            long long j = n0 - H + i;
            j = j < 0 ? 0 : (j > n - 1 ? n - 1 : j);      // (the clamped extension)
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
#pragma unroll
        for (int e = 0; e < LM_PER; ++e) {
            const long long nn = n0 + l + e * LM_T;
            if (nn < n) {
                const float g = 1.f - acc[e];
                const float v = xr[nn] * (gL * g);
                yr[nn] = v;
                gm = fminf(gm, g);
                vm = fmaxf(vm, fabsf(v));
            }
        }
    }
    lm_minmax(gm, vm, ra, rb);
    if (l == 0) {
        lm.gmin[(long long)r * lm.nto + blockIdx.x] = gm;
        lm.vpk[(long long)r * lm.nto + blockIdx.x] = vm;
    }
}

// One workgroup per programme (per row when G = 0): result[o] = {L, gL, P, TP, bound, min g, t, TPv t}.  A programme that is not
// bound: {.., 0, 1, 1, float(gL) TP}.
__global__ __launch_bounds__(LM_T) void lk_lim_fold_kernel(const int* __restrict__ n_rows, long long n_max, int G, double target,
                                                           double ceiling_db, double* __restrict__ result, lk_tp t,
                                                           lk_grp grp, lk_lim lm) {
    __shared__ float ra[LM_T], rb[LM_T];
    const int l = threadIdx.x, o = blockIdx.x;
    int r = o, r1 = o + 1;
    if (G > 0) {
        r = grp.start[o];
        r1 = grp.start[o + 1];
        r = r < 0 ? 0 : (r > grp.B ? grp.B : r);
        r1 = r1 < r ? r : (r1 > grp.B ? grp.B : r1);
    }
    const bool any = r < r1;
    long long n = any ? n_rows[r] : 0;
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    const int bound = any ? lm.row[r].bound : 0;
    float gm = 1.f, vm = 0.f;
    if (bound) {                                          // (uniform over the workgroup)
        const long long nto = (n + LM_TILE - 1) / LM_TILE;
        const long long nt = t.R > 1 ? tp_tiles(n, t.R, t.c, t.Kal) : 0;
        for (int rr = r; rr < r1; ++rr) {
            for (long long j = l; j < nto; j += LM_T) {
                gm = fminf(gm, lm.gmin[(long long)rr * lm.nto + j]);
                vm = fmaxf(vm, lm.vpk[(long long)rr * lm.nto + j]);
            }
            for (long long j = l; j < nt; j += LM_T) vm = fmaxf(vm, lm.part2[(long long)rr * lm.ntiles + j]);
        }
        lm_minmax(gm, vm, ra, rb);
    }
    if (l == 0) {
        const double L = lm.res4[4 * o], tpk = lm.res4[4 * o + 3];
        const double gL = isfinite(L) ? pow(10.0, (target - L) / 20.0) : 1.0;
        const double cl = pow(10.0, ceiling_db / 20.0);
        float tf = 1.f;
        double after = (double)(float)gL * tpk;
        if (bound) {
            const double tpv = vm;
            if (tpv > cl) tf = (float)(cl / tpv);
            after = tpv * (double)tf;
        }
        result[8 * o] = L;
        result[8 * o + 1] = gL;
        result[8 * o + 2] = lm.res4[4 * o + 2];
        result[8 * o + 3] = tpk;
        result[8 * o + 4] = bound;
        result[8 * o + 5] = gm;
        result[8 * o + 6] = tf;
        result[8 * o + 7] = after;
        for (int rr = r; rr < r1; ++rr) lm.row[rr].t = tf;
    }
}

__global__ __launch_bounds__(LK_T) void lk_trim_kernel(const int* __restrict__ n_rows, long long n_max, lk_lim lm, float* out,
                                                       long long out_stride) {
    const int r = blockIdx.y;
    const lk_lim_row info = lm.row[r];
    if (!info.bound || !(info.t < 1.f)) return;           // (uniform over the workgroup)
    long long n = n_rows[r];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    float* yr = out + (long long)r * out_stride;
    const long long step = (long long)gridDim.x * LK_T;
    for (long long i = (long long)blockIdx.x * LK_T + threadIdx.x; i < n; i += step) yr[i] *= info.t;
}

// The launches behind the gate (vfx_loudness_limit_f32).  t: the measurement's true-peak tiles (t.R = 1: nothing was
// oversampled); G = 0: every row is its own programme.
static int lk_limit_run(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max, double target,
                        double ceiling_db, const float* bank, int J, int H, float* out, int64_t out_stride, double* result,
                        hipStream_t s, lk_tp t, lk_grp grp, int G, lk_lim lm) {
    const int count = G > 0 ? G : B;
    hipLaunchKernelGGL(lk_lim_prep_kernel, dim3((unsigned)((B + LK_T - 1) / LK_T)), dim3(LK_T), 0, s, (const int*)n_rows,
                       (long long)n_max, B, G, target, ceiling_db, grp, lm);
    VFX_LAUNCHED();
    const bool vx = vfx_aligned16(x) && x_stride % 4 == 0;
    const int Jp = tp_jp(J);
    const size_t tp_bytes = (size_t)(TP_TILE + Jp + t.R * Jp) * sizeof(float);
    const dim3 gt((unsigned)lm.ntiles, (unsigned)B);
    if (t.R > 1) {
#define ENV_LAUNCH(RR, VV) hipLaunchKernelGGL((lk_env_kernel<RR, VV>), gt, dim3(TP_T), tp_bytes, s, x, (long long)x_stride, \
                                              (const int*)n_rows, (long long)n_max, bank, J, Jp, t, lm)
        if (t.R == 4) { if (vx) ENV_LAUNCH(4, true); else ENV_LAUNCH(4, false); }
        else { if (vx) ENV_LAUNCH(2, true); else ENV_LAUNCH(2, false); }
#undef ENV_LAUNCH
    } else {
        hipLaunchKernelGGL(lk_env1_kernel, gt, dim3(TP_T), 0, s, x, (long long)x_stride, (const int*)n_rows, (long long)n_max, lm);
    }
    VFX_LAUNCHED();
    int lev = 0;
    while ((2 << lev) <= 2 * H + 1) ++lev;
    const long long off = t.R > 1 ? (long long)(t.c / t.R) - t.Kal : 0;
    const size_t lds = (size_t)(LM_TILE + 4 * H + LM_TILE + 2 * H + H + 1) * sizeof(float);
    int err = vfx_launch<lk_limit_kernel>(dim3((unsigned)lm.nto, (unsigned)B), dim3(LM_T), lds, s, x, (long long)x_stride,
                                          (const int*)n_rows, (long long)n_max, B, H, lev, off, t, lm, out, (long long)out_stride);
    if (err != VFX_OK) return err;
    if (t.R > 1) {                                        // the true peak of the limited rows (n2: 0 where not bound)
        const bool vo = vfx_aligned16(out) && out_stride % 4 == 0;
#define TP2_LAUNCH(RR, VV) hipLaunchKernelGGL((lk_truepeak_kernel<RR, VV>), gt, dim3(TP_T), tp_bytes, s, (const float*)out, \
                                              (long long)out_stride, (const int*)lm.n2, (long long)n_max, bank, J, Jp, lm.part2, t)
        if (t.R == 4) { if (vo) TP2_LAUNCH(4, true); else TP2_LAUNCH(4, false); }
        else { if (vo) TP2_LAUNCH(2, true); else TP2_LAUNCH(2, false); }
#undef TP2_LAUNCH
        VFX_LAUNCHED();
    }
    hipLaunchKernelGGL(lk_lim_fold_kernel, dim3((unsigned)count), dim3(LM_T), 0, s, (const int*)n_rows, (long long)n_max, G, target,
                       ceiling_db, result, t, grp, lm);
    VFX_LAUNCHED();
    long long nbx = (n_max + LK_T - 1) / LK_T;
    nbx = nbx < 1 ? 1 : (nbx > 2048 ? 2048 : nbx);
    hipLaunchKernelGGL(lk_trim_kernel, dim3((unsigned)nbx, (unsigned)B), dim3(LK_T), 0, s, (const int*)n_rows, (long long)n_max, lm,
                       out, (long long)out_stride);
    VFX_LAUNCHED();
    return vfx_last_error();
}
