// Word-length reduction: float32 rows -> 16- or 24-bit PCM with seeded dither (voicefixer_amd/wordlength.py is the
// specification; the integers written here are its integers, bit for bit).
//
//   vfx_quantize_rows_f32   q = clamp(rint(x * 2^(b-1) + d(n)), -2^(b-1), 2^(b-1) - 1) in float64, d(n) a pure function of the
//                           sample's absolute index n = n0 + i, its channel and the seed: no state is carried along a row, so the
//                           grid is (tiles of 1024 samples, rows) -- capped: a workgroup walks further tiles of its row -- and a
//                           thread takes four consecutive samples of a tile.
//
// Dither words: k_t(n) = word n % 4 of Philox4x32-10(counter (n / 4, channel, t), key(seed)) >> 8.  A thread draws the block of its
// first sample, n_a / 4, once per stream.  Its other samples lie in the same block when n0 % 4 == 0; otherwise (and for the
// k_0(n - 1) of the high-passed dither) some lie in the neighbouring thread's block, which is handed over through LDS -- only the
// two blocks beyond the tile's ends are drawn a second time, by one thread each.
//
// The multiply-add runs as ONE float64 fma (the product is exact, the sum rounds once, as the specification's does); the per-row
// counts go through a wave reduction and at most one vector atomic per workgroup (see the end of the kernel).
#include "vfx_common.h"
#include "vfx_philox.h"

namespace {

constexpr int Q_THREADS = 256;
constexpr int Q_TILE = Q_THREADS * 4;      // samples per workgroup and tile
constexpr int Q_GRID = 2048;               // workgroups of a launch (about): see the per-row counts at the kernel's end

struct QuantArgs {
    const float* x;
    long long x_stride;
    const int32_t* n_rows;
    long long n_max;
    const long long* n0;
    const int32_t* chan;
    uint2 key;
    void* out;
    long long out_stride;
    int32_t* result;
};

// w[k] <- w[k + s], 0 <= s <= 3 (wave-uniform), for the leading N - 3 entries: constant indices only, so w stays in registers
template <int N>
__device__ __forceinline__ void shift_words(uint32_t (&w)[N], int s) {
    if (s & 1) {
#pragma unroll
        for (int k = 0; k + 1 < N; ++k) w[k] = w[k + 1];
    }
    if (s & 2) {
#pragma unroll
        for (int k = 0; k + 2 < N; ++k) w[k] = w[k + 2];
    }
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// DITHER 0: none, 1: tpdf (k_0(n) - k_1(n)), 2: hp (k_0(n) - k_0(n - 1); n = 0: the tpdf value).  VEC: every row of x starts
// 16-byte aligned and every row of out 16-byte (int16 rows: 8-byte) aligned -- a thread with four samples inside its row then
// moves them with one load and one store; the others, and every thread without VEC, go sample by sample.
template <int BITS, int DITHER, bool VEC>
__global__ __launch_bounds__(Q_THREADS) void quantize_kernel(QuantArgs a) {
    __shared__ uint4 sh0[Q_THREADS + 2];
    __shared__ uint4 sh1[DITHER == 1 ? Q_THREADS + 2 : 1];
    const int r = blockIdx.y, tid = threadIdx.x;
    long long len = a.n_rows[r];
    len = len < 0 ? 0 : (len > a.n_max ? a.n_max : len);
    int clipped = 0, peak = 0;
    // tiles blockIdx.x, blockIdx.x + gridDim.x, ... of the row (the trip count is the same for the whole workgroup)
    for (long long tile0 = (long long)blockIdx.x * Q_TILE; tile0 < len; tile0 += (long long)gridDim.x * Q_TILE) {
        const long long i0 = tile0 + 4 * tid;
        const unsigned long long na = (unsigned long long)(a.n0 ? a.n0[r] : 0) + (unsigned long long)i0;
        const uint32_t c = a.chan ? (uint32_t)a.chan[r] : 0u;
        const int s = (int)(na & 3);           // the same for every thread of the row
        const unsigned long long qa = na >> 2;

        int diff[4] = {0, 0, 0, 0};            // d(n) * 2^24
        if (DITHER != 0) {
            const uint4 A0 = philox4x32_10(make_uint4((uint32_t)qa, (uint32_t)(qa >> 32), c, 0u), a.key);
            uint4 A1 = make_uint4(0u, 0u, 0u, 0u);
            if (DITHER == 1 || na == 0) A1 = philox4x32_10(make_uint4((uint32_t)qa, (uint32_t)(qa >> 32), c, 1u), a.key);
            uint4 N0 = A0, N1 = A1, P0 = A0;   // the next thread's blocks, the previous thread's (read only where needed)
            const bool need_next = s != 0, need_prev = DITHER == 2 && s == 0;
            if (need_next || need_prev) {
                __syncthreads();               // (the previous tile's reads are done)
                sh0[tid + 1] = A0;
                if (DITHER == 1) sh1[tid + 1] = A1;
                if (need_next && tid == Q_THREADS - 1) {
                    const unsigned long long qn = qa + 1;
                    sh0[Q_THREADS + 1] = philox4x32_10(make_uint4((uint32_t)qn, (uint32_t)(qn >> 32), c, 0u), a.key);
                    if (DITHER == 1)
                        sh1[Q_THREADS + 1] = philox4x32_10(make_uint4((uint32_t)qn, (uint32_t)(qn >> 32), c, 1u), a.key);
                }
                if (need_prev && tid == 0 && qa > 0) {
                    const unsigned long long qp = qa - 1;
                    sh0[0] = philox4x32_10(make_uint4((uint32_t)qp, (uint32_t)(qp >> 32), c, 0u), a.key);
                }
                __syncthreads();
                if (need_next) {
                    N0 = sh0[tid + 2];
                    if (DITHER == 1) N1 = sh1[tid + 2];
                }
                if (need_prev && (tid > 0 || qa > 0)) P0 = sh0[tid];
            }
            if (DITHER == 1) {
                uint32_t w0[7] = {A0.x, A0.y, A0.z, A0.w, N0.x, N0.y, N0.z};
                uint32_t w1[7] = {A1.x, A1.y, A1.z, A1.w, N1.x, N1.y, N1.z};
                shift_words(w0, s);
                shift_words(w1, s);
#pragma unroll
                for (int j = 0; j < 4; ++j) diff[j] = (int)(w0[j] >> 8) - (int)(w1[j] >> 8);
            } else {
                // e[k] = k_0's word of sample n_a - 1 + k: the previous block's last word, the own block, the next block
                uint32_t e[8] = {P0.w, A0.x, A0.y, A0.z, A0.w, N0.x, N0.y, N0.z};
                shift_words(e, s);
#pragma unroll
                for (int j = 0; j < 4; ++j) diff[j] = (int)(e[j + 1] >> 8) - (int)(e[j] >> 8);
                if (na == 0) diff[0] = (int)(A0.x >> 8) - (int)(A1.x >> 8);
            }
        }

        if (i0 < len) {
            const float* xp = a.x + (long long)r * a.x_stride + i0;
            const int m = len - i0 >= 4 ? 4 : (int)(len - i0);
            constexpr int TAIL = VEC ? 3 : 4;  // most samples the sample-by-sample path moves (with VEC it sees row ends only)
            float e[4] = {0.f, 0.f, 0.f, 0.f};
            if (VEC && m == 4) {
                const float4 v = *reinterpret_cast<const float4*>(xp);
                e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < TAIL; ++j)
                    if (j < m) e[j] = xp[j];
            }
            constexpr double SCALE = (double)(1 << (BITS - 1)), LO = -SCALE, HI = SCALE - 1.0;
            int q[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double v = DITHER != 0 ? __builtin_fma((double)e[j], SCALE, (double)diff[j] * 0x1p-24) : (double)e[j] * SCALE;
                const bool nan = v != v;
                const double rv = nan ? 0.0 : __builtin_rint(v);          // round half to even
                const double cl = rv < LO ? LO : (rv > HI ? HI : rv);
                q[j] = (int)cl;
                if (j < m) {
                    clipped += (nan || cl != rv) ? 1 : 0;
                    peak = max(peak, q[j] < 0 ? -q[j] : q[j]);
                }
            }
            if (BITS == 16) {
                int16_t* op = reinterpret_cast<int16_t*>(a.out) + (long long)r * a.out_stride + i0;
                if (VEC && m == 4) {
                    uint2 pk;
                    pk.x = ((uint32_t)q[0] & 0xffffu) | ((uint32_t)q[1] << 16);
                    pk.y = ((uint32_t)q[2] & 0xffffu) | ((uint32_t)q[3] << 16);
                    *reinterpret_cast<uint2*>(op) = pk;
                    asm volatile("");          // (see the 24-bit store below)
                } else {
#pragma unroll
                    for (int j = 0; j < TAIL; ++j)
                        if (j < m) op[j] = (int16_t)q[j];
                }
            } else {
                int32_t* op = reinterpret_cast<int32_t*>(a.out) + (long long)r * a.out_stride + i0;
                if (VEC && m == 4) {
                    *reinterpret_cast<int4*>(op) = make_int4(q[0], q[1], q[2], q[3]);
                    // keeps the branches' last instructions apart: without it the compiler sinks the last element's store into a
                    // tail shared with the sample-by-sample path and this one leaves as 12 + 4 bytes
                    asm volatile("");
                } else {
#pragma unroll
                    for (int j = 0; j < TAIL; ++j)
                        if (j < m) op[j] = q[j];
                }
            }
        }
    }
    // Per-row counts: wave reduction, the four waves folded through LDS, then at most one vector atomic each per workgroup -- and
    // none where it would change nothing: every workgroup of a row targets the same two words, and atomics on one address run
    // one after the other (measured: with one unconditional atomicMax per wave a 30-minute row took 3.5 ms whatever the dither,
    // 30 times a copy of its bytes; with one per workgroup of a grid of one workgroup per tile, every workgroup resident at the
    // start read 0 and fired, some 50 us per launch -- hence the capped grid).  The peak only grows, so a workgroup that reads a
    // value >= its own has nothing to add; a stale read costs a redundant atomic, never a wrong result.
    __shared__ int red[2 * (Q_THREADS / 64)];
    clipped = wave_sum(clipped);
    peak = wave_max(peak);
    if ((tid & 63) == 0) {
        red[2 * (tid >> 6)] = clipped;
        red[2 * (tid >> 6) + 1] = peak;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < Q_THREADS / 64; ++w) {
            clipped += red[2 * w];
            peak = max(peak, red[2 * w + 1]);
        }
        if (clipped) atomicAdd(a.result + 2 * r, clipped);
        if (peak > __hip_atomic_load(a.result + 2 * r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(a.result + 2 * r + 1, peak);
    }
}

template <int BITS, bool VEC>
void launch_quantize(int dither, dim3 grid, hipStream_t s, const QuantArgs& a) {
    if (dither == 0)
        hipLaunchKernelGGL((quantize_kernel<BITS, 0, VEC>), grid, dim3(Q_THREADS), 0, s, a);
    else if (dither == 1)
        hipLaunchKernelGGL((quantize_kernel<BITS, 1, VEC>), grid, dim3(Q_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL((quantize_kernel<BITS, 2, VEC>), grid, dim3(Q_THREADS), 0, s, a);
}

}  // namespace

extern "C" int vfx_quantize_rows_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max,
                                     const int64_t* n0, const int32_t* chan, int bits, int dither, uint64_t seed, void* out,
                                     int64_t out_stride, int32_t* result, vfx_stream_t stream) {
    if (!x || !n_rows || !out || !result || B < 0 || B > 65535 || n_max < 0 || (bits != 16 && bits != 24) || dither < 0 ||
        dither > 2 || x_stride < n_max || out_stride < n_max)
        return VFX_EINVAL;
    const long long tiles = (n_max + Q_TILE - 1) / Q_TILE;
    if (tiles > 0x7fffffffLL) return VFX_EINVAL;
    if (B == 0 || n_max == 0) return VFX_OK;
    hipStream_t s = (hipStream_t)stream;
    const int e = vfx_zero_u32(result, sizeof(int32_t) * 2 * (size_t)B, s);
    if (e != VFX_OK) return e;
    QuantArgs a;
    a.x = x;
    a.x_stride = x_stride;
    a.n_rows = n_rows;
    a.n_max = n_max;
    a.n0 = reinterpret_cast<const long long*>(n0);
    a.chan = chan;
    a.key = make_uint2((uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
    a.out = out;
    a.out_stride = out_stride;
    a.result = result;
    const uintptr_t omask = bits == 16 ? 7u : 15u;
    const bool vec = vfx_aligned16(x) && (B == 1 || (x_stride & 3) == 0) && (reinterpret_cast<uintptr_t>(out) & omask) == 0 &&
                     (B == 1 || (out_stride & 3) == 0);
    // at most ~Q_GRID workgroups per launch (eight per CU of an MI355X), each walking its row's tiles with that stride
    const long long per_row = Q_GRID / B > 0 ? Q_GRID / B : 1;
    const dim3 grid((unsigned)(tiles < per_row ? tiles : per_row), (unsigned)B);
    if (bits == 16)
        vec ? launch_quantize<16, true>(dither, grid, s, a) : launch_quantize<16, false>(dither, grid, s, a);
    else
        vec ? launch_quantize<24, true>(dither, grid, s, a) : launch_quantize<24, false>(dither, grid, s, a);
    VFX_LAUNCHED();
    return vfx_last_error();
}
