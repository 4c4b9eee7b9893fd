/*
 * vfx_hip.h -- C ABI of libvfx_hip.so, the MI355X (gfx950) kernel library behind
 * voicefixer_amd.VoiceFixer.restore()/restore_inmem() and Vocoder.forward()/oracle(), and of the stages between the restored
 * waveform and the file: rate conversion, loudness / true peak / limiter, and the word-length reduction to 16- or 24-bit PCM
 * (vfx_quantize_rows_f32), which -- when asked for -- takes the place of the reference's truncating int16 cast on the host.
 *
 * The reference (haoheliu/voicefixer) has no FFI: its hot path is a chain of stock torch
 * operators.  Each entry point below replaces the torch operator calls named in its
 * comment (paths relative to the reference root).  What a reference maintainer would bind
 * is shown in INTEGRATION.md (ctypes stubs).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. a torch tensor's
 *     data_ptr()), float32 unless stated, never retained after the call returns;
 *   - activations are channel-major: element (b, c, l) of a vfx_tensor lives at
 *     ptr[b*bstride + c*cstride + l*lstride] (strides in ELEMENTS). Inputs of the conv
 *     family need lstride == 1, cstride % 4 == 0 and a 16-byte aligned ptr;
 *   - 2-D feature maps (B,C,H,W) are stored flattened with a power-of-two row pitch
 *     P = W+1: element (h, w) at l = h*P + w; column P-1 is a structural zero that serves
 *     as left/right zero padding for 3x3 convolutions (the UNet works on W = 127, 63, ...
 *     1 mel bins, so P = 128, 64, ... 2);
 *   - all launches go to `stream` (a hipStream_t passed as void*), no internal
 *     synchronisation, no allocation; thread-safe for distinct streams;
 *   - return 0 on success, a negative VFX_E* code for bad arguments, or a positive
 *     hipError_t from the launch.  Nothing throws.
 */
#ifndef VFX_HIP_H
#define VFX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vfx_stream_t; /* hipStream_t */

#define VFX_OK 0
#define VFX_EINVAL (-1)   /* bad argument / unsupported shape */
#define VFX_EALIGN (-2)   /* pointer or stride alignment */
#define VFX_ERANGE (-3)   /* tile bookkeeping overflow (tap span too large for the tile) */
#define VFX_ENOTSUP (-4)  /* valid arguments, but a shape / activation this entry point does not take (vfx_conv1d_f16):
                             the caller runs the launch on the fp32 entry point instead */

typedef struct {
    void* ptr;
    int64_t bstride, cstride, lstride; /* element strides */
    int64_t guard; /* INPUT tensors of the conv family: number of elements that may be READ (contents
                      arbitrary, they are masked) before l = 0 and after l = L-1 of every (b, c) row.
                      With a guard >= the largest tap offset + 8 every tile takes the branch-free
                      interior kernel; 0 is always legal (boundary tiles then run the general kernel). */
    const int32_t* rows; /* ragged batches (may be NULL): device int32[B], the VALID length of batch item b of this
                      tensor (<= the L / H*P argument of the call, which is then the row capacity).  As an INPUT of the
                      conv family, positions >= rows[b] are zero padding of the activated input (reflect padding
                      mirrors at rows[b]); outputs past a row's valid length are unspecified.  Lets utterances of
                      different lengths share one launch with results identical to separate launches. */
} vfx_tensor;

/* pre-activation applied to the INPUT while it is staged into LDS */
#define VFX_PRE_NONE 0
#define VFX_PRE_LRELU 1         /* leaky_relu(x, pre_slope) */
#define VFX_PRE_AFFINE_LRELU 2  /* leaky_relu(x*pre_scale[c] + pre_shift[c], pre_slope): eval BatchNorm + (leaky)ReLU */
/* post-activation applied in the epilogue, after bias and residual.  The kernels behind vfx_conv1d_f32, vfx_convtr1d_f32,
 * vfx_conv2d_f32 and vfx_convtr2d_3x3s2_f32 start their accumulators at ZERO (both arithmetics): bias, then residual, are added to
 * the finished sum of products, in the order torch adds them, so no partial sum rounds at their magnitude.  (The fused direct
 * ResStack layer of vfx_resblock_f32 without w1_wino4 still starts its halves at b1 and at b2 + x.) */
#define VFX_POST_NONE 0
#define VFX_POST_LRELU 1        /* leaky_relu(., post_slope) */
#define VFX_POST_ELU 2
#define VFX_POST_TANH 3
#define VFX_POST_SIGMOID 4
#define VFX_POST_LRELU_SNAKE 5  /* v = leaky_relu(., post_slope); v + sin(v)  (UpsampleNet prologue fused upstream) */

/* arithmetic of the contraction (per launch) */
#define VFX_MATH_F32 0     /* v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation (default) */
#define VFX_MATH_BF16X3 1  /* opt-in: every fp32 operand split into two bf16 terms, x*w evaluated as
                              xh*wh + xh*wl + xl*wh on v_mfma_f32_32x32x16_bf16 with fp32 accumulation
                              (relative product error <= 2^-15 (1 + 2^-19) in the worst case, ~2^-17 observed; bias and
                              residual are added to the finished sum); needs w_x3 and an input guard band
                              (vfx_tensor.guard >= largest tap offset + tile width), falls back to fp32
                              per launch for geometries the bf16x3 kernel does not cover (Cin % 32,
                              reflect padding, more than 3 taps other than 3x3, mixed tap counts) */

typedef struct {
    int pre_act;
    float pre_slope;
    const float* pre_scale; /* [Cin] for VFX_PRE_AFFINE_LRELU */
    const float* pre_shift; /* [Cin] */
    int post_act;
    float post_slope;
    int math;               /* VFX_MATH_* */
    const void* w_x3;       /* VFX_MATH_BF16X3: the packed weights as bf16 (hi, lo) planes, layout
                               [slab][Cin/16][plane][k-half][Cout][8] (voicefixer_amd/packing.py::pack_x3) */
    const float* w_direct;  /* optional (may be NULL): the same fp32 weights packed [slab][CinPad/8][Cout][8], the 8
                               channels of a group in the order 0,2,4,6,1,3,5,7 (packing.py::pack_direct).  Lets 1-D
                               launches with 2-3 taps, zero padding, a guard band and no BatchNorm pre-activation run
                               on convw_kernel (weights read from L2 as MFMA A-operand vectors, activations staged
                               16-32 channels deep); bit-identical results are NOT implied (other summation order
                               within fp32 rounding).  Everything else, and small launches, use w_packed. */
    const float* w_wino4;   /* optional (may be NULL), k = 3 stride-1 Conv1d: the Winograd F(4,3) transform of the three tap
                               slabs, six slabs U = G w packed like w_direct (packing.py::pack_wino4).  Large launches (>=
                               512 workgroups) with Cin % 32 == 0, Cout % 64 == 0, zero padding and no BatchNorm
                               pre-activation then run on convwg4_kernel: four outputs a dilation apart share six
                               products instead of twelve (2x fewer fp32 MFMAs than the direct sum; rounding ~3x the
                               direct sum's, ~1e-6 relative, relative to the LARGEST operand of a quad's six-tap window:
                               profiles/r03_winograd_error_sweep.txt).  For vfx_conv2d_f32 with ksize 3: the transform
                               along the kernel's ROW axis for each kernel column, 18 slabs kx*6 + plane
                               (packing.py::pack_wino4_2d); launches with Cout % 64 == 0 and Cin % 32 == 0, or Cout % 32
                               == 0 and Cin % 16 == 0, on maps of pitch <= 64 / 128 run on convwg4s_kernel (four
                               vertically adjacent outputs share 18 products instead of 36).  For vfx_convtr1d_f32: the
                               Winograd F(3,2) transform along the INPUT axis for every output phase r of the polyphase
                               form (out[q s + r - pad] = w[r + s] x[q - 1] + w[r] x[q]) as ONE blob
                               [4 planes][Cin/8][s Cout][8] whose row c s + r is (channel c, phase r), phase fastest
                               (packing.py::pack_wino32_tr; a blob in the earlier [4 r + plane][Cin/8][Cout][8] order
                               gives wrong results, there is no way to tell the two apart); launches of >= 512 workgroups with Cin % 32 == 0, Cout % 64
                               == 0, stride <= 32 and no activation run on convtw_kernel: three consecutive q of a phase share four
                               products instead of six (transform constants 1 and 1/2: rounding as the direct sum's; the bias is
                               added after the output transform). */
} vfx_act;

#define VFX_PAD_ZERO 0
#define VFX_PAD_REFLECT 1

int vfx_version(void);

/* 16 hex digits: sha256 over every source file this library was built from (csrc/Makefile: BUILD_ID).  Measurement
 * records (bench.py, profiles/ PMC summaries) carry it so that a profile can be tied to the library that produced it. */
const char* vfx_build_id(void);

/* Number of hipLaunchKernel calls issued by this library in this process (test hook:
 * proves the HIP path, not a fallback, produced a result). */
uint64_t vfx_launch_count(void);

/* Kernel family chosen by the most recent conv-family launch of the calling thread, encoded
 * BM*100000 + BL*100 + code (bench.py's roofline bookkeeping maps it to the template instances a profiler shows):
 *   code 4 / 8        conv_taps_kernel<BM,BL,*,*,KC=code,...>   (first-generation kernel: small launches, reflect
 *                     padding, 1x1 / transposed 2-D convolutions, split-K)
 *   code 16           conv_x3_kernel<BM,BL,...>                  (opt-in bf16x3 arithmetic)
 *   code 51 / 52 / 54 convw_kernel<BM,BL,*,*,NT=2|3,*,false>     (1-D, activation chunks of 8 / 16 / 32 channels)
 *   code 59           convw_kernel<BM,BL,*,*,NT=9,*,false>       (3x3 on a pitch map)
 *   code 61 / 62 / 64 convw_kernel<BM,BL,*,*,3,*,true>           (vfx_resblock_f32: direct sums, chunks of 8 / 16 / 32 channels)
 *   code 71 / 72 / 74 convw_kernel<BM,BL,*,*,3,*,2>              (vfx_resblock_f32 with w2_wino: second half as Winograd F(2,3))
 *   code 91 / 92 / 94 convw_kernel<BM,BL,*,*,3,*,3>              (vfx_resblock_f32 with w2_wino4: second half as Winograd F(4,3))
 *   code 96           resblk4_kernel                             (vfx_resblock_f32 with w1_wino4 + w2_wino4: both halves F(4,3))
 *   code 97           resblk4s_kernel                            (vfx_resblock_wino4_f32 at a dilation resblk4_kernel does not take:
 *                     both halves F(4,3) on a strip tile)
 *   code 80           convwg4_kernel<..>                          (Winograd F(4,3), 1-D), BL = output positions
 *   code 81           convwg4p_kernel<..>                         (the same tile on persistent workgroups: the two long launches of a
 *                     ResStack layer, tap / staging / weight pipeline running across tiles)
 *   code 82           convwg4x_kernel<..>                         (the 128-channel convwg4_kernel tile with a 32 x 64 x 6 wave tile and a
 *                     deferred epilogue: the wide ResStack launches of large batches)
 *   code 83           convtw_kernel<..>                           (vfx_convtr1d_f32 as Winograd F(3,2) along the input axis,
 *                     BM = output channels x BL = 3 * positions per phase)
 *   code 88           convwg4s_kernel<..>                         (Winograd F(4,3), 3x3 on a pitch map, kernel columns share one tile)
 *   code 32           convh_kernel                                (opt-in f16 arithmetic, vfx_conv1d_f16: direct sum on
 *                     v_mfma_f32_32x32x16_f16, BM = 128 output channels x BL = 128 positions) */
int vfx_last_conv_tile(void);

/* ---- convolution family: implicit GEMM on v_mfma_f32_32x32x2_f32 -------------------
 * Weights are pre-packed on the host as [slab][CinPad][Cout] (Cout contiguous), where a
 * slab is one kernel tap, CinPad = Cin rounded up to 8 (zero filled).  See
 * voicefixer_amd/packing.py.  bias may be NULL; res may be NULL.                      */

/* y[b,n,l] = post( bias[n] + res[b,n,l] + sum_{c,t} w[t][c][n] * pre(x[b,c,l+(t-(k-1)/2)*dil]) )
 * Replaces torch conv1d (+ leaky_relu / ELU / tanh / ReflectionPad1d around it) in
 * voicefixer/vocoder/model/generator.py:33-54,74-76,95-99 and modules.py:549-576
 * (ResStack), and torch linear in voicefixer/restorer/model.py:69-99 (k = 1).
 * Cout % 32 == 0; for Cout == 1 use vfx_conv1d_cout1_f32. */
int vfx_conv1d_f32(const vfx_tensor* x, const float* w_packed, const float* bias,
                   const vfx_tensor* res, const vfx_tensor* y, int B, int Cin, int Cout, int L,
                   int k, int dilation, int pad_mode, const vfx_act* act, vfx_stream_t stream);

/* Opt-in f16 arithmetic for the k = 3 dilated Conv1d of the wide ResStack layers (C = Cin = Cout in {128, 256, 512}):
 *   y[b,n,l] = post( bias[n] + res[b,n,l] + sum_{c,t} f16(w[n][c][t]) * f16(pre(x[b,c,l+(t-1)*dil])) )
 * with both operands rounded to fp16 (round to nearest even) and the products accumulated in fp32 (direct sum on
 * v_mfma_f32_32x32x16_f16); pre-activation, bias, residual and post-activation are fp32.  Zero padding.
 * w_f16: fp16 weights [3][C/8][C][8], element [t][c8][n][e] = w[n][8 c8 + e][t] (packing.py::pack_f16).
 * act: pre_act VFX_PRE_NONE / VFX_PRE_LRELU, post_act VFX_POST_NONE / LRELU / LRELU_SNAKE (math and the weight
 * fields are ignored); NULL = no activation.  x, res and y need lstride 1; x is read only inside [0, row length)
 * (guard 0 is legal; x->rows honoured as in vfx_conv1d_f32); res may alias y (in-place residual update), x may not.
 * range_flag (device int32, may be NULL): set to nonzero when a staged activation operand is not finite or exceeds
 * the fp16 range (|v| > 65504); y is then unspecified (the caller re-runs in fp32).  The flag is never cleared here.
 * Returns VFX_ENOTSUP for a C, activation or layout it does not take. */
int vfx_conv1d_f16(const vfx_tensor* x, const void* w_f16, const float* bias, const vfx_tensor* res,
                   const vfx_tensor* y, int B, int C, int L, int dilation, const vfx_act* act, int32_t* range_flag,
                   vfx_stream_t stream);

/* One whole ResStack layer, fused (voicefixer/vocoder/model/modules.py:592-609, one iteration of the loop):
 *   y[b,n,l] = post( x[b,n,l] + bias2[n] + conv_k3_d1( lrelu_s( bias1 + conv_k3_dil( lrelu_s(x) ) ) )[b,n,l] )
 * for C = 64 or 128 channels.  The intermediate tensor lives in LDS (one tile of columns per workgroup), never in HBM.
 * x needs a guard band >= dilation + 264 (vfx_tensor.guard) unless resblk4_kernel takes the launch; y must NOT alias x
 * (a tile reads the input columns of its neighbours).  post_act as vfx_act.post_act.
 * Weights: both convolutions in the w_direct layout of vfx_act (required), and optionally their Winograd transforms --
 * the library picks the cheapest arithmetic the operands allow, results differ by fp32 rounding only:
 *   w2_wino   F(2,3) of the SECOND convolution (U0 = w0, U1 = (w0+w1+w2)/2, U2 = (w0-w1+w2)/2, U3 = w2, four slabs packed like
 *             w_direct, packing.py::pack_wino): its dilation-1 half forms 4 products per output pair instead of 6 on the LDS
 *             tile (C = 64 with the 256-column tile, C = 128);
 *   w2_wino4  F(4,3) of the second convolution (six slabs U = G w as vfx_act.w_wino4, packing.py::pack_wino4), C = 64 with
 *             16-byte aligned rows of x and y: 6 products per output QUAD instead of 12 (63 quads per 256-column tile; residual
 *             and stores move as 16-byte vectors);
 *   w1_wino4  F(4,3) of the FIRST (dilated) convolution, C = 64 together with w2_wino4 and a dilation whose blocks of 4 d
 *             positions fill a 256-column tile (d <= 32 with >= 48 of 64 quad columns used: the stage's d = 1, 3, 9, 27): BOTH
 *             halves form 6 products per four outputs (resblk4_kernel: the dilated half along the dilated axis, its output
 *             transform into the LDS tile; x needs no guard band there). */
typedef struct {
    const float* w1_direct;  /* required */
    const float* bias1;      /* may be NULL */
    const float* w2_direct;  /* required */
    const float* bias2;      /* may be NULL */
    const float* w2_wino;    /* optional */
    const float* w2_wino4;   /* optional */
    const float* w1_wino4;   /* optional */
} vfx_resblock_w;
int vfx_resblock_f32(const vfx_tensor* x, const vfx_tensor* y, const vfx_resblock_w* w, int B, int C, int L,
                     int dilation, float slope, int post_act, float post_slope, vfx_stream_t stream);

/* The same layer with both convolutions as Winograd F(4,3) at EVERY dilation, one launch: resblk4_kernel where
 * vfx_resblock_f32 would take it (d = 1, 3, 9, 27), resblk4s_kernel (a strip tile: a workgroup owns one or two
 * sub-ranges of a block of 4 d positions, the four strips a dilation apart) everywhere else.  C = 64; w1_wino4 and
 * w2_wino4 required (the direct and F(2,3) weights are not read); rows of x and y 16-byte aligned with lstride 1; y must
 * not alias x; x needs no guard band.  Returns VFX_ENOTSUP for anything else (the caller picks another form). */
int vfx_resblock_wino4_f32(const vfx_tensor* x, const vfx_tensor* y, const vfx_resblock_w* w, int B, int C, int L,
                           int dilation, float slope, int post_act, float post_slope, vfx_stream_t stream);

/* ConvTranspose1d(Cin, Cout, kernel 2s, stride s, padding s/2 + s%2, output_padding s%2):
 * Lin -> s*Lin.  Polyphase: s phases x 2 taps.  w_packed = [2s][CinPad][Cout], slab k is
 * kernel tap k.  Replaces voicefixer/vocoder/model/modules.py:449-459,519 (UpsampleNet.layer).
 * stride 1 .. 8; a launch that convtw_kernel takes (vfx_act.w_wino4) may have a stride up to 32.  VFX_EINVAL for any other
 * stride, nothing launched. */
int vfx_convtr1d_f32(const vfx_tensor* x, const float* w_packed, const float* bias,
                     const vfx_tensor* y, int B, int Cin, int Cout, int Lin, int stride,
                     const vfx_act* act, vfx_stream_t stream);

/* Conv2d ksize x ksize (ksize 1 or 3, padding ksize/2, stride 1) on pitch-P maps, P = 1<<pitch_log2,
 * W = P-1.  w_packed = [ksize*ksize][CinPad][Cout], slab ky*ksize+kx.  Output pad column is
 * written as zero.  Replaces voicefixer/restorer/modules.py:18-26,33-41,47-53 (ConvBlockRes). */
int vfx_conv2d_f32(const vfx_tensor* x, const float* w_packed, const float* bias,
                   const vfx_tensor* res, const vfx_tensor* y, int B, int Cin, int Cout, int H,
                   int pitch_log2, int ksize, const vfx_act* act, vfx_stream_t stream);

/* ConvTranspose2d 3x3 stride 2 padding 0 followed by the reference's prune of the last
 * output row: (h, w=P-1) -> (2h, 2w+1) on pitch 2P.  w_packed = [9][CinPad][Cout], slab
 * ky*3+kx.  Replaces voicefixer/restorer/modules.py:112-121,141-150 (DecoderBlockRes). */
int vfx_convtr2d_3x3s2_f32(const vfx_tensor* x, const float* w_packed, const vfx_tensor* y,
                           int B, int Cin, int Cout, int h, int in_pitch_log2,
                           const vfx_act* act, vfx_stream_t stream);

/* Cout == 1 convolution (channel reduction, HBM-bound): y[b,0,l] = post(bias + sum w[c][t] * x[b,c,l+t-(k-1)/2]),
 * w = [Cin][k].  Replaces the final ReflectionPad1d(3)+Conv1d(64,1,7)+Tanh
 * (generator.py:95-99) and UNet after_conv2 1x1 (restorer/model_kqq_bn.py:119-126,174). */
int vfx_conv1d_cout1_f32(const vfx_tensor* x, const float* w, const float* bias,
                         const vfx_tensor* y, int B, int Cin, int L, int k, int pad_mode,
                         int post_act, int out_mask_log2, vfx_stream_t stream);

/* avg_pool2d(2,2) (floor) on pitch maps: (H, P) -> (H/2, P/2).
 * Replaces voicefixer/restorer/modules.py:103. */
int vfx_avgpool2x2_f32(const vfx_tensor* x, const vfx_tensor* y, int B, int C, int H,
                       int pitch_log2, vfx_stream_t stream);

/* ---- analysis front-end ---------------------------------------------------------- */

/* One-time upload of the tables used by vfx_stft_mel_f32: periodic hann window [2048],
 * twiddles exp(-2*pi*i*m/2048) m<1024 as interleaved (re,im) [2048], and the banded mel
 * filterbank: lo[128], hi[128] (inclusive bin range), off[128] (start into coef), coef[nnz].
 * All HOST pointers; the library keeps device copies. */
int vfx_frontend_init(const float* window, const float* twiddle, const int32_t* lo,
                      const int32_t* hi, const int32_t* off, const float* coef, int nnz);

/* Test hook: copy the banded filterbank the kernels read back to HOST buffers lo/hi/off[128], coef[coef_capacity]
 * (which = 0: the HTK table of vfx_stft_mel_f32, 1: the slaney table of vfx_stft_mel_oracle_f32); *nnz_out = number
 * of coefficients.  Lets a test assert the mel bin indexing bit-exactly on what the device holds (the reference's
 * matrix is voicefixer/tools/mel_scale.py:147-238).  Tables are kept per device (the caller's current device). */
int vfx_frontend_readback(int which, int32_t* lo, int32_t* hi, int32_t* off, float* coef, int coef_capacity,
                          int* nnz_out);

/* wav [B][N] (row stride wav_stride) -> mel [B][T][128], T = 1 + N/441.  Reflect-padded,
 * centred STFT (n_fft 2048, hop 441), |.| with the 1e-8 power clamp, banded HTK mel.
 * The 1025-bin spectrogram never leaves LDS.  N >= 1025.
 * Replaces voicefixer/base.py:78-85 (_pre): fDomainHelper.py:81-110 + mel_scale.py:63-77. */
int vfx_stft_mel_f32(const float* wav, int64_t wav_stride, int B, int N, float* mel,
                     vfx_stream_t stream);

/* The same for rows of DIFFERENT sample counts n_rows[b] (device int32[B], each >= 1025): row b gets its own
 * 1 + n_rows[b]/441 frames, T is the row pitch of mel (>= every row's frame count).  Pair with vfx_post_rows_f32. */
int vfx_stft_mel_rows_f32(const float* wav, int64_t wav_stride, int B, const int32_t* n_rows, int T, float* mel,
                          vfx_stream_t stream);

/* Vocoder.oracle front-end on the device (voicefixer/vocoder/base.py:61-71): peak[b] = max|wav[b]|
 * (vfx_peak_f32, float bits in a uint32), then |librosa.stft(wav/peak)| (n_fft 2048, hop 441, zero
 * "constant" padding, no clamp) and the slaney-normalised HTK filterbank of librosa.filters.mel,
 * uploaded once in banded form by vfx_frontend_init_oracle -> mel [B][T][128].  Follow with
 * vfx_mel_to_cond_ex_f32(apply_weight = 0). */
int vfx_frontend_init_oracle(const int32_t* lo, const int32_t* hi, const int32_t* off, const float* coef,
                             int nnz);
int vfx_peak_f32(const float* y, int64_t y_bstride, int Ly, int B, uint32_t* peak, vfx_stream_t stream);
int vfx_stft_mel_oracle_f32(const float* wav, int64_t wav_stride, int B, int N, const uint32_t* peak,
                            float* mel, vfx_stream_t stream);

/* mode-1 pre-filter, VoiceFixer.remove_higher_frequency (voicefixer/base.py:87-104): STFT 2048/512
 * (periodic hann, centred, zero padding) -> per-bin clipped log10 energy -> cut-off bin at `ratio`
 * of the cumulative energy -> bins >= cut-off zeroed -> ISTFT (overlap-add, window-sum-square
 * normalisation).  wav [B][N] -> out [B][512*(N/512)].  workspace: vfx_hf_workspace_bytes(B, N)
 * device bytes, 16-byte aligned.  cutoff_out (device, B int32, may be NULL) receives the cut-off
 * bin index of every utterance.  Needs vfx_frontend_init (window, twiddles). */
size_t vfx_hf_workspace_bytes(int B, int N);
int vfx_hf_cut_f32(const float* wav, int64_t wav_stride, int B, int N, float* out, int64_t out_stride,
                   float ratio, void* workspace, size_t workspace_bytes, int32_t* cutoff_out,
                   vfx_stream_t stream);

/* (B,T,128) frame-major <-> channel-major (B,128,ld) transposes used around the denoiser. */
int vfx_tm_to_cm_f32(const float* src, float* dst, int B, int T, int C, int64_t dst_bstride,
                     int64_t dst_cstride, vfx_stream_t stream);

/* clean = mask*mel; x = log10(max(clean,1e-8)); U = [log10(max(mel,1e-8)), x] written as the
 * UNet input (B,nch>=2,Tp*128) pitch map (channels >= 2 are zero filler so the first conv has no
 * channel tail) with bin 127 and rows >= T zero.  mask is channel-major
 * (B,128,*).  Ragged batches: mask->rows[b] = frames of row b (T is then the frame pitch of mel; rows from
 * mask->rows[b] on are zero).  Replaces voicefixer/restorer/model.py:105-108 + model_kqq_bn.py:145-151. */
int vfx_unet_input_f32(const float* mel, const vfx_tensor* mask, const vfx_tensor* unet_in, int nch,
                       int B, int T, int Tp, vfx_stream_t stream);

/* logmel = unet_out + x, x = log10(max(mask*mel,1e-8)); the UNet never sees mel bin 127 and
 * emits 0 there (model_kqq_bn.py:151,177), so logmel[...,127] = x[...,127] is recomputed from
 * mel and mask.  denoised = 10^min(logmel,5).  Both outputs are (B,T,128) frame-major.
 * Replaces restorer/model.py:112 + voicefixer/base.py:125 (from_log). */
int vfx_unet_output_f32(const vfx_tensor* unet_out, const vfx_tensor* unet_in, const float* mel,
                        const vfx_tensor* mask, float* logmel, float* denoised, int B, int T,
                        int Tp, vfx_stream_t stream);

/* One bidirectional GRU layer, hidden 256, PyTorch gate order (r,z,n), h0 = 0: the recurrent
 * part.  gi = x-projections incl. b_ih, frame-major (B,T,1536) = [fwd r,z,n | bwd r,z,n].
 * whh_packed = W_hh of both directions in the layout of voicefixer_amd/packing.py::pack_gru_whh
 * (per direction: register-resident rows, LDS-resident rows, L2-streamed rows; the split is
 * reported by vfx_gru_layout).  bhh = [2][768].  out is channel-major (B,512,*): fwd in channels
 * 0..255, bwd in 256..511.  Ragged batches: out->rows[b] = frames of sequence b (T is then the frame pitch of gi; the
 * reverse direction starts at frame rows[b]-1, frames >= rows[b] of out are not written); same for vfx_gru_bidir2_f32.
 * Replaces the recurrent part of torch.nn.GRU in voicefixer/restorer/model.py:37-44,57-62. */
void vfx_gru_layout(int* kreg, int* klds, int* kstr);
int vfx_gru_bidir_f32(const float* gi, const float* whh_packed, const float* bhh,
                      const vfx_tensor* out, int B, int T, vfx_stream_t stream);

/* Same recurrence with every sequence owned by a PAIR of workgroups (one CU each) that keep W_hh
 * entirely in registers and exchange partial gate sums through tagged 8-byte granules: ~2x faster
 * per step, needs 4*B <= 240 workgroups to be co-resident (split larger batches).  whh_t = plain
 * [2][256][768] (W_hh transposed per direction); mailbox = B*24576 device bytes (zeroed by the call);
 * err_flag = device int32, set to 1 if a partner never answered (bounded spin, never hangs). */
int vfx_gru_bidir2_f32(const float* gi, const float* whh_t, const float* bhh, const vfx_tensor* out,
                       int B, int T, void* mailbox, size_t mailbox_bytes, int32_t* err_flag,
                       vfx_stream_t stream);

/* ---- synthesis front/back -------------------------------------------------------- */

/* mel (B,T,128) linear -> cond (B,128,T') channel-major, T' = T + T%2 + 4, tail = -4.0:
 * m/=18.8927416350036*exp(0.0269863588184314*k); S=20log10(max(1e-5,|m|))-20;
 * c=clip(8(S+115)/115-4,-4,4).  Replaces voicefixer/vocoder/base.py:51-54 +
 * model/util.py:8-36,69-80 + config.py:310-316. */
int vfx_mel_to_cond_f32(const float* mel, const vfx_tensor* cond, int B, int T,
                        vfx_stream_t stream);
/* same with the division by the analytic mel weights optional (0 for the Vocoder.oracle path,
 * whose mel is already slaney-normalised: vocoder/base.py:72 has no weight division) */
int vfx_mel_to_cond_ex_f32(const float* mel, const vfx_tensor* cond, int B, int T, int apply_weight,
                           vfx_stream_t stream);
/* ragged batches: t_rows (device int32[B], may be NULL) = frames of every row, T = row pitch of mel; row b is written
 * up to its own t_rows[b] + t_rows[b]%2 + 4 frames */
int vfx_mel_to_cond_rows_f32(const float* mel, const vfx_tensor* cond, int B, int T, const int32_t* t_rows,
                             int apply_weight, vfx_stream_t stream);

/* Per-utterance peak rule + centre trim (voicefixer/base.py:131-135, _trim_center :63-76):
 * peak[b] = max|y[b,:]|; out[b, 0:N] = y[b, d/2 : d/2+N] * (peak>1 ? 1/peak : 1), d = Ly-N.
 * peak_ws is a caller-provided device buffer of B uint32 words. */
int vfx_post_f32(const float* y, int64_t y_bstride, int Ly, float* out, int64_t out_bstride,
                 int N, int B, uint32_t* peak_ws, vfx_stream_t stream);

/* The same with per-row lengths (ragged batches): row b keeps n_rows[b] samples (device int32[B], every
 * n_rows[b] <= n_max) of its ly_rows[b] <= Ly vocoder samples (ly_rows NULL: every row has Ly), d = ly_rows[b] - n_rows[b];
 * the peak is taken over the row's own samples.  Columns >= n_rows[b] of out are left untouched. */
int vfx_post_rows_f32(const float* y, int64_t y_bstride, int Ly, const int32_t* ly_rows, float* out,
                      int64_t out_bstride, const int32_t* n_rows, int n_max, int B, uint32_t* peak_ws,
                      vfx_stream_t stream);

/* ---- rate conversion ---------------------------------------------------------------- */

/* Band-limited polyphase rate conversion of rows (what librosa.load(sr=44100) does inside the reference,
 * voicefixer/base.py:47-49; the same sum as the host resampler of include/vfx_audio.h, for B rows at once):
 *   y[r][m] = sum_i bank[p][i] * x[r][lo + i],  pos = c + m*down, kmax = pos / up, p = pos mod up, lo = kmax - J + 1,
 *   m < ny_r = ceil(n_rows[r] * up / down) (and < ny_max); x samples outside [0, n_rows[r]) count as zero.
 * bank: device float32 [up][J], phase p's J taps reversed (bank[p][i] = g[p + (J-1-i)*up], g = the L-tap zero-phase
 * low-pass scaled by up, zero past L; c = (L-1)/2): audio_io.polyphase_bank builds it.  x is [B][x_stride], y
 * [B][y_stride] (y_stride >= ny_max), n_rows device int32[B] (sample counts of x's rows, each <= x_stride).
 * row_index (device int32[n_index], may be NULL: then n_index == B and every row is converted) lists the rows ONE launch
 * converts -- a mixed-rate batch costs one launch per rate pair; rows not listed, and columns >= ny_r of listed rows,
 * are left untouched.  Positions are 64-bit (any row length).  Returns VFX_EINVAL on bad arguments. */
int vfx_resample_rows_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, const int32_t* row_index,
                          int n_index, const float* bank, int J, int up, int down, int c, float* y, int64_t y_stride,
                          int64_t ny_max, vfx_stream_t stream);

/* Outputs m in [m0, m1) of the polyphase sum of vfx_resample_rows_f32 for ONE row of n_total samples, of which the
 * caller holds only the window xw[k] = x[g0 + k], 0 <= k < wlen.  y[m - m0] receives output m; nothing else is written.
 * Samples outside [0, n_total) count as zero (n_total = INT64_MAX: the row's end is not yet known).  VFX_EINVAL, nothing
 * launched, unless the window covers every sample of [0, n_total) that any of the outputs reads:
 *   max(lo(m0), 0) >= g0   and   min(kmax(m1 - 1), n_total - 1) < g0 + wlen      (lo, kmax as in vfx_resample_rows_f32)
 * m0 == m1: VFX_OK, nothing launched.  All positions 64-bit.  Output m carries the same 32 bits vfx_resample_rows_f32
 * writes for output m of the whole row: the taps are clipped against [0, n_total), never against the window, so they
 * meet the same partial sums in the same order.  One launch. */
int vfx_resample_span_f32(const float* xw, int64_t g0, int64_t wlen, int64_t n_total, const float* bank, int J, int up,
                          int down, int c, int64_t m0, int64_t m1, float* y, vfx_stream_t stream);

/* out[k] = tail[k] * (1 - fade[k]) + head[k] * fade[k], 0 <= k < n: every operation rounded to fp32 on its own (no
 * contraction into an fma), so the result is the bits of numpy's float32  a * (1.0 - f) + b * f.  out may alias tail or
 * head.  n == 0: VFX_OK, nothing launched. */
int vfx_xfade_f32(const float* tail, const float* head, const float* fade, int64_t n, float* out, vfx_stream_t stream);

/* ---- loudness normalisation (ITU-R BS.1770-4; one channel per row -- programmes of several channels: further below) - */

/* Bytes of the workspace vfx_loudness_rows_f32 needs for B rows of at most n_max samples (0 on bad arguments). */
size_t vfx_loudness_workspace_bytes(int B, int64_t n_max, int hop, int S);

/* Integrated loudness L (LUFS) of B rows and, with a target, the normalising gain applied to them:
 *   K-weighting (shelf then high-pass biquad, coef = host float64[10]: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2, run
 *   in fp32), quarters of hop samples, 400 ms blocks of 4 quarters, absolute gate -70 LUFS, relative gate -10 LU;
 *   L = -inf when no block passes (silence, rows under 4 quarters).  g = min(10^((target - L)/20), 10^(ceiling_db/20) / P),
 *   P = max|x| of the row (a sample-peak ceiling); g = 1 when L = -inf; out = (float)g * x.
 * x is [B][x_stride] (x_stride >= n_max when B > 1), n_rows device int32[B] (each clamped to [0, n_max]).  The state of the
 * filter is carried across chunks of S samples (a multiple of 32, 32 <= S <= min(hop, 8192)) by an affine scan: mpow is
 * device float64[16][4][4], the powers M^(2^i) of the one-chunk state transition M = A^S; lookback (1..255) is the number
 * of preceding 256-chunk spans whose carry is summed (terms further back are negligible).  target NaN: measure only, out
 * may be NULL and nothing is applied; otherwise out ([B][out_stride], may be x itself) receives the first n_rows[r]
 * samples of every row and nothing past them.  result: device float64[B][3] = {L, g, P}.  ws: device workspace of
 * >= vfx_loudness_workspace_bytes bytes, 16-byte aligned.  At most 4 launches, no host synchronisation; VFX_EINVAL on bad
 * arguments (nothing launched). */
int vfx_loudness_rows_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max,
                          const double* coef, const double* mpow, int S, int hop, int lookback, double target,
                          double ceiling_db, float* out, int64_t out_stride, double* result, void* ws, size_t ws_bytes,
                          vfx_stream_t stream);

/* ---- true peak and loudness report (ITU-R BS.1770-4 Annex 2, EBU R 128 / Tech 3341 / Tech 3342) --------------------------- */

/* True peak TP of a row of n samples: the row is oversampled R times by the polyphase sum of vfx_resample_rows_f32 at
 * down = 1 and the largest magnitude is kept,
 *   y[m] = sum_i bank[p][i] * x[lo + i],  pos = c + m, kmax = pos / R, p = pos mod R, lo = kmax - J + 1,  m in [0, R*n),
 *   samples outside [0, n) count as zero;   TP = max(P, max_m |y[m]|),  P = max|x| (so TP >= P);   R = 1 or n = 0: TP = P.
 * bank: device float32 [R][J] in the layout of vfx_resample_rows_f32 (audio_io.polyphase_bank of the R-times
 * interpolator, c = (L-1)/2 its centre); 1 <= J <= 2048, R in {1, 2, 4}, 0 <= c < R*J.  y is never stored: one fused
 * kernel reduces |y| to one float per (row, tile of 1024 inputs), every output summed in one fixed order -- a row reads the
 * same bits alone and inside any batch; positions are 64-bit.
 *
 * Bytes vfx_loudness_tp_rows_f32 needs BEHIND the vfx_loudness_workspace_bytes(B, n_max, hop, S) bytes of the loudness
 * measurement, for B rows of at most n_max samples: B * (n_max/1024 + 2) floats, rounded (0 on bad arguments). */
size_t vfx_true_peak_workspace_bytes(int B, int64_t n_max, int R, int J);

/* vfx_loudness_rows_f32 with a TRUE-peak ceiling: the same arguments, measurement and bits of L and P, plus bank, J, R, c
 * (above);  g = min(10^((target - L)/20), 10^(ceiling_db/20) / TP) (1 when L = -inf), ceiling_db read as dBTP;
 * result: device float64[B][4] = {L, g, P, TP}.  target NaN: measure only.  ws: >= vfx_loudness_workspace_bytes(B, n_max,
 * hop, S) + vfx_true_peak_workspace_bytes(B, n_max, R, J) bytes, 16-byte aligned.  Exactly one launch more than
 * vfx_loudness_rows_f32 with the same arguments when R > 1 and n_max > 0 (the oversampling kernel; its partials are
 * folded by the gate kernel), none more when R = 1; no host synchronisation.  Nothing is read past a row's length and
 * nothing written outside ws, result and the rows of out.  VFX_EINVAL on bad arguments (nothing launched): those of
 * vfx_loudness_rows_f32, a NULL bank, J or c out of range, R not in {1, 2, 4}, ws too small. */
int vfx_loudness_tp_rows_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max,
                             const double* coef, const double* mpow, int S, int hop, int lookback, double target,
                             double ceiling_db, const float* bank, int J, int R, int c, float* out, int64_t out_stride,
                             double* result, void* ws, size_t ws_bytes, vfx_stream_t stream);

/* Bytes of the WHOLE workspace of vfx_loudness_report_rows_f32 (0 on bad arguments). */
size_t vfx_loudness_report_workspace_bytes(int B, int64_t n_max, int hop, int S, int R, int J);

/* Loudness report of B rows (measure only): report is device float64[B][6] = {L, LRA, Mmax, Smax, P, TP}.
 *   L, P, TP: as vfx_loudness_tp_rows_f32 (the same bits).
 *   Mmax: the largest momentary loudness -0.691 + 10 log10 z_j over ALL 400 ms blocks (ungated); -inf without a block.
 *   Short-term blocks: 30 consecutive quarters from every quarter j in [0, nq - 30], e_j = their energy / (30 hop);
 *   Smax: the largest -0.691 + 10 log10 e_j; -inf without a block.
 *   LRA (EBU Tech 3342): of the short-term values above -70 LUFS, those above the loudness of their mean energy - 20 LU,
 *   sorted ascending (n values s[]): s[((n-1)*95 + 50) / 100] - s[((n-1) + 5) / 10] (integer division); 0 when n = 0.
 * One launch more than vfx_loudness_tp_rows_f32 measuring only: one workgroup per row selects the two order statistics
 * by counting over the float64 bit patterns (64 passes each, any row length), fixed-order reductions throughout.
 * VFX_EINVAL on bad arguments (nothing launched). */
int vfx_loudness_report_rows_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max,
                                 const double* coef, const double* mpow, int S, int hop, int lookback, const float* bank,
                                 int J, int R, int c, double* report, void* ws, size_t ws_bytes, vfx_stream_t stream);

/* ---- programmes of several channels (ITU-R BS.1770-4 with channel weights) -------------------------------- */

/* The B rows form G programmes of adjacent rows: group_start is device int32[G + 1], ascending, group_start[0] = 0,
 * group_start[G] = B; weight is device float64[B], the channel weight G_c >= 0 of every row.  The length of a programme is
 * n_rows of its FIRST row; the caller guarantees that its other rows have the same and that group_start is as described (if
 * the lengths differ, or group_start is not ascending from 0 to B -- overlapping programmes, rows in none -- the figures are
 * unspecified, but nothing is read or written outside ws, result and the rows of out: the kernels clamp it into [0, B]).  With q_{c,i} the quarter sums of
 * row c (vfx_loudness_rows_f32),
 *   z_j = (sum_c G_c * (q_{c,j} + q_{c,j+1} + q_{c,j+2} + q_{c,j+3})) * 1/(4 hop),   rows in ascending order, fp64
 * (one row of weight 1.0: the bits of the per-row z_j), gates and L as vfx_loudness_rows_f32 on these z_j;
 * P = max_c P_c, TP = max_c TP_c (rows of weight 0 included);  g = min(10^((target - L)/20), 10^(ceiling_db/20) / TP),
 * 1 when L = -inf;  out = (float)g * x for every row of the programme over that row's own n_rows -- ONE factor per programme.
 * result: device float64[G][4] = {L, g, P, TP}.  The chunk, filter and true-peak kernels run per row as they do for
 * vfx_loudness_tp_rows_f32; one workgroup per programme folds them in a fixed order, so a programme's result does not depend
 * on what else the call holds.  Exactly the launches of vfx_loudness_tp_rows_f32 with the same arguments; no host
 * synchronisation.  ws: >= vfx_loudness_groups_workspace_bytes bytes (the WHOLE workspace), 16-byte aligned.
 * VFX_EINVAL on bad arguments (nothing launched): G < 1, G > B, NULL group_start or weight, and everything
 * vfx_loudness_tp_rows_f32 rejects. */
size_t vfx_loudness_groups_workspace_bytes(int B, int64_t n_max, int hop, int S, int R, int J);
int vfx_loudness_groups_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max,
                            const int32_t* group_start, const double* weight, int G, const double* coef, const double* mpow,
                            int S, int hop, int lookback, double target, double ceiling_db, const float* bank, int J, int R,
                            int c, float* out, int64_t out_stride, double* result, void* ws, size_t ws_bytes,
                            vfx_stream_t stream);

/* Loudness report of G programmes (measure only): report is device float64[G][6] = {L, LRA, Mmax, Smax, P, TP}, the recipe
 * of vfx_loudness_report_rows_f32 on the programme quarter sums Q_i = sum_c G_c * q_{c,i} (ascending rows, fp64) and on the
 * z_j above; L, P, TP: the bits of vfx_loudness_groups_f32.  Exactly the launches of vfx_loudness_report_rows_f32. */
size_t vfx_loudness_report_groups_workspace_bytes(int B, int64_t n_max, int hop, int S, int R, int J);
int vfx_loudness_report_groups_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max,
                                   const int32_t* group_start, const double* weight, int G, const double* coef,
                                   const double* mpow, int S, int hop, int lookback, const float* bank, int J, int R, int c,
                                   double* report, void* ws, size_t ws_bytes, vfx_stream_t stream);

/* ---- look-ahead peak limiter behind the loudness measurement ------------------------------------------------- */

/* Bytes of the WHOLE workspace of vfx_loudness_limit_f32 (0 on bad arguments): the workspace of vfx_loudness_groups_f32 and, behind
 * it, 4 bytes per sample of the batch (the required gain) and a few values per row and per tile of 1024 samples. */
size_t vfx_loudness_limit_workspace_bytes(int B, int64_t n_max, int hop, int S, int R, int J);

/* Loudness normalisation with a look-ahead limiter in place of the static ceiling: the arguments of vfx_loudness_groups_f32
 * (G = 0 with NULL group_start and weight: every row is its own programme), then H, the look-ahead in samples (1..4096),
 * true_peak (1: the ceiling is a true-peak one; 0: a sample-peak one, nothing is oversampled, bank / J / R / c are checked but
 * not used) and result, device float64[G or B][8].  Per programme, with L, P, TP as vfx_loudness_groups_f32 measures them (the
 * same bits; TP = P when true_peak = 0 or R = 1), gL = 10^((target - L)/20) (1 when L = -inf) and Cl = 10^(ceiling_db/20):
 *   bound = Cl / TP < gL.  Not bound: out = (float)gL * x, the bits of vfx_loudness_groups_f32.
 *   bound: e[n] = max(|x[n]|, the R interpolated values in (n - 1, n]) (those behind the last sample go to n - 1), the
 *   maximum over the programme's rows;  c[n] = min(1, Cl / (gL e[n]));  m[n] = min c[j], |j - n| <= H inside the row;
 *   g[n] = 1 - sum_{|k| <= H} w[k] (1 - m[clamp(n + k)]),  w[k] = (1 + cos(pi k / (H + 1))) / (2 H + 2), summed in fp32 in
 *   ascending k;  v = ((float)gL * g[n]) * x;  TPv = the true peak of v (its sample peak when nothing is oversampled);
 *   t = min(1, Cl / TPv);  out = (float)t * v.
 * result = {L, gL, P, TP, bound (0 / 1), min g, t, TPv * t}; not bound: {L, gL, P, TP, 0, 1, 1, (float)gL * TP}.
 * out may be x itself (the same pointer and stride); any other overlap of the two batches is VFX_EINVAL.  A row gives the
 * same bits alone and in any batch.  Launches: those of vfx_loudness_groups_f32 measuring only, then 6 at R > 1 (row
 * parameters, envelope, limit, true peak of the limited rows, fold, trim) or 5 (R = 1 or true_peak = 0) -- the same number
 * whatever B and the lengths; no host synchronisation.  ws: >= vfx_loudness_limit_workspace_bytes(B, n_max, hop, S, R, J)
 * bytes (with R = 1 where true_peak = 0, if the smaller size is wanted), 16-byte aligned.
 * VFX_EINVAL on bad arguments (nothing launched): everything vfx_loudness_groups_f32 rejects (apart from G = 0 with both
 * pointers NULL), G or one pointer without the others, H outside [1, 4096], true_peak not 0 or 1, a NaN target, NULL out,
 * overlapping x and out, ws too small. */
int vfx_loudness_limit_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max,
                           const int32_t* group_start, const double* weight, int G, const double* coef, const double* mpow,
                           int S, int hop, int lookback, double target, double ceiling_db, const float* bank, int J, int R,
                           int c, float* out, int64_t out_stride, int H, int true_peak, double* result, void* ws,
                           size_t ws_bytes, vfx_stream_t stream);

/* ---- fixed-gain look-ahead limiter of a streaming session: the span form ------------------------------------- */

/* Bytes of the workspace of vfx_limit_span_f32 for spans of up to n_span outputs at look-ahead H (0 on bad arguments: n_span < 0
 * or > 2^30, H outside [1, 4096]): 4 bytes per output and per sample of the 4 H around the span, a few values per tile of 1024. */
size_t vfx_limit_span_workspace_bytes(int64_t n_span, int H);

/* Outputs [m0, m1) of the fixed-gain limiter F over ONE row of n_total samples (INT64_MAX: the row's end is not known yet) from
 * the window xw[k] = x[g0 + k], k < wlen; out[n - m0] receives output n.  F is the bound branch of vfx_loudness_limit_f32 with
 * a GIVEN gain and without the trim: gL = gain (linear, finite, > 0), Cl = 10^(ceiling_db/20), thr = (float)(Cl / gL),
 *   e[n] = max(|x[n]|, the R interpolated values in (n - 1, n]) (R = 1: |x[n]|; those behind the last sample go to n_total - 1,
 *   once n_total is known);  c[n] = e[n] > thr ? thr / e[n] : 1;  m[n] = min c[j], |j - n| <= H inside the row;
 *   g[n] = min(c[n], 1 - sum_{|k| <= H} w[k] (1 - m[clamp(n + k, 0, n_total - 1)])), fp32, ascending k (the exact sum never
 *   exceeds c[n]; the minimum takes the chain's rounding out, so that |out[n]| <= Cl to two roundings);  out = x * ((float)gL * g[n]).
 * Every value is a function of global positions, clipped and clamped against [0, n_total), never against the window: output n
 * has the bits the single span [0, n_total) writes for it, whatever the split, the window or g0.  While the end is unknown,
 * outputs below n_known - 2 H - Fw are final (n_known: the samples seen so far).  The window must cover
 *   [max(0, m0 - 2 H - Bk), min(n_total - 1, m1 - 1 + 2 H + Fw)],   Fw = c / R, Bk = J - 1 - c / R  (both 0 at R = 1),
 * and nothing outside the window is read.  bank / J / c: the R-phase interpolator of vfx_loudness_tp_rows_f32 (R = 1: not read,
 * may be NULL).  record: device float64[2] = {min g, max |out|} over [m0, m1).  ws: >= vfx_limit_span_workspace_bytes(m1 - m0,
 * H) bytes, 16-byte aligned.  Three launches (envelope, limit, fold) whatever the span; no host synchronisation.
 * An empty span (m0 == m1) is VFX_OK, launches nothing and leaves record alone (its value is {1, 0}).
 * VFX_EINVAL, nothing launched: a NULL xw, out, record or ws; g0, wlen, m0 < 0, m0 > m1, m1 > n_total, m1 - m0 > 2^30; a window
 * that does not cover the range above; H outside [1, 4096]; R not in {1, 2, 4}; at R > 1 a NULL bank, J outside [1, 2048] or c
 * outside [0, R J); a gain that is not finite and positive, a ceiling that is not finite; ws too small or misaligned; out
 * overlapping xw. */
int vfx_limit_span_f32(const float* xw, int64_t g0, int64_t wlen, int64_t n_total, int64_t m0, int64_t m1, double gain,
                       double ceiling_db, int H, const float* bank, int J, int R, int c, float* out, double* record, void* ws,
                       size_t ws_bytes, vfx_stream_t stream);

/* ---- streaming loudness leveller of a session: the span form (voicefixer_amd/loudness.py) ---------------------- */

#define VFX_LEVEL_STATE 64 /* float64 values of the caller's state */

/* Bytes of the workspace of vfx_level_span_f32 for spans of up to n_span outputs at quarters of hop samples (0 on bad arguments:
 * n_span < 0 or > 2^30, hop outside [400, 19200]): vfx_level_span_rows_workspace_bytes(n_span, hop, 1), 20 bytes per quarter of
 * the span and a few more -- ask for the size; the row runs the programme's kernels as a programme of one channel. */
size_t vfx_level_span_workspace_bytes(int64_t n_span, int hop);

/* Outputs [m0, m1) of the loudness leveller over ONE row of n_total samples at fs Hz (INT64_MAX: the row's end is not known yet)
 * from the window xw[k] = x[g0 + k], k < wlen; out[t - m0] receives output t.  hop = (fs + 5) / 10, Q = n_total / hop:
 *   E_q = the K-weighted energy (fp32 filter of coef, fp64 sum) of quarter q = [q hop, (q + 1) hop), the filter started from zero
 *         at sample max(0, (q - 2) hop);
 *   l_q = -0.691 + 10 log10(mean of E_j / hop over j in [q - 20, q + 9] within [0, Q)), q = 0..Q (ascending fp64 sum);
 *   G_q = clamp(target - l_q, -40, max_gain_db) where l_q > gate, else G_{q-1} (G_{-1} = 0; an empty or silent window holds);
 *   a_q = (float)10^(G_q / 20);  out[t] = x[t] * (a_q + (a_{q+1} - a_q) * ((float)(t - q hop) / (float)hop)) for t in quarter
 *   q < Q, fp32, every operation rounded once in this order;  out[t] = x[t] * a_Q for t >= Q hop.
 * Every value is a function of global positions: output t has the bits one call over the whole row writes for it, whatever the
 * split, the window or g0.  While the end is unknown, outputs below (n_known / hop - 10) hop are final (n_known = g0 + wlen).
 * Calls come IN ORDER: the first has m0 = 0 (which initialises state), every other the m1 of the one before, so that what a
 * call finds in state follows from m0: the anchors [0, na(m0)) evaluated, the energies [0, ne(m0)) computed,
 *   na(m) = m == 0 ? 0 : min(Q, (m - 1) / hop + 1) + 1,   ne(m) = m == 0 ? 0 : min(Q, na(m) + 9)   (Q = infinity while unknown).
 * The window must cover [m0, m1) and, when ne(m1) > ne(m0), [max(0, ne(m0) - 2) hop, ne(m1) hop); nothing else is read.
 * coef: the 10 K-weighting values of vfx_loudness_rows_f32 (host); S = 32 ceil(3 hop / 8192), mpow: device float64[8][16],
 * M^(2^i) of the zero-input transition M of S samples.  state: device float64[VFX_LEVEL_STATE], the caller's, one per row:
 *   [0] min G  [1] max G  [2] anchors evaluated  [3] anchors gated  [4] G of the last anchor  [5] energies computed
 *   [6] 1 once a call came out of order  [8..12) the last four a_q  [16..48) the last 32 E_j  -- [0..4) is the record, folded
 *   exactly over the calls.  ws: >= vfx_level_span_workspace_bytes(m1 - m0, hop) bytes, 16-byte aligned.
 * At most three launches (new quarters, anchors, apply); no host synchronisation.  An empty span is VFX_OK and launches nothing.
 * VFX_EINVAL, nothing launched: a NULL pointer; g0, wlen, m0 < 0, m0 > m1, m1 > n_total, m1 - m0 > 2^30; fs outside [4000, 192000];
 * S not the chunk length of fs; a coefficient that is not finite; target outside [-70, 0), max_gain_db outside [0, 40], gate
 * outside [-70, target); m1 beyond the ready bound while the end is unknown; a window that does not cover the ranges above; ws
 * too small or misaligned; out overlapping xw. */
int vfx_level_span_f32(const float* xw, int64_t g0, int64_t wlen, int64_t n_total, int64_t m0, int64_t m1, int fs,
                       const double* coef, const double* mpow, int S, double target, double max_gain_db, double gate,
                       double* state, float* out, void* ws, size_t ws_bytes, vfx_stream_t stream);

/* ---- the span stages of a session of several channels: ONE gain curve per programme ------------------------- */

/* Bytes of the workspace of vfx_limit_span_rows_f32 for spans of up to n_span outputs per channel at look-ahead H (0 on bad
 * arguments: those of vfx_limit_span_workspace_bytes, or C outside [1, 8]).  One envelope per programme: the size does not grow
 * with C. */
size_t vfx_limit_span_rows_workspace_bytes(int64_t n_span, int H, int C);

/* Outputs [m0, m1) of the LINKED fixed-gain limiter over a programme of C channels of n_total samples each: vfx_limit_span_f32
 * with the envelope e[n] = max over the channels of the per-channel envelope (|x_c[n]| and, at R > 1, its R interpolated values),
 * so that every channel is multiplied by the same float(gain) g[n].  Channel ch's window is xw + ch w_stride (wlen samples from
 * g0 of the row, as there), its outputs go to out + ch out_stride; g0, wlen, n_total, m0, m1 hold for every channel.  Every
 * output has the bits of the single span [0, n_total), whatever the split, the strides and the alignment; C = 1 gives the bits
 * and the record of vfx_limit_span_f32.  Ready rule, window coverage (per channel), bank / J / c, ws alignment: as there, with ws
 * >= vfx_limit_span_rows_workspace_bytes(m1 - m0, H, C).  Nothing outside a channel's window is read.  record: device float64[2]
 * = {min g, max |out| over all channels} over [m0, m1).  Three launches (envelope, limit, fold) whatever the span and C; no
 * host synchronisation.  An empty span is VFX_OK, launches nothing and leaves record alone.
 * VFX_EINVAL, nothing launched: everything vfx_limit_span_f32 refuses; C outside [1, 8]; w_stride < wlen; out_stride < m1 - m0;
 * the block of the outputs [out, out + (C - 1) out_stride + m1 - m0) overlapping the block of the windows
 * [xw, xw + (C - 1) w_stride + wlen). */
int vfx_limit_span_rows_f32(const float* xw, int64_t w_stride, int C, int64_t g0, int64_t wlen, int64_t n_total, int64_t m0,
                            int64_t m1, double gain, double ceiling_db, int H, const float* bank, int J, int R, int c, float* out,
                            int64_t out_stride, double* record, void* ws, size_t ws_bytes, vfx_stream_t stream);

/* Bytes of the workspace of vfx_level_span_rows_f32 (0 on bad arguments: those of vfx_level_span_workspace_bytes, or C outside
 * [1, 8]): 12 bytes per quarter of the span, and 8 more per quarter and channel. */
size_t vfx_level_span_rows_workspace_bytes(int64_t n_span, int hop, int C);

/* Outputs [m0, m1) of the LINKED loudness leveller over a programme of C channels: vfx_level_span_f32 with the quarter energy
 *   E_q = sum_c weight[c] E_{q,c}   (float64, c ascending from 0.0, every product and every sum rounded on its own),
 * E_{q,c} the quarter energy of channel c as defined there -- BS.1770-4's sum over the channels -- and the one ramp applied to
 * every channel.  Channel ch's window is xw + ch w_stride, its outputs go to out + ch out_stride.  weight: C HOST doubles,
 * finite and >= 0 (copied into the kernel arguments: nothing is uploaded).  state: ONE device float64[VFX_LEVEL_STATE] per
 * programme, laid out as there; it holds the linked energies.  Order of the calls, ready rule, window coverage (per channel),
 * coef / mpow / S: as there.  C = 1 with weight {1} gives the bits and the state of vfx_level_span_f32.  ws: >=
 * vfx_level_span_rows_workspace_bytes(m1 - m0, hop, C) bytes, 16-byte aligned.  At most three launches (new quarters of all
 * channels, anchors, apply) whatever C; no host synchronisation.  An empty span is VFX_OK and launches nothing.
 * VFX_EINVAL, nothing launched: everything vfx_level_span_f32 refuses; a NULL weight, or one that is not finite or < 0; C
 * outside [1, 8]; w_stride < wlen; out_stride < m1 - m0; the block of the outputs overlapping the block of the windows. */
int vfx_level_span_rows_f32(const float* xw, int64_t w_stride, int C, const double* weight, int64_t g0, int64_t wlen,
                            int64_t n_total, int64_t m0, int64_t m1, int fs, const double* coef, const double* mpow, int S,
                            double target, double max_gain_db, double gate, double* state, float* out, int64_t out_stride,
                            void* ws, size_t ws_bytes, vfx_stream_t stream);

/* ---- streaming loudness meter of a session: the span form and its report (voicefixer_amd/loudness.py) --------- */

#define VFX_METER_STATE 16 /* float64 values of the caller's state */

/* Bytes of the workspace of vfx_meter_span_rows_f32 for spans of up to n_span samples per channel at quarters of hop samples (0
 * on bad arguments: n_span < 0 or > 2^30, hop outside [400, 19200], C outside [1, 8]): 8 bytes per quarter of the span and
 * channel, 8 bytes per 1024 samples, and a few more. */
size_t vfx_meter_span_workspace_bytes(int64_t n_span, int hop, int C);

/* Folds the samples [m0, m1) of a programme of C channels of n_total samples each at fs Hz (INT64_MAX: the end is not known
 * yet) into the caller's meter: state and qlog.  Channel ch's window is xw + ch w_stride, xw[ch w_stride + k] = x_ch[g0 + k],
 * k < wlen; g0, wlen, n_total, m0, m1 hold for every channel.  hop = (fs + 5) / 10, nq(m) = m / hop.  After [0, m):
 *   qlog[q], q < nq(m) = sum_c weight[c] E_{q,c}   (float64, c ascending from 0.0, every product and every sum rounded on its
 *         own), E_{q,c} the quarter energy of vfx_level_span_f32: the linked quarter energy of vfx_level_span_rows_f32, bit for bit;
 *   state: [0] P = max_c max |x_c[n]|, n < m   [1] TP = max(P, the largest |y| among the interpolated values that BELONG to a
 *         sample n < m)   [2] quarters logged = nq(m)   [3] samples metered = m   [4] 1 once a call came out of order (sticky)
 *         [5..16) zero.  y: the R-phase interpolation of vfx_loudness_tp_rows_f32 (bank / J / c as there; R = 1: nothing is
 *         interpolated, TP = P, bank may be NULL); value (K, p) belongs to sample n = K - c / R, reads x[n - Bk .. n + Fw], Fw =
 *         c / R, Bk = J - 1 - c / R (both 0 at R = 1), and counts iff it lies in the row, by the tests of vfx_limit_span_f32's
 *         envelope.  The R - 1 values behind the last sample (n = n_total) are folded by the call with m1 == n_total, so that
 *         after it TP is the true peak of vfx_loudness_tp_rows_f32 over the whole programme, bit for bit.
 * Every value is a function of global positions and every fold is a maximum: state and qlog have the bits of one call over
 * the whole row, whatever the split, the window, g0, the stride or the alignment.  Calls come IN ORDER: the first has m0 = 0
 * (which initialises state; a zeroed state is that of a programme with nothing metered), every other the m1 of the one before; a
 * call out of order sets state[4] and stays inside its buffers.  Ready rule while the end is unknown: m1 <= n_known - Fw
 * (n_known = g0 + wlen).  Every channel's window must cover [max(0, m0 - Bk), min(n_total - 1, m1 - 1 + Fw)] and, when nq(m1) >
 * nq(m0), [max(0, nq(m0) - 2) hop, nq(m1) hop); nothing else is read.  weight: C HOST doubles, finite and >= 0.  coef / mpow / S:
 * as vfx_level_span_f32 takes them.  qlog: device float64[qcap], the caller's: 8 bytes per 100 ms of the programme.  ws: >=
 * vfx_meter_span_workspace_bytes(m1 - m0, hop, C) bytes, 16-byte aligned.  At most three launches (new quarters of all channels;
 * one {max |x|, max |y|} per tile of 1024 samples; the weighted sums and the fold, one workgroup), no float atomics, no host
 * synchronisation.  An empty span (m0 == m1) is VFX_OK and launches nothing.
 * VFX_EINVAL, nothing launched: a NULL xw, weight, coef, mpow, state, qlog or ws; g0, wlen, m0 < 0, m0 > m1, m1 > n_total, m1 -
 * m0 > 2^30; fs outside [4000, 192000]; S not the chunk length of fs; a coefficient that is not finite; a weight that is not
 * finite or < 0; C outside [1, 8]; w_stride < wlen; R not in {1, 2, 4}; at R > 1 a NULL bank, J outside [1, 2048] or c outside
 * [0, R J); qcap < 0 or nq(m1) > qcap; m1 beyond the ready bound while the end is unknown; a window that does not cover the
 * ranges above; ws too small or misaligned; state or qlog not 8-byte aligned. */
int vfx_meter_span_rows_f32(const float* xw, int64_t w_stride, int C, const double* weight, int64_t g0, int64_t wlen,
                            int64_t n_total, int64_t m0, int64_t m1, int fs, const double* coef, const double* mpow, int S,
                            const float* bank, int J, int R, int c, double* state, double* qlog, int64_t qcap, void* ws,
                            size_t ws_bytes, vfx_stream_t stream);

/* Bytes of the workspace of vfx_meter_report_f32 for a meter whose log holds `quarters` quarters (0 on a negative count): 8
 * bytes per quarter, at least 8.  Pass the log's capacity: ws_bytes / 8 is also the most quarters the report reads from qlog,
 * whatever state says. */
size_t vfx_meter_report_workspace_bytes(int64_t quarters);

/* The EBU R 128 figures of a meter: report (device float64[10]) = {integrated loudness L, loudness range, maximum momentary,
 * maximum short-term loudness, P, TP (both linear), momentary and short-term loudness of the LAST 4 / 30 quarters, quarters,
 * flag}, from state and qlog[0 .. state[2]) by the recipe of vfx_loudness_report_groups_f32 on these quarter sums: z_j = (q_j +
 * q_{j+1} + q_{j+2} + q_{j+3}) / (4 hop), L over the z_j that pass -70 LUFS and the relative gate 10 LU under their mean,
 * maximum momentary over ALL z_j; short-term energies (30 quarters, from every quarter) with the -70 LUFS / -20 LU gates and the
 * nearest-rank indices ((n - 1) + 5) / 10 and ((n - 1) 95 + 50) / 100, selected by counting over float64 bit patterns; fixed-order
 * reductions.  -inf: no block (LRA then 0.0).  One launch of one workgroup, which reads the log from memory; it writes report
 * and ws and NOTHING else, so a report in the middle of a session changes nothing that follows.  flag: state[4], or 2 where
 * state[2] is not a count that fits ws (ws_bytes / 8 quarters): the figures are then those of an empty log.
 * VFX_EINVAL, nothing launched: a NULL pointer; hop outside [400, 19200]; a pointer that is not 8-byte aligned; report overlapping
 * state. */
int vfx_meter_report_f32(const double* state, const double* qlog, int hop, double* report, void* ws, size_t ws_bytes,
                         vfx_stream_t stream);

/* ---- word-length reduction: 16- / 24-bit PCM with seeded dither (voicefixer_amd/wordlength.py) ----------------- */

/* The last stage of the output chain (the reference's save_wave truncates to int16 on the host, voicefixer/tools/wav.py:27-34;
 * this is the opt-in replacement): row r of x ([B][x_stride] float32, n_rows device int32[B], each clamped to [0, n_max])
 * becomes PCM of `bits` in {16, 24} bits.  With n = n0[r] + i the ABSOLUTE index of sample i in its file (n0: device int64[B],
 * each >= 0; NULL: all 0), c = chan[r] its channel (device int32[B], 0..7; NULL: all 0) and
 *   k_t(n) = (word n % 4 of Philox4x32-10(counter = ((n / 4) & 0xffffffff, (n / 4) >> 32, c, t), key = (seed & 0xffffffff,
 *            seed >> 32))) >> 8,   t in {0, 1},
 *   dither 0 (none): d = 0;   1 (tpdf): d = (k_0(n) - k_1(n)) * 2^-24;   2 (hp): d = (k_0(n) - k_0(n - 1)) * 2^-24, d(0) as tpdf,
 *   v = (double)x * 2^(bits-1) + d  (one float64 rounding);  NaN -> 0;
 *   q = clamp(rint(v), -2^(bits-1), 2^(bits-1) - 1)          (round half to even; saturates, never wraps),
 * the integers of voicefixer_amd/wordlength.py, bit for bit, whatever the batch, the alignment or the split of a row into calls.
 * out: int16 rows at bits == 16, int32 rows at 24, [B][out_stride] (strides in elements); the first n_rows[r] samples of every
 * row are written and nothing else.  result: device int32[B][2] = {clipped, peak}, overwritten: clipped counts the samples the
 * clamp changed or whose x was NaN, peak = max |q|.  Grid (tiles of 1024 samples, B), capped at about 2048 workgroups (a
 * workgroup then walks further tiles of its row); four consecutive samples per thread (one 16-byte load and one 8- / 16-byte store
 * when x, out and both strides allow it), float64 arithmetic, per-row counts by a wave reduction and at most one vector atomic of
 * each kind per workgroup.  One kernel behind one clear of result on the stream; no host synchronisation.
 * VFX_EINVAL, nothing launched: a NULL x, n_rows, out or result, B < 0 or > 65535, n_max < 0, bits not 16 or 24, dither not in
 * 0..2, x_stride or out_stride < n_max.  B == 0 or n_max == 0: VFX_OK, nothing launched. */
int vfx_quantize_rows_f32(const float* x, int64_t x_stride, const int32_t* n_rows, int B, int64_t n_max,
                          const int64_t* n0, const int32_t* chan, int bits, int dither, uint64_t seed, void* out,
                          int64_t out_stride, int32_t* result, vfx_stream_t stream);

/* ---- train-mode restorer (the reference's mode 2:restorer/model.py:69-99 and modules.py in .train()) --------------- */

/* BatchNorm batch statistics: per (batch row b, BN channel g) the mean and BIASED variance of a region of x, turned into
 * the affine of torch's train-mode batch_norm: scale[b*G+g] = gamma[g]/sqrt(var+eps), shift[b*G+g] = beta[g] - mean*scale.
 *   pitch_log2 in 1..7 (map form, G = C): channel c of a (B,C,L = H*P) pitch map, over the rows below x->rows[b] (an
 *                       element count, a multiple of P; NULL: all of L) and the first P-1 columns -- the spare column
 *                       P-1 never counts;
 *   pitch_log2 == 0    (1-D form, G = 1): all C channels of a (B,C,L) activation together, over positions < x->rows[b].
 * Guard slack and positions past a row's extent are never summed.  Two launches: per-chunk (count, mean, M2) partials
 * into ws (vfx_bn_stats_workspace_bytes(B,C,L,pitch_log2) bytes, 8-byte aligned), then a finalize that folds them in a
 * fixed order in fp64 -- bit-reproducible.  x needs lstride 1, a 16-byte aligned ptr, cstride/bstride % 4 == 0. */
size_t vfx_bn_stats_workspace_bytes(int B, int C, int L, int pitch_log2);
int vfx_bn_stats_f32(const vfx_tensor* x, int B, int C, int L, int pitch_log2, const float* gamma, const float* beta,
                     float eps, float* scale, float* shift, void* ws, size_t ws_bytes, vfx_stream_t stream);

/* y = act(x*scale[b*G+g] + shift[b*G+g]) over the positions below x->rows[b] (NULL: L) of every channel c, with g = c
 * (groups == C) or g = 0 (groups == 1); act VFX_POST_NONE or VFX_POST_LRELU(slope) (slope 0: ReLU).  Map form
 * (pitch_log2 > 0): column P-1 is written 0 (the structural zero of the 3x3 convolutions).  In place (y == x) or not;
 * y's positions past a row's extent are unspecified afterwards. */
int vfx_bn_apply_f32(const vfx_tensor* x, const vfx_tensor* y, int B, int C, int L, int pitch_log2, int groups,
                     const float* scale, const float* shift, int act, float slope, vfx_stream_t stream);

/* Seeded nn.Dropout(0.5), in place on a (B,C,T) channel-major activation (C % 4 == 0), positions below x->rows[b]
 * (NULL: T).  rowkey: device uint32[3*B] = (segment index, key lo, key hi) per row.  Element (t, c) of row b uses word
 * i % 4 of Philox4x32-10(counter = (i / 4, segment, layer, 0), key), i = t*C + c: dropped (0) if the word is < 2^31,
 * else kept x2.  relu != 0 applies max(.,0) afterwards.  Specification: voicefixer_amd/dropout.py. */
int vfx_dropout_f32(const vfx_tensor* x, int B, int C, int T, const uint32_t* rowkey, int layer, int relu,
                    vfx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VFX_HIP_H */
