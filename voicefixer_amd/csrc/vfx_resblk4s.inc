// vfx_resblk4s.inc -- included by vfx_conv.hip after vfx_resblk4.inc.
//
// resblk4s_kernel: one whole C = 64 ResStack layer for ANY dilation, both convolutions as Winograd F(4,3) and the intermediate
// tile in LDS -- resblk4_kernel (vfx_resblk4.inc) on a strip tile, for the dilations whose blocks of 4d positions do not fit its
// 256 columns (the stage's d = 81, 243, 729, 2187).
//
// Tile geometry.  A first-half quad {p, p + d, p + 2d, p + 3d} may start at any position p.  Positions are q = 4d blk + i d + r
// (0 <= r < d, strip i = 0..3 of block blk); a SEGMENT is a sub-range r in [r0, r0 + W) of one block, W = P - 4, P = 64 or 32 (the
// host picks the one that wastes fewer columns at this d).  A workgroup owns G = 64 / P consecutive segments of the row (segment n
// = G bx + g; blk = n / nseg, r0 = (n % nseg) W, nseg = ceil(d / W) segments per block):
//   first half:  for every segment the W + 2 quads starting at p = 4d blk + r0 - 1 + j (j < W + 2) -- the same 64 quad columns
//                x 64 channels as resblk4_kernel, with the same staging and MFMAs; their output transform goes to the Y strip
//                4 g + i at column j (Y[64][4 G P] natural order within each strip; strip pitch P);
//   second half: every strip turns into W outputs (W / 4 quads of consecutive positions, the ±1 halo is the only recomputed
//                work); 64 quad lanes = 4 G strips x W / 4 quads (60 / 56 used).
// Outputs with r >= d belong to the next strip's first segment and are not written; nor is anything past the row's end.  The
// output quads start at 4d blk + i d + r0 + 4 jq, not 16-byte aligned in general (d is odd): residual loads and stores are
// unaligned dwordx4 buffer accesses (legal on gfx950, DESIGN.md 3.0), the partly owned quads go element by element.
// Column use (outputs per quad lane of one half): d = 81 P = 32: 81 / 96 = 0.84; d = 243 P = 32: 243 / 288 = 0.84; d = 729 P = 64:
// 729 / 832 = 0.88; d = 2187 P = 64: 2187 / 2368 = 0.92.
// Tap sharing: tile (blk, r0) reads the strips -1 .. 4 of its block, i.e. strip 3 of block blk - 1 and strip 0 of blk + 1: the
// tiles a row's nseg segments apart share taps; the XCD-aware order (convw_grid_x) keeps them on one XCD within one residency
// round, so that overlap is read from L2.
// The body is resblk4_kernel's (resblk4_body<true>, vfx_resblk4.inc): only the tile geometry differs.
__global__ __launch_bounds__(256, 2) void resblk4s_kernel(const ConvArgs a) { resblk4_body<true>(a); }

// vfx_resblock_wino4_f32 (include/vfx_hip.h): one C = 64 ResStack layer, both halves F(4,3), one launch at every dilation.
extern "C" int vfx_resblock_wino4_f32(const vfx_tensor* x, const vfx_tensor* y, const vfx_resblock_w* w, int B, int C, int L,
                                      int dilation, float slope, int post_act, float post_slope, vfx_stream_t stream) {
    if (!w) return VFX_EINVAL;
    if (!resblk4_args_ok(x, y, w, B, C, L, dilation, slope, post_act, post_slope)) return VFX_ENOTSUP;
    if (resblk4_takes(dilation)) return resblk4_launch(x, y, w, B, C, L, dilation, slope, post_act, post_slope, stream);
    ConvArgs a;
    resblk4_fill_args(a, x, y, w, B, C, L, dilation, slope, post_act, post_slope);
    // strip pitch: the one with fewer quad columns per block, nseg P (more outputs per column)
    auto nseg_of = [&](int P) { return (dilation + P - 5) / (P - 4); };
    const int pshift = 32 * nseg_of(32) < 64 * nseg_of(64) ? 5 : 6;
    const int nseg = nseg_of(1 << pshift);
    a.rs_pshift = pshift;
    a.rs_nseg = nseg;
    const long long nblk = ((long long)L + 4ll * dilation - 1) / (4ll * dilation);
    const long long nsegs = nblk * nseg;
    const int G = 64 >> pshift;
    const long long ntiles = (nsegs + G - 1) / G;
    if (ntiles * G >= (1 << 20)) return VFX_ENOTSUP;   // fast_div's range
    const size_t lds = (size_t)C * a.yp * sizeof(float);   // 66 560 bytes (the staging buffers, 49 152, alias it)
    const dim3 grid(convw_grid_x(a, (int)ntiles), 1, B);
    set_last_tile(C, 256, TILE_RESBLK4S);
    return vfx_launch<resblk4s_kernel>(grid, dim3(256), lds, (hipStream_t)stream, a);
}
