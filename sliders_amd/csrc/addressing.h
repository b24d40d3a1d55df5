// Operand addressing shared by the bf16 GEMM kernels (gemm*.hip) and the skinny LoRA products (lora.hip): which source pixel
// feeds a filter tap of the implicit-GEMM 3x3 convolution, which concat source holds a channel, where a weight / adapter row
// starts.  The helpers are templates over the argument struct: GemmArgs and lora.hip's AddrArgs name the geometry fields alike
// (a0, a1, lda0, lda1, ca0, ca1, hs, ws, src_xform, stride).  The fp32 kernels of vae.hip take pixel_of_row from here.  gfx950 only.
#pragma once
#include "common.h"

// row m of the implicit GEMM -> (sample, output pixel); rows run [b][oy][ox]
struct RowPixel { int b, oy, ox; };
__device__ __forceinline__ RowPixel pixel_of_row(const int m, const int ho, const int wo) {
    const int hw = ho * wo;
    const int b = m / hw;
    const int rem = m - b * hw;
    const int oy = rem / wo;
    return {b, oy, rem - oy * wo};
}

// Source pixel of filter tap (ky, kx) of a 3x3, pad-1 convolution at output pixel (b, oy, ox).  src_xform 0: the source is the
// input; 1: its nearest-neighbour 2x upsampling; 2: its zero-dilated 2x grid (only even (iy, ix) hold data: the backward-data
// form of a stride-2 convolution).  !ok: the tap reads padding or a hole (the callers substitute zeros); pix indexes the source's
// [b][hs][ws] pixels.  (vae.hip shares pixel_of_row and keeps its own tap - conv_tap_src: fp32, pad 0 or 1, its own descriptor;
// lora_conv_dgrad_kernel - the transposed walk, from an input pixel to the outputs it feeds - states its own addressing.)
struct ConvTap { bool ok; long pix; };
template <class G>
__device__ __forceinline__ ConvTap conv_tap(const G& g, const int b, const int oy, const int ox, const int ky, const int kx) {
    const int sh = g.src_xform ? 1 : 0;
    const int HL = g.hs << sh, WL = g.ws << sh;
    const int iy = oy * g.stride + ky - 1;
    const int ix = ox * g.stride + kx - 1;
    bool ok = (iy >= 0) & (iy < HL) & (ix >= 0) & (ix < WL);
    if (g.src_xform == 2) ok = ok & (((iy | ix) & 1) == 0);
    const int sy = iy >> sh, sx = ix >> sh;
    return {ok, ((long)b * g.hs + sy) * g.ws + sx};
}

// channel c of the (optionally two-source, channel-concatenated) A operand -> the source that holds it, its row pitch and the
// channel inside it
struct SrcSel { const __bf16* base; int ld, cc; bool second; };
template <class G>
__device__ __forceinline__ SrcSel src_select(const G& g, const int c) {
    const bool s1 = c >= g.ca0;
    return {s1 ? g.a1 : g.a0, s1 ? g.lda1 : g.lda0, s1 ? c - g.ca0 : c, s1};
}

// First K tile of weight row n as an LDS-DMA lane fetches it (16-byte slot `slot` of the row's 128 bytes).  Packed weights
// (pack_gemm_w: [N/64][K/64] blocks of 64 rows x 64 k) are stored swizzled, so a lane reads its PHYSICAL slot; the swizzle key
// of a packed row, (n >> 1) & 7, has period 16, so a tile may start at row 0 / 16 / 32 / 48 of a block and still land swizzled
// by its tile-relative row.  A kernel whose LDS rows are not 128 bytes (gemm7: 64) passes the slot it wants, keyed by n itself.
template <class P>
__device__ __forceinline__ const __bf16* w_row_src_packed(const P& p, const int n, const int slot) {
    return p.w + ((long)(n >> 6) * (p.K >> 6)) * 4096 + ((n & 63) << 6) + (slot << 3);
}
// ... and for either layout (w_packed 0: row-major [N][ldw], swizzled here by the tile-relative row)
template <class P>
__device__ __forceinline__ const __bf16* w_row_src(const P& p, const int n, const int row, const int fslot) {
    return p.w_packed ? w_row_src_packed(p, n, fslot) : p.w + (long)n * p.ldw + ((fslot ^ ((row >> 1) & 7)) << 3);
}

// k0-th column of row `row` of the fused adapter's down matrix (lora_down [rank][K], staged as a 32-row tile): rows past the
// rank come from the zero page
template <class P>
__device__ __forceinline__ const __bf16* lora_down_src(const P& p, const int row, const int k0, const int fslot) {
    return row < p.lora_rank ? p.lora_down + (long)row * p.K + k0 + ((fslot ^ ((row >> 1) & 7)) << 3) : (const __bf16*)slh_zero_page;
}
