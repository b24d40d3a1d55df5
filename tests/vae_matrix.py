"""The fp32 kernels of the image path (csrc/vae.hip: slh_sgemm in its three forms, slh_gn32_stats / _apply, slh_softmax32,
slh_vae_conv_in, slh_vae_moments, slh_vae_sample, slh_vae_post_quant) element by element: the case matrix, float64 references with
derived per-element bounds, and plain-torch stand-ins of each kernel's arithmetic.  Importable without a GPU.

tests/test_vae_matrix_gpu.py runs every case on the device inside a fenced, NaN-prefilled arena (the LoRA matrix's arena);
tests/test_host.py proves on the CPU that the bounds admit the stand-ins and reject mutants of them, and that the matrix reaches every
form and edge.  Which sgemm kernel a case takes is asked of the library (lib.sgemm_form - slh_sgemm's own selection answers), how many
clusters a GroupNorm reduction has of lib.gn32_workspace; no dispatch rule is restated here.

Notation: eps = 2^-24 (one fp32 rounding).  An fp32 sum of t terms has t - 1 additions, a product of two fp32 values rounds once (or not
at all inside an fma): a dot product of t terms plus a bias is within (t + 1) eps S of the exact value, S the expression on absolute
values (first order in eps, as everywhere in tests/util.py).  Every bound is elementwise_bound(ref, S, n, extra, rel) = rel |ref| + n eps S
+ extra with rel = 0 for an fp32 output and 2^-8 for the bf16 one.  The references are float64 evaluations on exactly the fp32 / bf16
values the kernel is given.  No figure below is fitted to a kernel's output.

What the transcendental terms rest on: the library is built with -O3 and nothing that relaxes floating point (no -ffast-math, no
-fno-hip-fp32-correctly-rounded-divide-sqrt): `/` is the correctly rounded division (v_div_scale / v_div_fmas / v_div_fixup: one
rounding, eps), expf is the device library's (argument reduction in two pieces, v_exp_f32, ldexp: documented 1 ulp = 2 eps), fp32
denormals are kept but a library routine may flush its result: a value below the smallest normal carries an absolute 2^-126.

Every kind of case is five functions of the case: bufs (the buffers of its arena), inputs (what they hold, valid columns only), descs
(the launches), reference ({label: (buffer, ref, bound)}; bound None = bit-exact; it is handed the outputs because two checks are
defined on the kernel's own earlier output: GroupNorm's y on its fp32 statistics, noisy_bf16 on noisy_f32) and standin.
"""
import math
from typing import Dict, List

import torch

from sliders_amd import lib
from tests.attention_matrix import BF, F32, FAKE_BASE, Buf, layout
from tests.lora_matrix import Arena, _gen, _short          # noqa: F401  (Arena: re-exported for the GPU test)
from tests.util import BF16_RND, FP32_EPS, elementwise_bound

F64 = torch.float64
FLUSH = 2.0 ** -126           # smallest normal fp32
VAE_SCALING = 0.13025
GN_EPS = 1e-6


class Case:
    """kind + keyword parameters (defaults per kind in _DEFAULTS); .id names every parameter that is not at its default"""

    def __init__(self, kind, **kw):
        d = dict(_DEFAULTS[kind])
        for k in kw:
            assert k in d, (kind, k)
        d.update(kw)
        self.kind, self.kw = kind, d
        self.__dict__.update(d)
        self.id = (kind + " " + " ".join(f"{k}={_short(v)}" for k, v in d.items() if v != _DEFAULTS[kind][k])).strip()

    def __repr__(self):
        return self.id


_DEFAULTS = {
    # dense: M, N, K.  conv: (B, hs, ws) of the SOURCE image, cin, N = Cout; M and K follow.  bias: 0 none, 1 per column, 2 per row;
    # pads: (ldx, ldw, ldr, ldc) minus the row; split: the descriptor's split_bf16 REQUEST (the library decides the form)
    "sgemm": dict(M=64, N=128, K=64, conv=None, stride=1, pad=1, up=0, cin=0, alpha=1.0, bias=0, res=0, pads=(0, 0, 0, 0), split=0),
    # x = 2 randn + off; pads: (ldx - C, ldy - C)
    "gn32": dict(C=128, groups=32, hw=64, B=1, pads=(0, 0), act=0, off=0.5),
    # cls n: 3 randn; s: every element -80 but the LAST column of each row, +80
    "softmax": dict(rows=3, cols=1024, ld=1024, cls="n"),
    "conv_in": dict(cin=3, cout=128, geo=(2, 3, 5)),
    "moments": dict(C=128, geo=(2, 3, 5)),
    "sample": dict(B=1, hw=15, outs=("latent_f32", "noisy_f32", "noisy_bf16")),
    "post_quant": dict(B=1, hw=15, zbf=0),
}

MUTANTS = {
    "sgemm": ("split_drops_hi_lo", "split_skips_last_step_nk_mod3_1", "upsample_bounds_hs", "stride2_reads_pad1", "row_bias_per_column",
              "alpha_after_bias", "sample_offset_uses_ho", "bottom_tap_unmasked_stride2"),
    "gn32": ("one_pass_no_shift", "first_cluster_only"),
    "softmax": ("sum_first_1024",),
    "moments": ("lanes_stop_at_256",),
    "sample": ("no_logvar_clamp",),
    "conv_in": ("drop_fourth_channel",),
    "post_quant": ("no_inv_scaling",),
}


def conv_out_dims(hs, ws, stride, pad, up):
    """the output size slh_sgemm's conv mode requires of its caller (include/sliders_hip.h, slh_sgemm_desc); None: no output"""
    he, we = hs << up, ws << up
    if he + pad < 2 or we + pad < 2:
        return None
    return (he + pad - 2) // stride + 1, (we + pad - 2) // stride + 1


def _cases() -> List[Case]:
    cs = []
    G = lambda **kw: cs.append(Case("sgemm", **kw))
    Ms, Ns, Ks = (1, 63, 64, 65, 127, 128, 129, 300), (4, 124, 128, 132, 260), (16, 32, 48, 64, 96, 128, 160, 224)
    # --- sgemm, dense.  Every M (below / at / above the 64- and 128-row tiles, one row, three tiles), every N (one quad, just below / at /
    # above the 128-column tile, three tiles), every K: exact form K / 16 = 1 .. 14 steps; split form nk = K / 32 = 1, 2, 3, 4, 5, 7 (the
    # prologue's clamped k1, k2 at nk = 1, 2; zero, one and two tail steps after the triples) and the fallbacks K = 16, 48.  Two passes over K
    # with different M, N, epilogues and leading dimensions, each K in both requests.
    for i in range(8):
        for split in (0, 1):
            G(M=Ms[i], N=Ns[i % 5], K=Ks[i], alpha=(1.0, 0.37)[i & 1], bias=i % 3, res=(i >> 1) & 1, pads=((0, 0, 0, 0), (4, 8, 12, 4))[(i >> 2) & 1],
              split=split)
    for i in range(8):
        G(M=Ms[(i + 3) % 8], N=Ns[(i + 2) % 5], K=Ks[i], alpha=(0.37, 1.0)[i & 1], bias=(i + 1) % 3, res=1 - ((i >> 1) & 1), pads=(8, 4, 4, 12), split=1)
    for split in (0, 1):                                   # the epilogue in full: alpha, either bias, residual, every ld wider
        G(M=300, N=132, K=64, alpha=0.37, bias=2, res=1, pads=(4, 4, 4, 4), split=split)
        G(M=300, N=132, K=64, alpha=0.37, bias=1, split=split)
    G(M=129, N=260, K=128, alpha=0.37, bias=2, split=1)    # nk = 4 (one tail step) over 3 x 3 tiles of the 64-row form
    G(M=65, N=124, K=224, split=1)                         # nk = 7: two triples and one tail step
    # --- sgemm, conv.  Odd, even and one-pixel images x the four stride / pad pairs x every cin, all with the split request: cin 32, 64 run
    # the split kernel, 16, 48 fall back to the exact one.  Batch and residual do NOT follow the form: cin 16 and 32 run batch 3 (a tap that
    # escapes its mask, or a wrong sample offset, lands in the next sample's data; with one sample it reads a fence of tiny values), 48 and
    # 64 batch 1; the residual alternates with the image and the cin, so every (stride, pad) pair has it on and off in both kernels
    for hi, hw in enumerate(((7, 5), (8, 6), (1, 1))):
        for si, (stride, pad) in enumerate(((1, 1), (2, 0), (1, 0), (2, 1))):
            if conv_out_dims(hw[0], hw[1], stride, pad, 0) is None:
                continue                                   # (1, 1) without padding has no output pixel
            for ci, cin in enumerate((16, 32, 48, 64)):
                G(conv=((3, 3, 1, 1)[ci], hw[0], hw[1]), stride=stride, pad=pad, cin=cin, N=(4, 132)[(ci + si + hi) % 2], bias=(ci + si) % 2,
                  res=(hi + ci) & 1, pads=((0, 0, 0, 0), (4, 8, 4, 8))[(ci + hi) % 2], split=1)
    for k, (hw, stride, pad) in enumerate((((7, 5), 1, 1), ((8, 6), 2, 0), ((7, 5), 2, 1), ((8, 6), 1, 0))):     # the exact kernel at cin 32 / 64
        G(conv=(3, hw[0], hw[1]), stride=stride, pad=pad, cin=(32, 64)[k & 1], N=(132, 4)[k & 1], bias=1, res=k & 1, split=0)
    # the decoder's Upsample2D read: ho = 2 hs, source pixel (iy >> 1, ix >> 1), bounds hs << 1
    for k, hw in enumerate(((7, 5), (4, 3), (1, 1))):
        for split in (0, 1):
            G(conv=((3, 1, 3)[k], hw[0], hw[1]), up=1, cin=(32, 16, 64)[k], N=(4, 132, 4)[k], bias=1, res=(k + split) & 1, split=split)
    G(conv=(3, 7, 5), up=1, cin=48, N=132, split=1, pads=(4, 4, 4, 4))
    # --- sgemm, the 128-row split form, either side of its threshold (256 tiles of 128 x 128) - where the library puts it, see
    # test_vae_matrix_is_not_hollow
    G(M=32763, N=4, K=32, bias=1, split=1)                 # 256 tiles, nk = 1, a ragged last tile
    G(M=32640, N=4, K=32, bias=1, split=1)                 # 255 tiles: the 64-row form with 510 workgroups
    G(M=16381, N=132, K=96, alpha=0.37, bias=2, pads=(4, 0, 0, 4), split=1)            # 128 x 2 tiles, nk = 3, a second column tile of 4 columns
    G(conv=(2, 128, 128), cin=32, N=4, bias=1, split=1)    # 32 768 pixels = 256 tiles, nk = 9
    G(conv=(2, 64, 64), up=1, cin=32, N=4, bias=1, res=1, split=1)
    # --- gn32: every (C, groups) class - cg = 4, 8, 16, 32; rpi = 32 (C = 32) .. 1 (C = 1024); lpg from 16 down to 4 - at every hw (one
    # row, below / at / above one row block of 64 rows, 16 row blocks = one cluster, 17 = two, 18 with a ragged last block)
    for i, (C, g) in enumerate(((32, 8), (128, 32), (256, 32), (256, 64), (512, 32), (1024, 32))):
        for jj, hw in enumerate((1, 63, 64, 65, 1024, 1025, 1093)):
            B = 1 if C * hw >= 1 << 20 else (1, 3)[(i + jj) % 2]            # (three samples of the largest tensor would be 25 MB)
            cs.append(Case("gn32", C=C, groups=g, hw=hw, B=B, pads=((0, 0), (4, 8))[(i + jj) % 3 == 0], act=(jj + i // 2) % 2,
                           off=(0.5, 300.0)[(i + jj // 2) % 2]))
    # --- softmax32: one quad, exactly one pass of the 256 threads, a ragged second pass with padding columns, four passes
    for rows, cols, ld in ((1, 4, 4), (3, 1024, 1024), (3, 1028, 1040), (5, 4096, 4096)):
        for cls in "ns":
            cs.append(Case("softmax", rows=rows, cols=cols, ld=ld, cls=cls))
    # --- conv_in: both channel counts, one quad and 32 quads of outputs, one pixel / a thread total that is no multiple of 256
    for cin in (3, 4):
        for cout in (4, 128):
            for geo in ((1, 1, 1), (2, 3, 5), (3, 9, 7)):
                cs.append(Case("conv_in", cin=cin, cout=cout, geo=geo))
    # --- moments: one lane, half a pass, one full pass of the 64 lanes, a ragged second pass (C = 260: lane 0 alone), two passes; pixel
    # counts that are no multiple of the four waves of a workgroup
    for i, C in enumerate((4, 128, 256, 260, 512)):
        for jj, geo in enumerate(((1, 1, 1), (2, 3, 5), (3, 3, 3))):
            cs.append(Case("moments", C=C, geo=geo))
    # --- sample: every non-empty subset of the outputs; hw 1 .. 2500 (2 x 4 x 2500 = 20 000 bf16 elements: the rounding statistic)
    outs = ("latent_f32", "noisy_f32", "noisy_bf16")
    subsets = [tuple(o for b, o in enumerate(outs) if m >> b & 1) for m in range(1, 8)]
    for i, sub in enumerate(subsets):
        cs.append(Case("sample", B=(1, 2)[i & 1], hw=(1, 15, 300)[i % 3], outs=sub))
    cs.append(Case("sample", B=2, hw=2500))
    cs.append(Case("sample", B=2, hw=1))
    # --- post_quant: fp32 and bf16 latents
    for zbf in (0, 1):
        for i, hw in enumerate((1, 15, 300)):
            cs.append(Case("post_quant", B=(1, 3)[(i + zbf) % 2], hw=hw, zbf=zbf))
    return cs


def _rn(g, *s, off=0.0, scale=1.0, dtype=F32):
    return (torch.randn(*s, generator=g, device=g.device, dtype=F32) * scale + off).to(dtype)


def _f32(v: float) -> float:
    """v rounded to fp32, as a descriptor's float field holds it"""
    return float(torch.tensor(v, dtype=F32))


# ---------------------------------------------------------------------------------------------------------------------------
# sgemm
# ---------------------------------------------------------------------------------------------------------------------------
def _sg_geo(c):
    """(rows of x, columns of x, M, N, K, ho, wo)"""
    if c.conv:
        B, hs, ws = c.conv
        ho, wo = conv_out_dims(hs, ws, c.stride, c.pad, c.up)
        return B * hs * ws, c.cin, B * ho * wo, c.N, 9 * c.cin, ho, wo
    return c.M, c.K, c.M, c.N, c.K, 0, 0


def sgemm_bufs(c):
    rows, xc, M, N, K, _, _ = _sg_geo(c)
    b = [Buf("x", rows, xc, xc + c.pads[0], F32, "in"), Buf("w", N, K, K + c.pads[1], F32, "in")]
    if c.bias:
        n = M if c.bias == 2 else N
        b.append(Buf("bias", 1, n, n, F32, "in"))
    if c.res:
        b.append(Buf("res", M, N, N + c.pads[2], F32, "in"))
    b.append(Buf("c", M, N, N + c.pads[3], F32, "out"))
    return b


def sgemm_inputs(c, dev, seed):
    g = _gen(dev, seed)
    rows, xc, M, N, K, _, _ = _sg_geo(c)
    L = {"x": _rn(g, rows, xc), "w": _rn(g, N, K, scale=1.0 / math.sqrt(K))}
    if c.bias:
        L["bias"] = _rn(g, 1, M if c.bias == 2 else N)
    if c.res:
        L["res"] = _rn(g, M, N)
    return L


def sgemm_desc(c, base=FAKE_BASE, off=None):
    off = off if off is not None else layout(sgemm_bufs(c))[0]
    rows, xc, M, N, K, ho, wo = _sg_geo(c)
    kw = dict(x=base + off["x"], w=base + off["w"], c=base + off["c"], ldx=xc + c.pads[0], ldw=K + c.pads[1], ldr=N + c.pads[2], ldc=N + c.pads[3],
              M=M, N=N, K=K, mode=1 if c.conv else 0, alpha=c.alpha, bias_per_row=1 if c.bias == 2 else 0, split_bf16=c.split)
    if c.bias:
        kw["bias"] = base + off["bias"]
    if c.res:
        kw["residual"] = base + off["res"]
    if c.conv:
        kw.update(cin=c.cin, batch=c.conv[0], hs=c.conv[1], ws=c.conv[2], ho=ho, wo=wo, stride=c.stride, pad=c.pad, upsample=c.up)
    return lib.SgemmDesc(**kw)


def sgemm_descs(c, base=FAKE_BASE, off=None):
    return [(lib.OP_SGEMM, sgemm_desc(c, base, off))]


def sgemm_form(c) -> str:
    """'exact' | 'split<64>' | 'split<128>': the library's answer for the case's descriptor"""
    return lib.sgemm_form(sgemm_desc(c))


def _sg_window(c, x):
    """the reference's im2col: x [B*hs*ws][cin] -> [M][9*cin], K index = tap * cin + channel, written as array slicing of the (upsampled)
    image padded with `pad` zero rows / columns before and two after - no index arithmetic shared with the kernel or the stand-in"""
    if not c.conv:
        return x
    B, hs, ws = c.conv
    rows, cin, M, N, K, ho, wo = _sg_geo(c)
    img = x.reshape(B, hs, ws, cin)
    if c.up:
        img = img.repeat_interleave(2, 1).repeat_interleave(2, 2)
    P = torch.nn.functional.pad(img, (0, 0, c.pad, 2, c.pad, 2))
    s = c.stride
    taps = [P[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s, :] for ky in range(3) for kx in range(3)]
    return torch.stack(taps, 3).reshape(M, K)


def _sg_gather(c, x, mutant=None):
    """the stand-in's operand fetch, as the kernels' load_x writes it: output row -> (sample, oy, ox), tap -> (iy, ix), the bounds check
    against hs << upsample, the read of source pixel (iy >> upsample, ix >> upsample); zero outside"""
    if not c.conv:
        return x
    B, hs, ws = c.conv
    rows, cin, M, N, K, ho, wo = _sg_geo(c)
    m = torch.arange(M, device=x.device)
    b, rem = m // (ho * wo), m % (ho * wo)
    oy, ox = rem // wo, rem % wo
    sh = 1 if c.up else 0
    lim_h, lim_w = (hs, ws) if mutant == "upsample_bounds_hs" else (hs << sh, ws << sh)
    pad = 1 if (mutant == "stride2_reads_pad1" and c.stride == 2) else c.pad
    Z = torch.zeros(M, 9, cin, dtype=x.dtype, device=x.device)
    for tap in range(9):
        iy, ix = oy * c.stride + tap // 3 - pad, ox * c.stride + tap % 3 - pad
        ok = (iy >= 0) & (iy < lim_h) & (ix >= 0) & (ix < lim_w)
        if mutant == "bottom_tap_unmasked_stride2" and c.stride == 2:
            ok = (iy >= 0) & (ix >= 0) & (ix < lim_w)                 # row hs of a sample is row 0 of the next one
        hb = ho if mutant == "sample_offset_uses_ho" else hs
        src = ((b * hb + (iy >> sh)) * ws + (ix >> sh)).clamp(0, rows - 1)
        Z[:, tap] = torch.where(ok[:, None], x[src], torch.zeros((), dtype=x.dtype, device=x.device))
    return Z.reshape(M, K)


def _split(t32):
    """fp32 -> (hi, lo, r) in fp32 with t = hi + lo + r exactly: hi = bf16(t), lo = bf16(t - hi) (t - hi is exact in fp32: it has at most 16
    significant bits), r = (t - hi) - lo (exact likewise) - the kernel's split_store4"""
    hi = t32.to(BF).to(F32)
    d = t32 - hi
    lo = d.to(BF).to(F32)
    return hi, lo, d - lo


def sgemm_reference(c, L, got=None):
    """ref = alpha sum_k x w + bias + residual in float64 (conv: x the 3 x 3 window; what lies outside the image is a zero term).

    exact (sgemm_kernel): v_mfma_f32_32x32x2_f32 multiplies and adds in fp32: K products and K - 1 additions in some order, then
    `* alpha`, `+ bias`, `+ residual`: n = K + 3 over S = |alpha| sum |x||w| + |bias| + |res|.

    split (sgemm_bf16x3_kernel): every operand is t = hi + lo + r with hi = bf16(t), lo = bf16(t - hi), so |t - hi| <= 2^-9 |t| at the top
    of a binade (2^-8 |t| just above a power of two) and |r| <= 2^-8 |lo|.  The kernel adds hi.hi + hi.lo + lo.hi - each a product of two
    8-bit significands, exact in fp32 - and drops the rest:
        x w - (xh wh + xh wl + xl wh) = xl wl + xr w + (x - xr) wr,
    per product at most |xl||wl| + |xr||w| + |x - xr||wr|: about 3 * 2^-18 |x||w| for operands spread over their binades, 3 * 2^-16 |x||w|
    in the worst case.  The halves are functions of the inputs alone (round to nearest even), so the term is EVALUATED, not estimated:
    extra = |alpha| (|xl| |wl|^T + |xr| |w|^T + |x - xr| |wr|^T) - never more than the worst case, and what "16 mantissa bits per operand"
    means element by element (a kernel that also drops hi.lo is off by 2^-9 |x||w| per product).  The 3K products are summed in fp32 by the
    bf16 MFMAs: n = 3K + 3 over S = |alpha| (|xh||wh| + |xh||wl| + |xl||wh|) + |bias| + |res|."""
    rows, xc, M, N, K, _, _ = _sg_geo(c)
    Z32, W32 = _sg_window(c, L["x"]), L["w"]
    a = _f32(c.alpha)
    ref = a * (Z32.to(F64) @ W32.to(F64).T)
    form = sgemm_form(c)
    extra = None
    if form == "exact":
        S, n = abs(a) * (Z32.to(F64).abs() @ W32.to(F64).abs().T), K + 3
    else:
        (xh, xl, xr), (wh, wl, wr) = (tuple(t.to(F64).abs() for t in _split(v)) for v in (Z32, W32))
        S, n = abs(a) * (xh @ wh.T + xh @ wl.T + xl @ wh.T), 3 * K + 3
        x_minus_r = (Z32.to(F64) - _split(Z32)[2].to(F64)).abs()
        extra = abs(a) * (xl @ wl.T + xr @ W32.to(F64).abs().T + x_minus_r @ wr.T)
    if c.bias:
        bv = L["bias"][0].to(F64)
        bv = bv[:, None] if c.bias == 2 else bv[None, :]
        ref, S = ref + bv, S + bv.abs()
    if c.res:
        ref, S = ref + L["res"].to(F64), S + L["res"].to(F64).abs()
    return {"c": ("c", ref, elementwise_bound(ref, S, n, extra, rel=0.0))}


def sgemm_split_terms(c, L):
    """(extra, 3 * 2^-18 |alpha| sum |x||w|) of a split case: the evaluated dropped-product term next to the figure for operands spread
    over their binades (the host test holds the first below the second on every case)"""
    Z32, W32 = _sg_window(c, L["x"]), L["w"]
    a = abs(_f32(c.alpha))
    (xh, xl, xr), (wh, wl, wr) = (tuple(t.to(F64).abs() for t in _split(v)) for v in (Z32, W32))
    x_minus_r = (Z32.to(F64) - _split(Z32)[2].to(F64)).abs()
    extra = a * (xl @ wl.T + xr @ W32.to(F64).abs().T + x_minus_r @ wr.T)
    return extra, 3.0 * 2.0 ** -18 * a * (Z32.to(F64).abs() @ W32.to(F64).abs().T)


def sgemm_standin(c, L, mutant=None):
    """fp32 torch: the operand fetch of load_x, then an fp32 matrix product per K step (exact form: the whole K; split form: per step of
    32 the three products lo.hi, hi.lo, hi.hi of the explicit halves), then alpha, bias, residual in the kernel's order"""
    assert mutant is None or mutant in MUTANTS["sgemm"]
    rows, xc, M, N, K, _, _ = _sg_geo(c)
    Z, W = _sg_gather(c, L["x"], mutant), L["w"]
    form = sgemm_form(c)
    if form == "exact":
        acc = Z @ W.T
    else:
        (xh, xl, _), (wh, wl, _) = _split(Z), _split(W)
        nk = K // 32
        acc = torch.zeros(M, N, dtype=F32, device=Z.device)
        for k in range(nk):
            if mutant == "split_skips_last_step_nk_mod3_1" and k == nk - 1 and nk % 3 == 1:
                continue
            s = slice(32 * k, 32 * k + 32)
            acc = acc + xh[:, s] @ wl[:, s].T
            if mutant != "split_drops_hi_lo":
                acc = acc + xl[:, s] @ wh[:, s].T
            acc = acc + xh[:, s] @ wh[:, s].T
    a = torch.tensor(c.alpha, dtype=F32, device=Z.device)
    bv = None
    if c.bias:
        bv = L["bias"][0]
        if c.bias == 2 and mutant != "row_bias_per_column":
            bv = bv[:, None]
        else:
            bv = bv[None, :N]
    if mutant == "alpha_after_bias" and bv is not None:
        out = (acc + bv) * a
    else:
        out = acc * a
        if bv is not None:
            out = out + bv
    if c.res:
        out = out + L["res"]
    return {"c": out}


# ---------------------------------------------------------------------------------------------------------------------------
# gn32: statistics, then apply
# ---------------------------------------------------------------------------------------------------------------------------
GN32_ROWS_PER_BLOCK = 64      # rows a statistics workgroup sums in fp32 before the partial sums continue in double (csrc/vae.hip)


def gn32_workspace(c):
    return lib.gn32_workspace(c.hw)


def gn32_bufs(c):
    prow, ntick = gn32_workspace(c)
    return [Buf("x", c.B * c.hw, c.C, c.C + c.pads[0], F32, "in"), Buf("gamma", 1, c.C, c.C, F32, "in"), Buf("beta", 1, c.C, c.C, F32, "in"),
            Buf("stats", c.B * c.groups, 2, 2, F32, "out"), Buf("y", c.B * c.hw, c.C, c.C + c.pads[1], F32, "out"),
            Buf("partial", c.B * prow, c.groups * 2, c.groups * 2, F32, "ws"), Buf("ticket", 1, c.B * ntick, c.B * ntick, F32, "acc")]


def gn32_inputs(c, dev, seed):
    g = _gen(dev, seed)
    _, ntick = gn32_workspace(c)
    return {"x": _rn(g, c.B * c.hw, c.C, off=c.off, scale=2.0), "gamma": _rn(g, 1, c.C), "beta": _rn(g, 1, c.C),
            "ticket": torch.zeros(1, c.B * ntick, device=dev)}


def gn32_descs(c, base=FAKE_BASE, off=None):
    off = off if off is not None else layout(gn32_bufs(c))[0]
    d = lib.Gn32Desc(x=base + off["x"], gamma=base + off["gamma"], beta=base + off["beta"], stats=base + off["stats"], y=base + off["y"],
                     ldx=c.C + c.pads[0], ldy=c.C + c.pads[1], C=c.C, batch=c.B, hw=c.hw, groups=c.groups, eps=GN_EPS, act=c.act,
                     partial=base + off["partial"], ticket=base + off["ticket"])
    return [(lib.OP_GN32_STATS, d), (lib.OP_GN32_APPLY, d)]


def _gn_groups(c, x, dt):
    """x [B*hw][C] -> ([B][groups][hw*cg] in dt, the shift k [B][groups][1]: the group's first element, as the kernel takes it)"""
    cg = c.C // c.groups
    xg = x.to(dt).reshape(c.B, c.hw, c.groups, cg).permute(0, 2, 1, 3).reshape(c.B, c.groups, c.hw * cg)
    return xg, xg[:, :, :1]


def gn32_reference(c, L, got=None):
    """stats = (mean, rstd = 1 / sqrt(var + eps)) per (sample, group) in float64.

    gn32_stats_kernel sums f = x - k (k the group's first element; one rounding) and f f in fp32 inside a row block of 64 rows - 64 cg
    terms per group, 64 cg - 1 additions in an order the geometry fixes - and the block sums on in double, but for one conversion to float
    where two clusters meet.  Against the exact sums A = sum (x - k), Q = sum (x - k)^2:
        |S^ - A| <= n_s eps sum |x - k|,   n_s = 64 cg + 1   (the additions, the subtraction, the conversion)
        |Q^ - Q| <= n_q eps sum (x - k)^2, n_q = 64 cg + 4   (as before, the product's rounding, and f's relative error twice in f f)
    gn_finish in double: m = A / n, mean = float(k + m), var = Q / n - m^2, rstd = float((var + eps)^-1/2):
        |d mean| <= n_s eps sum |x - k| / n + eps |mean|
        |d var|  <= n_q eps sum (x - k)^2 / n + 2 |m| n_s eps sum |x - k| / n,   |d rstd| <= rstd^3 |d var| / 2 + eps rstd.
    The shift is what keeps sum (x - k)^2 of the order of n var when the offset is 300: without it the second line holds 9e4 n.

    y is checked against the float64 value of ((x - mean) rstd gamma + beta) (SiLU) at the kernel's OWN fp32 (mean, rstd) - a wrong
    statistic fails above, a wrong apply here.  gn32_apply_kernel: a subtraction, two products and an addition (or an fma), each one
    rounding of a value no larger than |xhat gamma| + |beta|: n = 4.  SiLU y / (1 + expf(-y)): the error of y passes through a slope of at
    most 1.1 (sup |silu'| = 1.0998), so n = 4.4; then expf is off by 2 eps of t = e^-y, 1 + t rounds once, the division once:
    t / (1 + t) 2 eps + eps + eps <= 4 eps of |silu|, which is `extra`."""
    cg, n = c.C // c.groups, c.hw * (c.C // c.groups)
    xg, k = _gn_groups(c, L["x"], F64)
    f = xg - k
    A1, Q1 = f.abs().sum(-1) / n, (f * f).sum(-1) / n
    m = f.sum(-1) / n
    mean, var = k[:, :, 0] + m, ((xg - xg.mean(-1, keepdim=True)) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + _f32(GN_EPS))
    n_s, n_q = GN32_ROWS_PER_BLOCK * cg + 1, GN32_ROWS_PER_BLOCK * cg + 4
    ref = torch.stack([mean, rstd], -1).reshape(c.B * c.groups, 2)
    b_mean = elementwise_bound(mean, A1, n_s, FP32_EPS * mean.abs(), rel=0.0)
    b_rstd = elementwise_bound(rstd, 0.5 * rstd ** 3 * Q1, n_q, 0.5 * rstd ** 3 * 2 * m.abs() * n_s * FP32_EPS * A1 + FP32_EPS * rstd, rel=0.0)
    out = {"stats": ("stats", ref, torch.stack([b_mean, b_rstd], -1).reshape(c.B * c.groups, 2))}
    if got is not None:
        st = got["stats"].to(F64).reshape(c.B, 1, c.groups, 1, 2)
        x5 = L["x"].to(F64).reshape(c.B, c.hw, c.groups, cg, 1)[..., 0]
        gm, bt = L["gamma"].to(F64).reshape(1, 1, c.groups, cg), L["beta"].to(F64).reshape(1, 1, c.groups, cg)
        xg_ = (x5 - st[..., 0]) * st[..., 1] * gm
        y, S = xg_ + bt, xg_.abs() + bt.abs()
        if c.act:
            y = y * torch.sigmoid(y)
            bound = elementwise_bound(y, S, 4.4, 4 * FP32_EPS * y.abs(), rel=0.0)
        else:
            bound = elementwise_bound(y, S, 4, rel=0.0)
        out["y"] = ("y", y.reshape(c.B * c.hw, c.C), bound.reshape(c.B * c.hw, c.C))
    return out


def gn32_standin(c, L, mutant=None):
    """fp32 torch: per row block of 64 rows the shifted sums run row by row in fp32 (a thread's order), the groups' channels and the
    blocks are added in fp32 / double as in the kernel, gn_finish in double; then the apply in fp32"""
    assert mutant is None or mutant in MUTANTS["gn32"]
    cg, R = c.C // c.groups, GN32_ROWS_PER_BLOCK
    nb = (c.hw + R - 1) // R
    x = L["x"].reshape(c.B, c.hw, c.C)
    k = x[:, :1].reshape(c.B, 1, c.groups, cg)[..., :1].expand(c.B, 1, c.groups, cg).reshape(c.B, 1, c.C)
    if mutant == "one_pass_no_shift":
        k = torch.zeros_like(k)
    f = torch.zeros(c.B, nb * R, c.C, dtype=F32, device=x.device)
    f[:, :c.hw] = x - k
    f = f.reshape(c.B, nb, R, c.C)
    valid = (torch.arange(nb * R, device=x.device) < c.hw).reshape(1, nb, R, 1)
    s, q = torch.zeros(c.B, nb, c.C, device=x.device), torch.zeros(c.B, nb, c.C, device=x.device)
    for r in range(R):
        s = s + f[:, :, r]
        q = torch.where(valid[:, :, r], q + f[:, :, r] * f[:, :, r], q)
    s, q = s.reshape(c.B, nb, c.groups, cg).sum(-1), q.reshape(c.B, nb, c.groups, cg).sum(-1)          # fp32, per block and group
    if mutant == "first_cluster_only":
        s, q = s[:, :16], q[:, :16]
    Sd, Qd = s.to(F64).sum(1), q.to(F64).sum(1)
    n = float(c.hw * cg)
    m = Sd / n
    var = (Qd / n - m * m).clamp_min(0.0)
    piv = k.reshape(c.B, c.groups, cg)[..., 0].to(F64)
    mean, rstd = (piv + m).to(F32), (1.0 / torch.sqrt(var + _f32(GN_EPS))).to(F32)
    stats = torch.stack([mean, rstd], -1).reshape(c.B * c.groups, 2)
    mc, rc = (t.reshape(c.B, 1, c.groups, 1).expand(c.B, 1, c.groups, cg).reshape(c.B, 1, c.C) for t in (mean, rstd))
    y = (x - mc) * rc * L["gamma"] + L["beta"]
    if c.act:
        y = y / (1.0 + torch.exp(-y))
    return {"stats": stats, "y": y.reshape(c.B * c.hw, c.C)}


# ---------------------------------------------------------------------------------------------------------------------------
# softmax32 (in place)
# ---------------------------------------------------------------------------------------------------------------------------
def softmax_bufs(c):
    return [Buf("x", c.rows, c.cols, c.ld, F32, "acc")]


def softmax_inputs(c, dev, seed):
    g = _gen(dev, seed)
    if c.cls == "n":
        return {"x": _rn(g, c.rows, c.cols, scale=3.0)}
    x = torch.full((c.rows, c.cols), -80.0, device=dev)
    x[:, c.cols - 1] = 80.0
    return {"x": x}


def softmax_descs(c, base=FAKE_BASE, off=None):
    off = off if off is not None else layout(softmax_bufs(c))[0]
    return [(lib.OP_SOFTMAX32, lib.Softmax32Desc(x=base + off["x"], ld=c.ld, rows=c.rows, cols=c.cols))]


def softmax_reference(c, L, got=None):
    """p_j = e^(x_j - max) / sum_i e^(x_i - max).  softmax32_kernel: max is exact; d_j = x_j - max rounds once, which the exponential
    turns into a relative |x_j - max| eps; expf adds 2 eps.  The sum of `cols` such terms: cols - 1 additions (cols eps, with the
    reciprocal's rounding), and its terms' own errors, the p-weighted mean of theirs: sum_i p_i (|x_i - max| + 2) eps = (A + 2) eps.  The
    product with the reciprocal rounds once.  Relative to p_j: (|x_j - max| + A + cols + c) eps with c = 2 + 2 + 1 = 5 (expf of the
    element, expf inside the sum, the product; the reciprocal is counted with the sum), on the flags named at the top of this file.
    The term A is not in the formula the matrix was specified with, (|x - max| + cols + c) eps: it is the rounded subtraction acting on
    the terms of the sum, derived like the rest and small beside cols (about 3 on the randn rows).
    Absolute: e^(x_j - max) below the smallest normal may come back flushed, and so may its product with a reciprocal <= 1: 2 * 2^-126."""
    x = L["x"].to(F64)
    d = x - x.max(-1, keepdim=True).values
    p = torch.softmax(x, -1)
    A = (p * d.abs()).sum(-1, keepdim=True)
    bound = elementwise_bound(p, p * (d.abs() + A + c.cols + 5), 1, 2 * FLUSH, rel=0.0)
    return {"x": ("x", p, bound)}


def softmax_standin(c, L, mutant=None):
    assert mutant is None or mutant in MUTANTS["softmax"]
    x = L["x"]
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    s = (e[:, :1024] if mutant == "sum_first_1024" else e).sum(-1, keepdim=True)
    return {"x": e * (1.0 / s)}


# ---------------------------------------------------------------------------------------------------------------------------
# conv_in (3 | 4 -> cout, 3 x 3, padding 1) and moments (conv_out C -> 8, 3 x 3, then quant_conv 8 -> 8)
# ---------------------------------------------------------------------------------------------------------------------------
def _window3(img, B, H, W):
    """[B*H*W][C] -> [B*H*W][9][C]: the 3 x 3 window of padding 1, tap-major"""
    C = img.shape[1]
    P = torch.nn.functional.pad(img.reshape(B, H, W, C), (0, 0, 1, 1, 1, 1))
    return torch.stack([P[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], 3).reshape(B * H * W, 9, C)


def conv_in_bufs(c):
    B, H, W = c.geo
    return [Buf("img", B * H * W, c.cin, c.cin, F32, "in"), Buf("w", c.cout, 9 * c.cin, 9 * c.cin, F32, "in"), Buf("bias", 1, c.cout, c.cout, F32, "in"),
            Buf("y", B * H * W, c.cout, c.cout, F32, "out")]


def conv_in_inputs(c, dev, seed):
    g = _gen(dev, seed)
    B, H, W = c.geo
    return {"img": _rn(g, B * H * W, c.cin), "w": _rn(g, c.cout, 9 * c.cin, scale=1.0 / math.sqrt(9 * c.cin)), "bias": _rn(g, 1, c.cout)}


def conv_in_descs(c, base=FAKE_BASE, off=None):
    off = off if off is not None else layout(conv_in_bufs(c))[0]
    B, H, W = c.geo
    return [(lib.OP_VAE_CONV_IN, lib.VaeConvDesc(x=base + off["img"], w=base + off["w"], bias=base + off["bias"], y=base + off["y"], batch=B, h=H, wd=W,
                                                 cin=c.cin, cout=c.cout))]


def conv_in_reference(c, L, got=None):
    """y = bias + sum over 9 taps x cin channels of x w.  vae_conv_in_kernel: one thread adds the 9 cin products (each one rounding at
    most) to the bias in fp32: 9 cin + 1 terms, 9 cin additions, n = 9 cin + 1; S = |bias| + sum |x||w|."""
    B, H, W = c.geo
    Z, Wt = _window3(L["img"].to(F64), B, H, W).reshape(B * H * W, 9 * c.cin), L["w"].to(F64)
    bias = L["bias"][0].to(F64)
    ref, S = Z @ Wt.T + bias, Z.abs() @ Wt.abs().T + bias.abs()
    return {"y": ("y", ref, elementwise_bound(ref, S, 9 * c.cin + 1, rel=0.0))}


def conv_in_standin(c, L, mutant=None):
    assert mutant is None or mutant in MUTANTS["conv_in"]
    B, H, W = c.geo
    Z, Wt = _window3(L["img"], B, H, W), L["w"].reshape(c.cout, 9, c.cin)
    if mutant == "drop_fourth_channel":
        Z, Wt = Z[:, :, :3], Wt[:, :, :3]
    acc = L["bias"][0][None, :].expand(B * H * W, c.cout).clone()
    for tap in range(9):
        acc = acc + Z[:, tap] @ Wt[:, tap].T
    return {"y": acc}


def moments_bufs(c):
    B, H, W = c.geo
    return [Buf("x", B * H * W, c.C, c.C, F32, "in"), Buf("w", 8, 9 * c.C, 9 * c.C, F32, "in"), Buf("bias", 1, 8, 8, F32, "in"),
            Buf("qw", 8, 8, 8, F32, "in"), Buf("qb", 1, 8, 8, F32, "in"), Buf("out", B * H * W, 8, 8, F32, "out")]


def moments_inputs(c, dev, seed):
    g = _gen(dev, seed)
    B, H, W = c.geo
    return {"x": _rn(g, B * H * W, c.C), "w": _rn(g, 8, 9 * c.C, scale=1.0 / math.sqrt(9 * c.C)), "bias": _rn(g, 1, 8), "qw": _rn(g, 8, 8, scale=0.35),
            "qb": _rn(g, 1, 8)}


def moments_descs(c, base=FAKE_BASE, off=None):
    off = off if off is not None else layout(moments_bufs(c))[0]
    B, H, W = c.geo
    return [(lib.OP_VAE_MOMENTS, lib.VaeConvDesc(x=base + off["x"], w=base + off["w"], bias=base + off["bias"], qw=base + off["qw"], qb=base + off["qb"],
                                                 y=base + off["out"], batch=B, h=H, wd=W, cin=c.C, cout=8))]


def moments_reference(c, L, got=None):
    """a_o = bias_o + sum over 9 taps x C channels of x w (conv_out), out_l = qb_l + sum_o qw[l][o] a_o (quant_conv).
    vae_moments_kernel: the lanes of a wave share the 9 C products, the shuffle tree adds the lanes, the bias comes last: 9 C + 1 terms,
    n1 = 9 C + 1 over S1 = |bias| + sum |x||w| - so |a^ - a| <= n1 eps S1.  Then 9 terms, n = 9, over S2 = |qb| + sum |qw| S1 (|a| <= S1),
    and the first stage's error reaches the output through |qw|: extra = sum_o |qw[l][o]| n1 eps S1_o."""
    B, H, W = c.geo
    Z, Wt = _window3(L["x"].to(F64), B, H, W).reshape(B * H * W, 9 * c.C), L["w"].to(F64)
    bias, qw, qb = L["bias"][0].to(F64), L["qw"].to(F64), L["qb"][0].to(F64)
    a, S1 = Z @ Wt.T + bias, Z.abs() @ Wt.abs().T + bias.abs()
    ref, S2 = a @ qw.T + qb, S1 @ qw.abs().T + qb.abs()
    extra = ((9 * c.C + 1) * FP32_EPS * S1) @ qw.abs().T
    return {"out": ("out", ref, elementwise_bound(ref, S2, 9, extra, rel=0.0))}


def moments_standin(c, L, mutant=None):
    """fp32 torch: lane l of 64 adds the products of channels 4 l .. 4 l + 3 (and 256 further on) tap by tap, the lanes meet in the xor
    tree, then bias and the 8 x 8 product"""
    assert mutant is None or mutant in MUTANTS["moments"]
    B, H, W = c.geo
    Z, Wt = _window3(L["x"], B, H, W), L["w"].reshape(8, 9, c.C)
    acc = torch.zeros(B * H * W, 64, 8, device=Z.device)
    for tap in range(9):
        for c0 in range(0, c.C, 256):
            if mutant == "lanes_stop_at_256" and c0 >= 256:
                continue
            nl = min(256, c.C - c0) // 4
            zz = Z[:, tap, c0:c0 + 4 * nl].reshape(-1, nl, 1, 4)
            ww = Wt[:, tap, c0:c0 + 4 * nl].reshape(8, nl, 4).permute(1, 0, 2)[None]
            acc[:, :nl] = acc[:, :nl] + (zz * ww).sum(-1)
    o = 32
    while o:
        acc = acc + acc[:, torch.arange(64, device=Z.device) ^ o]
        o //= 2
    a = acc[:, 0] + L["bias"][0]
    q = L["qb"][0][None, :].expand(B * H * W, 8).clone()
    for o in range(8):
        q = q + L["qw"][:, o][None, :] * a[:, o:o + 1]
    return {"out": q}


# ---------------------------------------------------------------------------------------------------------------------------
# sample and post_quant
# ---------------------------------------------------------------------------------------------------------------------------
SQRT_ALPHA, SQRT_1M_ALPHA = 0.8, 0.6
_LOGVAR_EDGES = (-40.0, -30.0, 20.0, 25.0)


def sample_bufs(c):
    n = c.B * 4
    b = [Buf("moments", c.B * c.hw, 8, 8, F32, "in"), Buf("post_noise", n, c.hw, c.hw, F32, "in"), Buf("noise", n, c.hw, c.hw, F32, "in")]
    return b + [Buf(o, n, c.hw, c.hw, BF if o == "noisy_bf16" else F32, "out") for o in c.outs]


def sample_inputs(c, dev, seed):
    """mean ~ N(0, 1); logvar ~ N(0, 1) with every fifth element one of -40, -30 (below / at the lower clamp), 20, 25 (at / above the
    upper one), in turn"""
    g = _gen(dev, seed)
    m = _rn(g, c.B * c.hw, 8)
    lv = m[:, 4:].clone().reshape(-1)
    idx = torch.arange(0, lv.numel(), 5, device=dev)
    lv[idx] = torch.tensor(_LOGVAR_EDGES, device=dev)[torch.arange(idx.numel(), device=dev) % 4]
    m[:, 4:] = lv.reshape(-1, 4)
    return {"moments": m, "post_noise": _rn(g, c.B * 4, c.hw), "noise": _rn(g, c.B * 4, c.hw)}


def sample_descs(c, base=FAKE_BASE, off=None):
    off = off if off is not None else layout(sample_bufs(c))[0]
    kw = {o: base + off[o] for o in c.outs}
    return [(lib.OP_VAE_SAMPLE, lib.VaeSampleDesc(moments=base + off["moments"], post_noise=base + off["post_noise"], noise=base + off["noise"], batch=c.B,
                                                  hw=c.hw, scaling=VAE_SCALING, sqrt_alpha=SQRT_ALPHA, sqrt_one_minus_alpha=SQRT_1M_ALPHA, **kw))]


def _sample_nchw(c, t):
    """[B*hw][4] -> [B*4][hw]"""
    return t.reshape(c.B, c.hw, 4).permute(0, 2, 1).reshape(c.B * 4, c.hw)


def sample_reference(c, L, got=None):
    """z = (mean + e^(clamp(logvar, -30, 20) / 2) n1) scaling; noisy = sa z + so n2.
    vae_sample_kernel: the clamp and the halving are exact; expf is off by 2 eps of std; std n1 rounds once, the sum with the mean once,
    the product with scaling once: every rounding is of a value no larger than (|mean| + |std n1|) |scaling| =: Sz, five of them: n = 5.
    noisy: z's error times |sa|, then two products and a sum (or an fma and a product): n = 8 over Sn = |sa| Sz + |so n2|.
    noisy_bf16 is the bf16 rounding of the fp32 value: rel = 2^-8, and the fp32 error passes the rounding enlarged by 1 + 2^-8 at most
    (extra); where the case also writes noisy_f32 the two must agree BIT FOR BIT (label noisy_bf16 == bf16(noisy_f32))."""
    mom = L["moments"].to(F64)
    mean, lv = _sample_nchw(c, mom[:, :4]), _sample_nchw(c, mom[:, 4:]).clamp(-30.0, 20.0)
    sc, sa, so = _f32(VAE_SCALING), _f32(SQRT_ALPHA), _f32(SQRT_1M_ALPHA)
    sn = torch.exp(0.5 * lv) * L["post_noise"].to(F64)
    z, Sz = (mean + sn) * sc, (mean.abs() + sn.abs()) * abs(sc)
    noisy, Sn = sa * z + so * L["noise"].to(F64), abs(sa) * Sz + (so * L["noise"].to(F64)).abs()
    out = {}
    if "latent_f32" in c.outs:
        out["latent_f32"] = ("latent_f32", z, elementwise_bound(z, Sz, 5, rel=0.0))
    if "noisy_f32" in c.outs:
        out["noisy_f32"] = ("noisy_f32", noisy, elementwise_bound(noisy, Sn, 8, rel=0.0))
    if "noisy_bf16" in c.outs:
        out["noisy_bf16"] = ("noisy_bf16", noisy, elementwise_bound(noisy, Sn, 8, BF16_RND * 8 * FP32_EPS * Sn, rel=BF16_RND))
        if got is not None and "noisy_f32" in c.outs:
            out["noisy_bf16 == bf16(noisy_f32)"] = ("noisy_bf16", got["noisy_f32"].to(BF), None)
    return out


def sample_standin(c, L, mutant=None):
    assert mutant is None or mutant in MUTANTS["sample"]
    mom = L["moments"]
    mean, lv = _sample_nchw(c, mom[:, :4]), _sample_nchw(c, mom[:, 4:])
    if mutant != "no_logvar_clamp":
        lv = lv.clamp(-30.0, 20.0)
    t = lambda v: torch.tensor(v, dtype=F32, device=mom.device)
    z = (mean + torch.exp(0.5 * lv) * L["post_noise"]) * t(VAE_SCALING)
    noisy = t(SQRT_ALPHA) * z + t(SQRT_1M_ALPHA) * L["noise"]
    full = {"latent_f32": z, "noisy_f32": noisy, "noisy_bf16": noisy.to(BF)}
    return {o: full[o] for o in c.outs}


def post_quant_bufs(c):
    return [Buf("z", c.B * 4, c.hw, c.hw, BF if c.zbf else F32, "in"), Buf("qw", 1, 16, 16, F32, "in"), Buf("qb", 1, 4, 4, F32, "in"),
            Buf("y", c.B * c.hw, 4, 4, F32, "out")]


def post_quant_inputs(c, dev, seed):
    g = _gen(dev, seed)
    return {"z": _rn(g, c.B * 4, c.hw, dtype=BF if c.zbf else F32), "qw": _rn(g, 1, 16, scale=0.5), "qb": _rn(g, 1, 4)}


def post_quant_descs(c, base=FAKE_BASE, off=None):
    off = off if off is not None else layout(post_quant_bufs(c))[0]
    return [(lib.OP_VAE_POST_QUANT, lib.VaeConvDesc(x=base + off["z"], qw=base + off["qw"], qb=base + off["qb"], y=base + off["y"], batch=c.B, h=c.hw, wd=1,
                                                    cin=c.zbf, inv_scaling=1.0 / VAE_SCALING))]


def post_quant_reference(c, L, got=None):
    """y[pixel][o] = qb_o + sum_c qw[o][c] (z_c inv_scaling).  vae_post_quant_kernel: z inv_scaling rounds once, each product once (or
    inside an fma), five terms and four additions: n = 6 over S = |qb| + sum |qw||z inv_scaling|.  A bf16 z converts to fp32 exactly."""
    inv = _f32(1.0 / VAE_SCALING)
    v = L["z"].to(F64).reshape(c.B, 4, c.hw).permute(0, 2, 1).reshape(c.B * c.hw, 4) * inv
    qw, qb = L["qw"].to(F64).reshape(4, 4), L["qb"][0].to(F64)
    ref, S = v @ qw.T + qb, v.abs() @ qw.abs().T + qb.abs()
    return {"y": ("y", ref, elementwise_bound(ref, S, 6, rel=0.0))}


def post_quant_standin(c, L, mutant=None):
    assert mutant is None or mutant in MUTANTS["post_quant"]
    v = L["z"].to(F32).reshape(c.B, 4, c.hw).permute(0, 2, 1).reshape(c.B * c.hw, 4)
    if mutant != "no_inv_scaling":
        v = v * torch.tensor(1.0 / VAE_SCALING, dtype=F32, device=v.device)
    qw, qb = L["qw"].reshape(4, 4), L["qb"][0]
    out = qb[None, :].expand(c.B * c.hw, 4).clone()
    for ch in range(4):
        out = out + qw[:, ch][None, :] * v[:, ch:ch + 1]
    return {"y": out}


# ---------------------------------------------------------------------------------------------------------------------------
KINDS = {k: dict(bufs=globals()[k + "_bufs"], inputs=globals()[k + "_inputs"], descs=globals()[k + "_descs"], reference=globals()[k + "_reference"],
                 standin=globals()[k + "_standin"]) for k in _DEFAULTS}

SGEMM_FORMS = ["sgemm " + f for f in lib.SGEMM_FORMS]
FORMS = SGEMM_FORMS + ["gn32_stats", "gn32_apply", "softmax32", "vae_conv_in", "vae_moments", "vae_sample", "vae_post_quant"]


def form_of(c: Case, label: str = "") -> str:
    """the kernel form an output of the case belongs to (the sgemm ones as the library names them)"""
    if c.kind == "sgemm":
        return "sgemm " + sgemm_form(c)
    if c.kind == "gn32":
        return "gn32_stats" if label == "stats" else "gn32_apply"
    return {"softmax": "softmax32", "conv_in": "vae_conv_in", "moments": "vae_moments", "sample": "vae_sample", "post_quant": "vae_post_quant"}[c.kind]


CASES = _cases()


def _find(kind, **kw):
    for c in CASES:
        if c.kind == kind and all(getattr(c, k) == v for k, v in kw.items()):
            return c
    raise KeyError((kind, kw))


def mutant_cases() -> Dict[str, Case]:
    """'kind/mutant' -> the case of the GPU list that catches it"""
    return {
        "sgemm/split_drops_hi_lo": _find("sgemm", M=300, N=132, K=64, bias=1, split=1),
        "sgemm/split_skips_last_step_nk_mod3_1": _find("sgemm", M=129, N=260, K=128, split=1),
        "sgemm/upsample_bounds_hs": _find("sgemm", conv=(3, 7, 5), up=1, cin=32, split=1),
        "sgemm/stride2_reads_pad1": _find("sgemm", conv=(3, 8, 6), stride=2, pad=0, split=0),
        "sgemm/row_bias_per_column": _find("sgemm", M=300, N=132, K=64, bias=2, split=0),
        "sgemm/alpha_after_bias": _find("sgemm", M=300, N=132, K=64, bias=1, split=0),
        "sgemm/sample_offset_uses_ho": _find("sgemm", conv=(3, 8, 6), stride=2, pad=0, cin=32, split=1),
        "sgemm/bottom_tap_unmasked_stride2": _find("sgemm", conv=(3, 8, 6), stride=2, pad=0, cin=32, split=1),
        "gn32/one_pass_no_shift": _find("gn32", C=32, groups=8, hw=1093, off=300.0),
        "gn32/first_cluster_only": _find("gn32", C=128, groups=32, hw=1093),
        "softmax/sum_first_1024": _find("softmax", cols=1028, cls="s"),
        "moments/lanes_stop_at_256": _find("moments", C=260, geo=(2, 3, 5)),
        "sample/no_logvar_clamp": _find("sample", B=2, hw=2500),
        "conv_in/drop_fourth_channel": _find("conv_in", cin=4, cout=128, geo=(3, 9, 7)),
        "post_quant/no_inv_scaling": _find("post_quant", hw=300, zbf=0),
    }
