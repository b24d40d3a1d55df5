"""The LoRA helper kernels (csrc/lora.hip: slh_skinny, slh_gemv, slh_lora_wgrad, slh_lora_wgrad_batch, slh_lora_conv_dgrad,
slh_temb_lora_bwd, slh_lora_ln_fold; csrc/ops.hip: ew_kernel's COPY / ADD / UPSAMPLE_BWD and colsum_kernel) element by element: the
case matrix, the input classes, float64 references with derived per-element bounds, and plain-torch stand-ins of each kernel's
arithmetic.  Importable without a GPU.

tests/test_lora_matrix_gpu.py runs every case on the device inside a fenced, NaN-prefilled arena; tests/test_host.py proves on the CPU
that the bounds admit the stand-ins (fp32 accumulation in the kernel's chunk and lane order, the kernel's internal roundings) and reject
mutants of them, and that the matrix reaches every form.  Which skinny instantiation a case takes and how a weight gradient is split
is asked of the library (lib.skinny_kernel_name, lib.wgrad_geometry - the dispatch code itself answers, no rule is restated here).

Notation: eps = 2^-24 (one fp32 rounding; an n-term fp32 sum in any order is within n eps (sum of |terms|)), u = 2^-8 (bf16 round to
nearest).  A reference is the float64 evaluation of the operation on exactly the bf16 / fp32 values the kernel is given; S is the same
expression on absolute values.  Every bound is elementwise_bound(ref, S, n, extra, rel): rel |ref| + n eps S + extra with rel = u for a
bf16 output and 0 for an fp32 one.  A product of two bf16 values is exact in fp32; a product with an fp32 factor rounds once, which is
counted as one more term.  No figure below is fitted to a kernel's output.

Every kind of case is five functions of the case: bufs (the buffers of its arena), inputs (what they hold, in storage layout, valid
columns only), launches (the descriptors), reference ({buffer: (ref, bound)}; bound None = bit-exact) and standin.
"""
import math
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from sliders_amd import lib
from tests.attention_matrix import BF, F32, FAKE_BASE, Arena as _Arena, Buf, _ESIZE, layout
from tests.util import BF16_RND, FP32_EPS, elementwise_bound

F64 = torch.float64
NCHUNK_SLAB = 256            # floats per slab and rank row: 32 chunks x 8 channels


def rup(x, q):
    return (x + q - 1) // q * q


class Case:
    """kind + keyword parameters (defaults per kind in _DEFAULTS); .id names every parameter that is not at its default"""

    def __init__(self, kind, **kw):
        d = dict(_DEFAULTS[kind])
        for k in kw:
            assert k in d, (kind, k)
        d.update(kw)
        self.kind, self.kw = kind, d
        self.__dict__.update(d)
        self.id = kind + " " + " ".join(f"{k}={_short(v)}" for k, v in d.items() if v != _DEFAULTS[kind][k])

    def __repr__(self):
        return self.id


def _short(v):
    if isinstance(v, (list, tuple)) and v and isinstance(v[0], dict):
        return "[" + ";".join(",".join(f"{k}{_short(x)}" for k, x in p.items()) for p in v) + "]"
    if isinstance(v, (list, tuple)):
        return "x".join(str(x) for x in v)
    return str(v)


INPUT_CLASSES = {
    "n": "randn everywhere",
    "o": "randn + 1 on the activation side (a / x / z / u / emb / the elementwise operand): the terms of a sum no longer average out, and a "
         "bf16 output has enough elements above 0.1 for the rounding statistic where it has 10 000 of them at all",
}
# the += kernels (wgrad, temb_lora_bwd, colsum, conv_dgrad with accumulate) always start from a non-zero random output

_DEFAULTS = {
    # conv: (B, hs, ws) of the SOURCE image or None (dense, M rows); ca: (ca0, ca1); pad: (lda0 - ca0, lda1 - ca1); kmajor: three
    # launches, a0 at columns 0 / K / 2K of one [M][3K] buffer, out columns 0 / 4 / 8 of ldo = 12
    "skinny": dict(M=5, R=4, ca=(64, 0), pad=(0, 0), conv=None, stride=1, xform=0, bias=0, ldo_pad=0, out_kind=0, kmajor=0, cls="n"),
    "gemv": dict(nb=2, N=37, K=320, in_act=1, out_f32=0, bias=1, addend=1, lora=1, tcol=1, pad=0, cls="n"),
    # probs: the problems (one, or the batch); each dict(M | conv, stride, xform, c=(c0, c1), R (the case's), rmajor, vg, pad)
    # form: "atomic" | "slab" (single launches), "batch" | "batch_slab"
    "wgrad": dict(R=4, form="atomic", probs=(), cls="n"),
    "cdgrad": dict(B=1, hl=7, wl=5, stride=1, cin=8, acc=1, ldu=4, ucol=0, pad=0, cls="n"),
    "temb": dict(C=320, ted=1280, cls="n"),
    "lnfold": dict(rows=(4,), K=320, cls="n"),
    # op: copy | add | add_inplace | upsample | colsum.  M rows (copy / add), (B, h, w) (upsample: the OUTPUT image), (B, hw) (colsum)
    "ew": dict(op="copy", M=37, C=8, geo=None, pads=(8, 16, 24), cls="n"),
}

MUTANTS = {
    "skinny": ("drop_last_partial_step", "row_ge_R_into_row0", "no_bias"),
    "wgrad": ("ignore_vgroup", "taps_as_stride1", "no_scale", "assign_not_add"),
    "cdgrad": ("no_oy_check", "no_parity_check"),
    "gemv": ("ignore_tcol", "mask_last_sample"),
    "ew": ("colsum_first_512_rows",),
}


def _wp(M=None, conv=None, stride=1, xform=0, c=(64, 0), rmajor=0, vg=0, pad=(0, 0)):
    return dict(M=M, conv=conv, stride=stride, xform=xform, c=c, rmajor=rmajor, vg=vg, pad=pad)


def _cases() -> List[Case]:
    cs = []
    S = lambda **kw: cs.append(Case("skinny", **kw))
    # --- skinny, dense: every R (RMAX 4 / 12 / 16 with and without masked rows), every K edge (8: a lane's first chunk lies past K for 63
    # of 64 lanes; 512 / 520: a second, ragged step), every M (1: three masked rows of the workgroup; 333: 84 workgroups)
    for i, R in enumerate((1, 3, 4, 5, 8, 12, 13, 16)):
        K = (8, 64, 320, 512, 520)[i % 5]
        S(M=(1, 5, 333)[i % 3], R=R, ca=(K, 0), bias=i & 1, ldo_pad=(0, 3)[(i >> 1) & 1], cls="no"[i & 1])
    for i, K in enumerate((8, 64, 320, 512, 520)):
        S(M=(333, 1, 5)[i % 3], R=(12, 4, 16, 3, 5)[i], ca=(K, 0), bias=(i + 1) & 1, ldo_pad=5)
    S(M=333, R=4, ca=(8, 16), pad=(8, 24), bias=1)                                    # two sources, both wider than the source
    S(M=5, R=13, ca=(8, 16), pad=(16, 8), ldo_pad=3, cls="o")
    # --- k-major (the fused q|k|v down-gradient: a0 offset into a 3K-wide buffer, ldo = 12 written at columns 0 / 4 / 8)
    S(M=333, R=4, ca=(64, 0), kmajor=1)
    S(M=5, R=4, ca=(320, 0), kmajor=1, cls="o")
    # --- conv: odd and even images, both strides, every src_xform, one / two sources, every R class, both output forms
    k = 0
    for hw in ((7, 5), (8, 6)):
        for stride in (1, 2):
            for xform in (0, 1, 2):
                ca = ((8, 0), (8, 16), (72, 0))[k % 3]
                ok = (k // 2) & 1
                S(conv=(2, hw[0], hw[1]), stride=stride, xform=xform, ca=ca, pad=(8, 8 if ca[1] else 0), R=(3, 4, 12)[(k + k // 3) % 3],
                  out_kind=ok, bias=ok or (k & 1), ldo_pad=0 if ok else 4, cls="no"[k & 1])
                k += 1
    # --- the 16-lanes-per-row form: either side of the switch, a ragged M, K below one step (64 < 8 * 16) and a ragged last step (136)
    S(M=16384, R=4, ca=(64, 0))
    S(M=16385, R=4, ca=(64, 0), bias=1)
    S(M=16391, R=5, ca=(136, 0), cls="o")                                           # masked rows in the 16-lane form
    S(M=16385, R=13, ca=(136, 0), bias=1, ldo_pad=3)
    S(M=16391, R=4, ca=(64, 0), kmajor=1)
    S(conv=(5, 60, 56), ca=(8, 0), R=4, out_kind=1, bias=1, cls="o")                  # conv_out form, 16 800 pixels
    S(conv=(3, 40, 36), xform=1, ca=(8, 0), R=3, ldo_pad=1)                           # the upsampler's adapter: 17 280 output pixels

    G = lambda **kw: cs.append(Case("gemv", **kw))
    # covering set: every (option, value) pair occurs, with every nb, N and K
    G(nb=1, N=1, K=8, in_act=0, out_f32=1, bias=0, addend=0, lora=0, tcol=0)
    G(nb=2, N=5, K=320, in_act=1, out_f32=0, bias=1, addend=1, lora=1, tcol=1, pad=8)
    G(nb=7, N=37, K=512, in_act=0, out_f32=0, bias=1, addend=0, lora=1, tcol=0, pad=16)
    G(nb=8, N=37, K=520, in_act=1, out_f32=1, bias=0, addend=1, lora=1, tcol=1, cls="o")
    G(nb=8, N=5, K=1280, in_act=1, out_f32=0, bias=1, addend=1, lora=0, tcol=0, pad=8)
    G(nb=7, N=1, K=1280, in_act=0, out_f32=1, bias=0, addend=1, lora=1, tcol=1)
    G(nb=1, N=37, K=8, in_act=1, out_f32=0, bias=0, addend=0, lora=1, tcol=1, pad=24, cls="o")
    G(nb=2, N=1, K=512, in_act=1, out_f32=1, bias=1, addend=0, lora=0, tcol=0)

    W = lambda **kw: cs.append(Case("wgrad", **kw))
    forms = ("atomic", "slab", "batch", "batch_slab")
    # general: R x form x layout, C in {8, 64, 264 (a second column block with one valid chunk), 320}, M either side of every edge
    Ms, Cs = (1, 7, 64, 65, 512, 513, 1024, 1025), (8, 64, 264, 320)
    i = 0
    for R in (4, 12):
        for form in forms:
            for j in range(4):
                M, C = Ms[(2 * i + j) % 8], Cs[(i + j) % 4]
                if j == 3:                                       # two sources, the first wider than its row
                    p = _wp(M=M, c=(C - 8 if C > 8 else 8, 8), rmajor=(i + j) & 1, pad=(8, 16))
                else:
                    p = _wp(M=M, c=(C, 0), rmajor=(i + j) & 1, pad=(8 * (j & 1), 0))
                W(R=R, form=form, probs=(p,), cls="no"[(i + j) & 1])
            i += 1
    for form in forms:                                          # M = 512 / 513 / 1024 / 1025 in every form
        for M in (512, 513, 1024, 1025):
            W(R=4, form=form, probs=(_wp(M=M, c=(264, 0), rmajor=M & 1),))
    # the fused q|k|v up-gradients exactly as the planner builds them: C = 192 in groups of 64, V [M][12], out [192][4]
    for form in forms:
        W(R=4, form=form, probs=(_wp(M=333 if form != "slab" else 1025, c=(192, 0), vg=64),), cls="o")
    # conv mode
    k = 0
    for hw in ((7, 5), (8, 6)):
        for stride in (1, 2):
            for xform in (0, 1, 2):
                W(R=(4, 12)[k & 1], form=forms[k % 4], cls="no"[(k >> 1) & 1],
                  probs=(_wp(conv=(2, hw[0], hw[1]), stride=stride, xform=xform, c=((8, 0), (72, 0), (8, 64))[k % 3], rmajor=(k + 1) & 1, pad=(8, 0)),))
                k += 1
    W(R=4, form="slab", probs=(_wp(conv=(3, 7, 5), stride=2, c=(72, 0), rmajor=1),))
    W(R=12, form="slab", probs=(_wp(conv=(3, 8, 6), stride=1, xform=1, c=(8, 0), rmajor=1),))
    # one batch mixes dense, conv, vgroup_cols and two-source problems (each batch built with ONE slab / no-slab choice)
    mix = (_wp(M=513, c=(320, 0)), _wp(conv=(2, 7, 5), stride=2, c=(72, 0), rmajor=1), _wp(M=65, c=(192, 0), vg=64),
           _wp(M=1025, c=(56, 8), rmajor=1, pad=(8, 8)), _wp(M=1, c=(8, 0)), _wp(conv=(1, 8, 6), xform=2, c=(8, 0), rmajor=1))
    W(R=4, form="batch", probs=mix)
    W(R=4, form="batch_slab", probs=mix, cls="o")
    mix12 = (_wp(M=513, c=(264, 0), rmajor=1), _wp(conv=(2, 7, 5), stride=2, c=(8, 0), rmajor=1), _wp(M=7, c=(8, 64), pad=(0, 8)))
    W(R=12, form="batch", probs=mix12)
    W(R=12, form="batch_slab", probs=mix12)

    D = lambda **kw: cs.append(Case("cdgrad", **kw))
    k = 0
    for stride in (1, 2):
        for hl, wl in ((7, 5), (8, 6), (1, 1)):
            for cin in (8, 64, 72):
                wide = k % 3 == 0                                # ldu = 12 with U at a column offset, as inside a fused q|k|v T buffer
                D(B=(1, 3)[k & 1], hl=hl, wl=wl, stride=stride, cin=cin, acc=(k >> 1) & 1, ldu=12 if wide else 4,
                  ucol=(4, 8)[(k // 3) & 1] if wide else 0, pad=(0, 8)[(k // 3) & 1], cls="no"[k & 1])
                k += 1
    D(B=3, hl=7, wl=5, stride=2, cin=72, acc=0, ldu=12, ucol=8, pad=16)
    D(B=1, hl=8, wl=6, stride=2, cin=8, acc=0, pad=8)
    D(B=3, hl=40, wl=36, stride=2, cin=8, acc=1, cls="o")        # 4 320 threads (16.9 workgroups), 34 560 outputs: the rounding statistic applies

    for C, ted in ((320, 1280), (100, 104), (8, 8)):
        cs.append(Case("temb", C=C, ted=ted, cls="no"[C == 100]))
    L = lambda **kw: cs.append(Case("lnfold", **kw))
    L(rows=(1,), K=8)
    L(rows=(12,), K=320)
    L(rows=(4, 16, 1), K=2048)
    L(rows=(16, 12, 4), K=2056, cls="o")
    L(rows=(1, 4, 12), K=320)

    E = lambda **kw: cs.append(Case("ew", **kw))
    for op in ("copy", "add", "add_inplace"):
        E(op=op, M=37, C=8)                                        # 37 threads
        E(op=op, M=333, C=72, cls="o")                             # 2 997 threads: 11.7 workgroups
    E(op="add", M=4099, C=72, cls="o")                            # 295 128 elements: the rounding statistic applies
    E(op="upsample", geo=(2, 3, 5), C=8)
    E(op="upsample", geo=(2, 6, 10), C=72, cls="o")
    for i, hw in enumerate((1, 7, 512, 513, 1030)):
        E(op="colsum", geo=((1, 3)[i & 1], hw), C=(8, 264)[i & 1], cls="no"[i & 1])
        E(op="colsum", geo=((3, 1)[i & 1], hw), C=(264, 8)[i & 1])
    seen, out = set(), []
    for c in cs:                                                  # the generators above may name one case twice
        if c.id not in seen:
            seen.add(c.id)
            out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# shared arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def conv_out_dims(hs, ws, xform, stride):
    HL, WL = (hs << 1, ws << 1) if xform else (hs, ws)
    return (HL - 1) // stride + 1, (WL - 1) // stride + 1


def logical_image(x, B, hs, ws, xform):
    """[B hs ws][C] -> the image the 3x3 window walks, [B][HL][WL][C]: xform 0 as stored; 1 every pixel doubled in both directions
    (nearest upsampling in front of the convolution); 2 zeros inserted between the pixels (the adjoint of a stride-2 subsampling)"""
    img = x.reshape(B, hs, ws, -1)
    if xform == 1:
        img = img.repeat_interleave(2, 1).repeat_interleave(2, 2)
    elif xform == 2:
        z = img.new_zeros(B, 2 * hs, 2 * ws, img.shape[-1])
        z[:, ::2, ::2] = img
        img = z
    return img


def im2col(x, B, hs, ws, xform, stride):
    """-> [B ho wo][9][C], padding 1: column (tap, c) of output pixel o is image pixel o * stride + tap - 1, zero outside the image"""
    img = logical_image(x, B, hs, ws, xform)
    ho, wo = conv_out_dims(hs, ws, xform, stride)
    pad = F.pad(img, (0, 0, 1, 1, 1, 1))
    taps = [pad[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride] for ky in range(3) for kx in range(3)]
    return torch.stack(taps, 3).reshape(B * ho * wo, 9, -1)


def silu_rel_err(x):
    """Relative error of common.h's silu_f(x) = x / (1.0f + __expf(-x)) against the exact silu, per element (x float64):
      __expf(-x) is v_exp_f32(fl(-x log2 e)): the constant and the product round once each, an absolute error of 2 eps |x| log2 e in the
      exponent, that is 2 eps |x| relative in the result; v_exp_f32 itself is accurate to 1 ulp (2 eps).  e = exp(-x) (1 + d), |d| <= 2 eps (|x| + 1).
      1 + e rounds once (eps); the error of e reaches the sum scaled by e / (1 + e) < 1.  The division is correctly rounded or, in the
      fast form, within 2.5 ulp: 4 eps counted.
        |silu_f(x) - silu(x)| <= (2 |x| + 2 + 1 + 4) eps |silu(x)| = (2 |x| + 7) eps |silu(x)|.
    (bf16 inputs of the cases stay below |x| = 8: no overflow or flush of the exponential.)"""
    return (2.0 * x.abs() + 7.0) * FP32_EPS


def silu_bf16_terms(x):
    """x: the bf16 inputs as float64 -> (t, amb): the value the kernel's round_bf16(silu_f(x)) is compared with, and what the rounding
    may add per unit of the factor it is multiplied with.  Where lo = silu (1 - d) and hi = silu (1 + d), d = silu_rel_err, round to the
    same bf16 value the kernel's rounding is determined: t is that value, amb = 0.  Where they do not - the float64 silu lies within the
    error of silu_f of a rounding boundary, the kernel may round either way - t is the unrounded silu and amb = u |silu| (either
    neighbour is within half a bf16 ulp of it)."""
    s = x * torch.sigmoid(x)
    d = silu_rel_err(x)
    lo, hi = (s * (1 - d)).to(BF), (s * (1 + d)).to(BF)
    same = lo == hi
    t = torch.where(same, lo.double(), s)
    amb = torch.where(same, torch.zeros_like(s), BF16_RND * s.abs())
    return t, amb


def _silu_f32(x):
    """silu_f in fp32 torch arithmetic, then round_bf16"""
    x = x.float()
    return (x / (1.0 + torch.exp(-x))).to(BF).float()


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _rn(g, *s, off=0.0, dtype=BF):
    return (torch.randn(*s, generator=g, device=g.device, dtype=F32) + off).to(dtype)


def _esz(dt):
    return _ESIZE[dt]


class Arena(_Arena):
    """attention_matrix.Arena with two more roles: "acc" - a += target or an in-place operand: writable, filled with the case's own
    starting values; "ws" - a workspace: writable, NaN-prefilled (slabs)"""

    def __init__(self, bufs, dev):
        super().__init__(bufs, dev)
        for b in bufs:
            if b.role in ("acc", "ws"):
                self._bytes(b, self.writable, b.wrows)[:, :b.cols * _ESIZE[b.dtype]] = True
            if b.role == "ws":
                self.nan_fill(b.name)

    def restore(self):
        """back to the state of freeze(): NaN prefill, starting values of the += targets, zeroed tickets"""
        self.mem.copy_(self.snap)


# ---------------------------------------------------------------------------------------------------------------------------
# skinny
# ---------------------------------------------------------------------------------------------------------------------------
def _sk_geo(c):
    cin = c.ca[0] + c.ca[1]
    if c.conv:
        B, hs, ws = c.conv
        ho, wo = conv_out_dims(hs, ws, c.xform, c.stride)
        return cin, 9 * cin, B * hs * ws, B * ho * wo, ho, wo
    return cin, cin, c.M, c.M, 0, 0


def skinny_bufs(c):
    cin, K, rows, M, ho, wo = _sk_geo(c)
    G = 3 if c.kmajor else 1
    b = [Buf("a0", rows, G * c.ca[0], G * c.ca[0] + c.pad[0], BF, "in")]
    if c.ca[1]:
        b.append(Buf("a1", rows, c.ca[1], c.ca[1] + c.pad[1], BF, "in"))
    b.append(Buf("w", G * (K if c.kmajor else c.R), 4 if c.kmajor else K, 4 if c.kmajor else K, BF, "in"))
    if c.bias:
        b.append(Buf("bias", 1, 16, 16, BF, "in"))
    if c.out_kind == 0:
        b.append(Buf("out", M, G * c.R, G * c.R + c.ldo_pad, F32, "out"))
    else:
        b.append(Buf("out", c.conv[0] * c.R, ho * wo, ho * wo, BF, "out"))
    return b


def skinny_inputs(c, dev, seed):
    g = _gen(dev, seed)
    cin, K, rows, M, _, _ = _sk_geo(c)
    G = 3 if c.kmajor else 1
    off = 1.0 if "o" in c.cls else 0.0
    L = {"a0": _rn(g, rows, G * c.ca[0], off=off)}
    if c.ca[1]:
        L["a1"] = _rn(g, rows, c.ca[1], off=off)
    L["w"] = _rn(g, G * K, 4) if c.kmajor else _rn(g, c.R, K)
    if c.bias:
        L["bias"] = _rn(g, 1, 16)
    return L


def skinny_descs(c, base=FAKE_BASE, off=None):
    off = off if off is not None else layout(skinny_bufs(c))[0]
    cin, K, rows, M, ho, wo = _sk_geo(c)
    out = []
    for gi in range(3 if c.kmajor else 1):
        kw = dict(a0=base + off["a0"] + 2 * gi * c.ca[0], w=base + off["w"] + 2 * gi * K * 4, out=base + off["out"] + 4 * 4 * gi,
                  lda0=(3 if c.kmajor else 1) * c.ca[0] + c.pad[0], ca0=c.ca[0], M=M, R=c.R, K=K, out_kind=c.out_kind, w_kmajor=c.kmajor,
                  ldo=(3 if c.kmajor else 1) * c.R + c.ldo_pad if c.out_kind == 0 else 0, mode=1 if c.conv else 0, stride=c.stride)
        if c.ca[1]:
            kw.update(a1=base + off["a1"], lda1=c.ca[1] + c.pad[1], ca1=c.ca[1])
        if c.bias:
            kw["bias"] = base + off["bias"]
        if c.conv:
            kw.update(batch=c.conv[0], hs=c.conv[1], ws=c.conv[2], src_xform=c.xform, ho=ho, wo=wo)
        out.append((lib.OP_SKINNY, lib.SkinnyDesc(**kw)))
    return out


def skinny_form(c) -> str:
    return lib.skinny_kernel_name(skinny_descs(c)[0][1])


def _sk_operands(c, L, dt):
    """-> (Z [G][M][K], W [G][R][K], bias [R] or None) in dtype dt: Z the (im2col of the) concatenated sources"""
    cin, K, rows, M, _, _ = _sk_geo(c)
    if c.kmajor:
        Z = L["a0"].to(dt).reshape(M, 3, K).permute(1, 0, 2)
        W = L["w"].to(dt).reshape(3, K, 4).permute(0, 2, 1)
    else:
        a = torch.cat([L["a0"]] + ([L["a1"]] if c.ca[1] else []), 1).to(dt)
        Z = (im2col(a, c.conv[0], c.conv[1], c.conv[2], c.xform, c.stride).reshape(M, K) if c.conv else a)[None]
        W = L["w"].to(dt)[None]
    return Z, W, (L["bias"][0, :c.R].to(dt) if c.bias else None)


def _sk_store(c, t):
    """[G][M][R] -> the layout of the out buffer"""
    if c.out_kind == 1:
        B = c.conv[0]
        return t[0].reshape(B, -1, c.R).permute(0, 2, 1).reshape(B * c.R, -1)
    return t.permute(1, 0, 2).reshape(t.shape[1], -1)


def skinny_reference(c, L):
    """out[m][r] = sum_k Z[m][k] W[r][k] + bias[r], Z the rows of A (conv: the 3x3 window of padding 1 over the transformed image; the
    kernel skips the taps outside the image, which are zero terms here).  skinny_kernel: each of LPR lanes adds its chunks' products
    (exact in fp32) into fp32, the lanes meet in a shuffle tree, bias is added: a K-term fp32 sum plus one add, n = K + 1,
    S = sum |Z| |W| + |bias|; rel = u for the bf16 NCHW form."""
    Z, W, bias = _sk_operands(c, L, F64)
    ref, S = Z @ W.transpose(1, 2), Z.abs() @ W.abs().transpose(1, 2)
    if bias is not None:
        ref, S = ref + bias, S + bias.abs()
    ref, S = _sk_store(c, ref), _sk_store(c, S)
    return {"out": (ref, elementwise_bound(ref, S, Z.shape[-1] + 1, rel=BF16_RND if c.out_kind else 0.0))}


def skinny_standin(c, L, mutant=None, lpr=None, rmax=None):
    """skinny_kernel<RMAX, LPR> in fp32 torch: lane `sub` of a row walks the chunks sub, sub + LPR, .. of K (conv: of every tap's cin),
    eight fmas per chunk and row of W, then the xor-shuffle tree over the LPR lanes, then bias."""
    assert mutant is None or mutant in MUTANTS["skinny"]
    if lpr is None:
        name = skinny_form(c)
        rmax, lpr = (int(x) for x in name[len("skinny<"):-1].split(","))
    Z, W, bias = _sk_operands(c, L, F32)
    G, M, K = Z.shape
    cin = c.ca[0] + c.ca[1]
    seg = cin if c.conv else K                                     # the lanes restart at every tap
    acc = torch.zeros(G, M, lpr, c.R)
    for s0 in range(0, K, seg):
        nch = seg // 8
        steps = (nch + lpr - 1) // lpr
        for j in range(steps):
            lo, hi = j * lpr, min(nch, (j + 1) * lpr)
            if mutant == "drop_last_partial_step" and hi - lo < lpr:
                continue
            for e in range(8):
                cols = s0 + torch.arange(lo, hi) * 8 + e
                acc[:, :, :hi - lo] += Z[:, :, cols, None] * W[:, :, cols].permute(0, 2, 1)[:, None]
                if mutant == "row_ge_R_into_row0":
                    acc[:, :, :hi - lo, 0] += (rmax - c.R) * (Z[:, :, cols] * W[:, 0, cols][:, None])
    o = lpr // 2
    while o:
        acc = acc + acc[:, :, torch.arange(lpr) ^ o]
        o //= 2
    out = acc[:, :, 0]
    if bias is not None and mutant != "no_bias":
        out = out + bias
    return {"out": _sk_store(c, out).to(BF if c.out_kind else F32)}


# ---------------------------------------------------------------------------------------------------------------------------
# gemv
# ---------------------------------------------------------------------------------------------------------------------------
def gemv_bufs(c):
    T = 12                                                          # ld_t: three groups of four T columns
    b = [Buf("x", c.nb, c.K, c.K + c.pad, BF, "in"), Buf("w", c.N, c.K, c.K, BF, "in")]
    if c.bias:
        b.append(Buf("bias", 1, c.N + 7, c.N + 7, BF, "in"))
    if c.addend:
        b.append(Buf("addend", c.nb, c.N, rup(c.N, 8) + 2 * c.pad, BF, "in"))
    if c.lora:
        b += [Buf("t", c.nb, T, T, F32, "in"), Buf("up", c.N, 4, 4, BF, "in"), Buf("ls", 1, 1, 1, F32, "in")]
        if c.tcol:
            b.append(Buf("tcol", 1, c.N, c.N, F32, "in"))        # int32 values in a 4-byte buffer
    b.append(Buf("y", c.nb, c.N, c.N + (3 if c.pad else 0), F32 if c.out_f32 else BF, "out"))
    return b


def gemv_inputs(c, dev, seed):
    g = _gen(dev, seed)
    off = 1.0 if "o" in c.cls else 0.0
    L = {"x": _rn(g, c.nb, c.K, off=off), "w": _rn(g, c.N, c.K)}
    if c.bias:
        L["bias"] = _rn(g, 1, c.N + 7)
    if c.addend:
        L["addend"] = _rn(g, c.nb, c.N)
    if c.lora:
        L.update(t=_rn(g, c.nb, 12, dtype=F32), up=_rn(g, c.N, 4), ls=torch.full((1, 1), 0.75, device=dev))
        if c.tcol:
            L["tcol"] = (4 * ((torch.arange(c.N, device=dev) + 1) % 3)).to(torch.int32).view(F32).reshape(1, c.N)
    return L


def gemv_descs(c, base=FAKE_BASE, off=None):
    bufs = {b.name: b for b in gemv_bufs(c)}
    off = off if off is not None else layout(gemv_bufs(c))[0]
    at = lambda n: base + off[n]
    kw = dict(x=at("x"), w=at("w"), y=at("y"), nb=c.nb, N=c.N, K=c.K, ldx=bufs["x"].ld, ldy=bufs["y"].ld, in_act=c.in_act, out_f32=c.out_f32)
    if c.bias:
        kw["bias"] = at("bias")
    if c.addend:
        kw.update(addend=at("addend"), ld_add=bufs["addend"].ld)
    if c.lora:
        kw.update(lora_t=at("t"), lora_up=at("up"), lora_scale=at("ls"), ld_t=12)
        if c.tcol:
            kw["lora_tcol"] = at("tcol")
    return [(lib.OP_GEMV, lib.GemvDesc(**kw))]


def _gemv_tcol(c, L, mutant=None):
    if c.lora and c.tcol and mutant != "ignore_tcol":
        return L["tcol"].view(torch.int32)[0].long()
    return torch.zeros(c.N, dtype=torch.long, device=L["x"].device)


def gemv_reference(c, L):
    """v[b][n] = sum_k x'[b][k] W[n][k] + bias[n] + ls sum_r t[b][tcol[n] + r] up[n][r];  y = v, or with an addend bf16(v) + addend.
    gemv_kernel: lane l adds the products of chunks l, l + 64, .. in fp32, wave_sum joins the lanes, lane 0 adds bias and the adapter
    term (four products with an fp32 factor, three adds, the product with ls, one add: 10 counted) - n = K + 10,
    S_v = sum |x'| |W| + |bias| + |ls| sum |t| |up|, e_v = n eps S_v.
    in_act: x' = round_bf16(silu_f(x)).  silu_bf16_terms gives the value to compare with and, where the float64 silu lies within the
    error of silu_f of a rounding boundary, u |silu| per unit of |W| for that term only: extra_x = sum_k amb[b][k] |W[n][k]|.
    addend: the kernel rounds v to bf16 before it adds: against the unrounded v that is u |v| + (1 + u) (e_v + extra_x); the add rounds
    once, eps (|v| + |addend|).  The output adds rel |ref| (u for bf16, 0 for fp32)."""
    x, w = L["x"].double(), L["w"].double()
    if c.in_act:
        x, amb = silu_bf16_terms(x)
        extra = amb @ w.abs().t()
    else:
        extra = torch.zeros(c.nb, c.N, dtype=F64, device=x.device)
    v, S = x @ w.t(), x.abs() @ w.abs().t()
    if c.bias:
        bias = L["bias"][0, :c.N].double()
        v, S = v + bias, S + bias.abs()
    if c.lora:
        idx = _gemv_tcol(c, L)[:, None] + torch.arange(4, device=x.device)
        t, up, ls = L["t"].double()[:, idx], L["up"].double(), float(L["ls"])
        v, S = v + ls * (t * up).sum(-1), S + abs(ls) * (t.abs() * up.abs()).sum(-1)
    n = c.K + 10
    rel = 0.0 if c.out_f32 else BF16_RND
    if c.addend:
        ad = L["addend"].double()
        ref = v + ad
        inner = BF16_RND * v.abs() + (1 + BF16_RND) * (n * FP32_EPS * S + extra)
        return {"y": (ref, rel * ref.abs() + inner + FP32_EPS * (v.abs() + ad.abs()))}
    return {"y": (v, elementwise_bound(v, S, n, extra, rel))}


def gemv_standin(c, L, mutant=None):
    assert mutant is None or mutant in MUTANTS["gemv"]
    x, w = L["x"].float(), L["w"].float()
    if c.in_act:
        x = _silu_f32(x)
    nb = c.nb - 1 if mutant == "mask_last_sample" else c.nb
    acc = torch.zeros(c.nb, c.N, 64)
    nch = c.K // 8
    for j in range((nch + 63) // 64):
        lo, hi = j * 64, min(nch, (j + 1) * 64)
        for e in range(8):
            cols = torch.arange(lo, hi) * 8 + e
            acc[:nb, :, :hi - lo] += x[:nb, None, cols] * w[None, :, cols]
    o = 32
    while o:
        acc = acc + acc[:, :, torch.arange(64) ^ o]
        o //= 2
    v = acc[:, :, 0]
    if c.bias:
        v = v + L["bias"][0, :c.N].float()
    if c.lora:
        idx = _gemv_tcol(c, L, mutant)[:, None] + torch.arange(4)
        t, up = L["t"][:, idx], L["up"].float()
        v = v + L["ls"][0, 0] * (((t[..., 0] * up[:, 0] + t[..., 1] * up[:, 1]) + t[..., 2] * up[:, 2]) + t[..., 3] * up[:, 3])
    if c.addend:
        v = v.to(BF).float() + L["addend"].float()
    return {"y": v.to(F32 if c.out_f32 else BF)}


# ---------------------------------------------------------------------------------------------------------------------------
# wgrad
# ---------------------------------------------------------------------------------------------------------------------------
def _wg_geo(p):
    C = p["c"][0] + p["c"][1]
    if p["conv"]:
        B, hs, ws = p["conv"]
        ho, wo = conv_out_dims(hs, ws, p["xform"], p["stride"])
        return C, 9 * C, B * hs * ws, B * ho * wo, ho, wo
    return C, C, p["M"], p["M"], 0, 0


def _wg_ldv(c, p):
    return 12 if (p["vg"] or c.R == 12) else 8


WGRAD_SCALE = 0.5


def wgrad_kind(c) -> int:
    return {"atomic": 0, "slab": 1, "batch": 0, "batch_slab": 2}[c.form]


def wgrad_bufs(c, blocks: Optional[List[int]] = None):
    """blocks: workgroups per problem (the library's answer), needed for the slab forms only"""
    b = [Buf("scale", 1, 1, 1, F32, "in")]
    for i, p in enumerate(c.probs):
        C, cols, rows, M, _, _ = _wg_geo(p)
        b.append(Buf(f"z0_{i}", rows, p["c"][0], p["c"][0] + p["pad"][0], BF, "in"))
        if p["c"][1]:
            b.append(Buf(f"z1_{i}", rows, p["c"][1], p["c"][1] + p["pad"][1], BF, "in"))
        b.append(Buf(f"v_{i}", M, _wg_ldv(c, p), _wg_ldv(c, p), F32, "in"))
        b.append(Buf(f"out_{i}", c.R, cols, cols + 8, F32, "acc") if p["rmajor"] else Buf(f"out_{i}", cols, c.R, c.R + 4, F32, "acc"))
    if c.form in ("slab", "batch_slab"):
        nb = wgrad_blocks(c) if blocks is None else blocks
        tot = sum(nb) if c.form == "batch_slab" else nb[0]
        b += [Buf("slabs", tot, NCHUNK_SLAB * c.R, NCHUNK_SLAB * c.R, F32, "ws"), Buf("tickets", 1, tot, tot, F32, "acc")]
    return b


def wgrad_inputs(c, dev, seed):
    g = _gen(dev, seed)
    off = 1.0 if "o" in c.cls else 0.0
    L = {"scale": torch.full((1, 1), WGRAD_SCALE, device=dev)}
    for i, p in enumerate(c.probs):
        C, cols, rows, M, _, _ = _wg_geo(p)
        L[f"z0_{i}"] = _rn(g, rows, p["c"][0], off=off)
        if p["c"][1]:
            L[f"z1_{i}"] = _rn(g, rows, p["c"][1], off=off)
        L[f"v_{i}"] = _rn(g, M, _wg_ldv(c, p), dtype=F32)
        L[f"out_{i}"] = _rn(g, c.R, cols, dtype=F32) if p["rmajor"] else _rn(g, cols, c.R, dtype=F32)
    if c.form in ("slab", "batch_slab"):
        tot = sum(wgrad_blocks(c)) if c.form == "batch_slab" else wgrad_blocks(c)[0]
        L["tickets"] = torch.zeros(1, tot, device=dev)
    return L


def wgrad_descs(c, base=FAKE_BASE, off=None, slab_marker=None):
    """one slh_wgrad_desc per problem.  slab_marker: what .slabs / .tickets hold in a batch's descriptors (any non-null value selects
    the slab geometry; the workspace is the batch's)"""
    bufs = {b.name: b for b in wgrad_bufs(c, blocks=[1] * len(c.probs))}
    if off is None:
        off = layout(list(bufs.values()))[0]
    out = []
    for i, p in enumerate(c.probs):
        C, cols, rows, M, ho, wo = _wg_geo(p)
        kw = dict(z0=base + off[f"z0_{i}"], v=base + off[f"v_{i}"], out=base + off[f"out_{i}"], scale=base + off["scale"], ldz0=bufs[f"z0_{i}"].ld,
                  c0=p["c"][0], mode=1 if p["conv"] else 0, stride=p["stride"], M=M, R=c.R, ldv=_wg_ldv(c, p), ldo=bufs[f"out_{i}"].ld,
                  out_rmajor=p["rmajor"], vgroup_cols=p["vg"])
        if p["c"][1]:
            kw.update(z1=base + off[f"z1_{i}"], ldz1=bufs[f"z1_{i}"].ld, c1=p["c"][1])
        if p["conv"]:
            kw.update(batch=p["conv"][0], hs=p["conv"][1], ws=p["conv"][2], src_xform=p["xform"], ho=ho, wo=wo)
        if c.form == "slab":
            kw.update(slabs=base + off.get("slabs", 0x1000), tickets=base + off.get("tickets", 0x1000))
        elif c.form == "batch_slab":
            kw.update(slabs=slab_marker or 8, tickets=slab_marker or 8)
        out.append(lib.WgradDesc(**kw))
    return out


def wgrad_geometry(c):
    """(gx, splits, taps, rows_per_block) of every problem, from the library"""
    return [lib.wgrad_geometry(d, wgrad_kind(c)) for d in wgrad_descs(c)]


def wgrad_blocks(c):
    return [g[0] * g[1] * g[2] for g in wgrad_geometry(c)]


def wgrad_form(c) -> str:
    return f"wgrad{'_batch' if c.form.startswith('batch') else ''}_kernel<{c.R}> kind {wgrad_kind(c)}"


def _wg_operands(c, p, L, i, dt, mutant=None):
    """-> (Z [M][cols], V [M][cols][R]) : V per output column (vgroup_cols selects the group's four columns)"""
    C, cols, rows, M, _, _ = _wg_geo(p)
    z = torch.cat([L[f"z0_{i}"]] + ([L[f"z1_{i}"]] if p["c"][1] else []), 1).to(dt)
    if p["conv"]:
        B, hs, ws = p["conv"]
        Z = im2col(z, B, hs, ws, p["xform"], p["stride"])
        if mutant == "taps_as_stride1" and p["stride"] == 2:
            # validity from o + tap - 1 (stride 1), the address from o * 2 + tap - 1: a tap outside the image reads the clamped pixel
            img = logical_image(z, B, hs, ws, p["xform"])
            HL, WL = img.shape[1:3]
            ho, wo = conv_out_dims(hs, ws, p["xform"], 2)
            oy, ox = torch.arange(ho)[:, None], torch.arange(wo)[None]
            taps = []
            for ky in range(3):
                for kx in range(3):
                    ok = ((oy + ky - 1 >= 0) & (oy + ky - 1 < HL) & (ox + kx - 1 >= 0) & (ox + kx - 1 < WL)).to(dt)
                    iy, ix = (2 * oy + ky - 1).clamp(0, HL - 1).expand(ho, wo), (2 * ox + kx - 1).clamp(0, WL - 1).expand(ho, wo)
                    taps.append(img[:, iy, ix] * ok[None, :, :, None])
            Z = torch.stack(taps, 3).reshape(M, 9, C)
        Z = Z.reshape(M, cols)
    else:
        Z = z
    v = L[f"v_{i}"].to(dt)
    ch = torch.arange(cols, device=z.device) % C
    voff = 4 * (ch // p["vg"]) if (p["vg"] and mutant != "ignore_vgroup") else torch.zeros_like(ch)
    V = v[:, voff[:, None] + torch.arange(c.R, device=z.device)]
    return Z, V


def wgrad_reference(c, L):
    """out[col][r] (or [r][col]) = out0 + s sum_m Z[m][col] V[m][voff(col) + r], col = tap C + c in conv mode (Z the 3x3 window as for
    skinny), voff = 4 (c / vgroup_cols).  wgrad_body: a thread adds its rows' products (bf16 x fp32: one rounding each) in fp32, row
    lanes, waves and M splits are joined in fp32 (slabs in split order, or atomics in arrival order - any order is covered), the total
    is multiplied by s and added to out: M products + the sum + two more roundings, n = M + 3,
    S = |s| sum |Z| |V| + |out0|.  fp32 output: rel = 0."""
    res = {}
    for i, p in enumerate(c.probs):
        Z, V = _wg_operands(c, p, L, i, F64)
        o0 = L[f"out_{i}"].double()
        acc, S = torch.einsum("mc,mcr->cr", Z, V) * WGRAD_SCALE, torch.einsum("mc,mcr->cr", Z.abs(), V.abs()) * WGRAD_SCALE
        if p["rmajor"]:
            acc, S = acc.t(), S.t()
        ref = o0 + acc
        res[f"out_{i}"] = (ref, elementwise_bound(ref, S + o0.abs(), Z.shape[0] + 3, rel=0.0))
    return res


def wgrad_standin(c, L, mutant=None):
    """wgrad_body in fp32 torch with the library's geometry: split `by` owns rows_per_block rows, row lane ry of 8 walks rows ry, ry + 8, ..
    of them, lanes 2w and 2w + 1 fold (one wave), the four waves are added in order, the splits in split order, then out += s * total."""
    assert mutant is None or mutant in MUTANTS["wgrad"]
    res = {}
    for i, (p, (gx, splits, taps, rpb)) in enumerate(zip(c.probs, wgrad_geometry(c))):
        Z, V = _wg_operands(c, p, L, i, F32, mutant)
        M, cols = Z.shape
        Zp, Vp = torch.zeros(splits * rpb, cols), torch.zeros(splits * rpb, cols, c.R)
        Zp[:M], Vp[:M] = Z, V
        Zp, Vp = Zp.view(splits, rpb // 8, 8, cols), Vp.view(splits, rpb // 8, 8, cols, c.R)
        acc = torch.zeros(splits, 8, cols, c.R)
        for j in range(rpb // 8):
            acc += Zp[:, j, :, :, None] * Vp[:, j]
        w = acc[:, 0::2] + acc[:, 1::2]
        t = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        s = 1.0 if mutant == "no_scale" else WGRAD_SCALE
        o = torch.zeros_like(L[f"out_{i}"]) if mutant == "assign_not_add" else L[f"out_{i}"].clone()
        if wgrad_kind(c) == 0:
            for k in range(splits):
                o = o + (s * t[k]).t() if p["rmajor"] else o + s * t[k]
        else:
            tot = torch.zeros(cols, c.R)
            for k in range(splits):
                tot = tot + t[k]
            o = o + (s * tot).t() if p["rmajor"] else o + s * tot
        res[f"out_{i}"] = o
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# conv_dgrad
# ---------------------------------------------------------------------------------------------------------------------------
CDGRAD_SCALE = 0.75


def _cd_geo(c):
    ho, wo = conv_out_dims(c.hl, c.wl, 0, c.stride)
    return ho, wo


def cdgrad_bufs(c):
    ho, wo = _cd_geo(c)
    return [Buf("u", c.B * ho * wo, c.ldu, c.ldu, F32, "in"), Buf("a_down", 4, 9 * c.cin, 9 * c.cin, BF, "in"), Buf("scale", 1, 1, 1, F32, "in"),
            Buf("gx", c.B * c.hl * c.wl, c.cin, c.cin + c.pad, BF, "acc" if c.acc else "out")]


def cdgrad_inputs(c, dev, seed):
    g = _gen(dev, seed)
    ho, wo = _cd_geo(c)
    L = {"u": _rn(g, c.B * ho * wo, c.ldu, off=1.0 if "o" in c.cls else 0.0, dtype=F32), "a_down": _rn(g, 4, 9 * c.cin),
         "scale": torch.full((1, 1), CDGRAD_SCALE, device=dev)}
    if c.acc:
        L["gx"] = _rn(g, c.B * c.hl * c.wl, c.cin)
    return L


def cdgrad_descs(c, base=FAKE_BASE, off=None):
    off = off if off is not None else layout(cdgrad_bufs(c))[0]
    ho, wo = _cd_geo(c)
    return [(lib.OP_LORA_CONV_DGRAD, lib.LoraCdgradDesc(u=base + off["u"] + 4 * c.ucol, a_down=base + off["a_down"], scale=base + off["scale"],
                                                        gx=base + off["gx"], batch=c.B, hl=c.hl, wl=c.wl, ho=ho, wo=wo, stride=c.stride, cin=c.cin,
                                                        ldu=c.ldu, ldgx=c.cin + c.pad, accumulate=c.acc))]


def cdgrad_form(c) -> str:
    return f"lora_conv_dgrad stride {c.stride}"


def cdgrad_reference(c, L):
    """The adjoint of the down convolution T[o][r] = sum_{tap, ch} x[o stride + tap - 1][ch] A[r][tap][ch] (padding 1), written as the
    forward scatter: every output pixel o adds U[o] . A[:, tap, :] to input pixel o stride + tap - 1 where that lies in the image;
    gx = bf16(s sum + gx0) (accumulate) or bf16(s sum).  lora_conv_dgrad_kernel gathers instead: up to 9 taps x 4 ranks of products with
    an fp32 factor (one rounding each) added in fp32, the product with s, the add of gx0: n = 36 + 3, S = |s| sum |U| |A| + |gx0|,
    rel = u."""
    ho, wo = _cd_geo(c)
    u = L["u"].double()[:, c.ucol:c.ucol + 4]
    A = L["a_down"].double().reshape(4, 9, c.cin)

    def scatter(u_, A_):
        G = torch.zeros(c.B, c.hl + 2, c.wl + 2, c.cin, dtype=F64, device=u.device)
        for tap in range(9):
            ky, kx = tap // 3, tap % 3
            G[:, ky:ky + c.stride * (ho - 1) + 1:c.stride, kx:kx + c.stride * (wo - 1) + 1:c.stride] += (u_ @ A_[:, tap]).reshape(c.B, ho, wo, c.cin)
        return CDGRAD_SCALE * G[:, 1:-1, 1:-1].reshape(-1, c.cin)

    ref, S = scatter(u, A), scatter(u.abs(), A.abs())
    if c.acc:
        g0 = L["gx"].double()
        ref, S = ref + g0, S + g0.abs()
    return {"gx": (ref, elementwise_bound(ref, S, 39))}


def cdgrad_standin(c, L, mutant=None):
    """lora_conv_dgrad_kernel in fp32 torch, as the kernel gathers: for every tap, the output pixel (i + 1 - tap) / stride if it
    exists.  The mutants read U at the flat index the kernel would form (past the sample: the next sample's rows, or 1.0 past the end)."""
    assert mutant is None or mutant in MUTANTS["cdgrad"]
    ho, wo = _cd_geo(c)
    u = L["u"].float()[:, c.ucol:c.ucol + 4]
    u = torch.cat([u, torch.ones(2 * wo + 2, 4)])
    A = L["a_down"].float().reshape(4, 9, c.cin)
    b = torch.arange(c.B).view(-1, 1, 1)
    iy, ix = torch.arange(c.hl).view(1, -1, 1), torch.arange(c.wl).view(1, 1, -1)
    acc = torch.zeros(c.B, c.hl, c.wl, c.cin)
    for tap in range(9):
        ky, kx = tap // 3, tap % 3
        ty, tx = iy + 1 - ky, ix + 1 - kx
        ok = (ty >= 0) & (tx >= 0)
        if c.stride == 2 and mutant != "no_parity_check":
            ok = ok & (((ty | tx) & 1) == 0)
        oy, ox = ty.clamp_min(0) // c.stride, tx.clamp_min(0) // c.stride
        ok = ok & (ox < wo)
        if mutant != "no_oy_check":
            ok = ok & (oy < ho)
        idx = ((b * ho * wo + oy * wo + ox) * ok).expand(c.B, c.hl, c.wl)
        uu = u[idx] * ok.expand(c.B, c.hl, c.wl)[..., None]
        for r in range(4):
            acc += uu[..., r, None] * A[r, tap]
    v = CDGRAD_SCALE * acc.reshape(-1, c.cin)
    if c.acc:
        v = v + L["gx"].float()
    return {"gx": v.to(BF)}


# ---------------------------------------------------------------------------------------------------------------------------
# temb_lora_bwd
# ---------------------------------------------------------------------------------------------------------------------------
TEMB_SCALE = 0.5


def temb_bufs(c):
    return [Buf("g", 1, c.C, c.C, F32, "in"), Buf("t", 1, 4, 4, F32, "in"), Buf("up", c.C, 4, 4, BF, "in"), Buf("emb", 1, c.ted, c.ted, BF, "in"),
            Buf("scale", 1, 1, 1, F32, "in"), Buf("d_up", c.C, 4, 4, F32, "acc"), Buf("d_down", 4, c.ted, c.ted, F32, "acc")]


def temb_inputs(c, dev, seed):
    g = _gen(dev, seed)
    return {"g": _rn(g, 1, c.C, dtype=F32), "t": _rn(g, 1, 4, dtype=F32), "up": _rn(g, c.C, 4), "emb": _rn(g, 1, c.ted, off=1.0 if "o" in c.cls else 0.0),
            "scale": torch.full((1, 1), TEMB_SCALE, device=dev), "d_up": _rn(g, c.C, 4, dtype=F32), "d_down": _rn(g, 4, c.ted, dtype=F32)}


def temb_descs(c, base=FAKE_BASE, off=None):
    off = off if off is not None else layout(temb_bufs(c))[0]
    at = lambda n: base + off[n]
    return [(lib.OP_TEMB_LORA_BWD, lib.TembLoraBwdDesc(g=at("g"), t=at("t"), up=at("up"), emb=at("emb"), d_up=at("d_up"), d_down=at("d_down"),
                                                       scale=at("scale"), C=c.C, ted=c.ted))]


def temb_reference(c, L):
    """d_up[ch][r] = d_up0 + s g[ch] t[r]: two products and one add in fp32, n = 3, S = |s g t| + |d_up0|.
    d_down[r][k] = d_down0 + s U[r] x'[k], U[r] = sum_ch g[ch] up[ch][r] (C products with an fp32 factor, joined over lanes and waves:
    C + 1 terms), x' = round_bf16(silu_f(emb[k])); two more products and the add: n = C + 4, S = |s| (sum |g| |up|) |x'| + |d_down0|.
    Where the silu rounding is ambiguous (silu_bf16_terms) the term is compared with the unrounded silu: extra = u |silu| |s| sum |g| |up|."""
    s = TEMB_SCALE
    g, t, up = L["g"].double()[0], L["t"].double()[0], L["up"].double()
    d0u, d0d = L["d_up"].double(), L["d_down"].double()
    ru = d0u + s * g[:, None] * t[None]
    bu = elementwise_bound(ru, (s * g[:, None] * t[None]).abs() + d0u.abs(), 3, rel=0.0)
    U, Ua = g @ up, g.abs() @ up.abs()
    x, amb = silu_bf16_terms(L["emb"].double()[0])
    rd = d0d + s * U[:, None] * x[None]
    bd = elementwise_bound(rd, s * Ua[:, None] * x.abs()[None] + d0d.abs(), c.C + 4, s * Ua[:, None] * amb[None], rel=0.0)
    return {"d_up": (ru, bu), "d_down": (rd, bd)}


def temb_standin(c, L, mutant=None):
    s = TEMB_SCALE
    g, t, up = L["g"][0], L["t"][0], L["up"].float()
    d_up = L["d_up"] + (s * g)[:, None] * t[None]
    Cp = rup(c.C, 256)
    gp, upp = torch.zeros(Cp), torch.zeros(Cp, 4)
    gp[:c.C], upp[:c.C] = g, up
    part = torch.zeros(256, 4)
    for j in range(Cp // 256):
        part += gp[j * 256:(j + 1) * 256, None] * upp[j * 256:(j + 1) * 256]
    part = part.view(4, 64, 4)
    o = 32
    while o:
        part = part + part[:, torch.arange(64) ^ o]
        o //= 2
    U = ((part[0, 0] + part[1, 0]) + part[2, 0]) + part[3, 0]
    x = _silu_f32(L["emb"][0])
    return {"d_up": d_up, "d_down": L["d_down"] + (s * U)[:, None] * x[None]}


# ---------------------------------------------------------------------------------------------------------------------------
# ln_fold
# ---------------------------------------------------------------------------------------------------------------------------
def lnfold_bufs(c):
    b = [Buf("gamma", 1, c.K, c.K, BF, "in"), Buf("beta", 1, c.K, c.K, BF, "in")]
    for i, r in enumerate(c.rows):
        b += [Buf(f"a_{i}", r, c.K, c.K, BF, "in"), Buf(f"a_out_{i}", r, c.K, c.K, BF, "out"), Buf(f"s_{i}", 1, r, 16, F32, "out"),
              Buf(f"c_{i}", 1, r, 16, F32, "out")]
    return b


def lnfold_inputs(c, dev, seed):
    g = _gen(dev, seed)
    off = 1.0 if "o" in c.cls else 0.0
    L = {"gamma": _rn(g, 1, c.K, off=1.0), "beta": _rn(g, 1, c.K)}
    for i, r in enumerate(c.rows):
        L[f"a_{i}"] = _rn(g, r, c.K, off=off)
    return L


def lnfold_items(c, base=FAKE_BASE, off=None):
    off = off if off is not None else layout(lnfold_bufs(c))[0]
    at = lambda n: base + off[n]
    return [lib.lnfold_item(at(f"a_{i}"), at("gamma"), at("beta"), at(f"a_out_{i}"), at(f"s_{i}"), at(f"c_{i}"), r, c.K) for i, r in enumerate(c.rows)]


def lnfold_reference(c, L):
    """a_out = bf16(a gamma): the fp32 product of two bf16 values is exact, so a_out is the round-to-nearest of the exact product -
    bit-exact (bound None).  s_out[r] = sum_k a_out[r][k] over those exact bf16 values: the rounded product inside s_out is therefore
    reproduced, not bounded (extra = 0); a K-term fp32 sum, n = K, S = sum |a_out|.  c_out[r] = sum_k a[r][k] beta[k]: exact products,
    n = K, S = sum |a| |beta|."""
    ga, be = L["gamma"].double()[0], L["beta"].double()[0]
    res = {}
    for i, r in enumerate(c.rows):
        a = L[f"a_{i}"].double()
        ao = (a * ga).to(BF)
        res[f"a_out_{i}"] = (ao, None)
        s = ao.double().sum(-1)[None]
        res[f"s_{i}"] = (s, elementwise_bound(s, ao.double().abs().sum(-1)[None], c.K, rel=0.0))
        cc = (a * be).sum(-1)[None]
        res[f"c_{i}"] = (cc, elementwise_bound(cc, (a.abs() * be.abs()).sum(-1)[None], c.K, rel=0.0))
    return res


def lnfold_standin(c, L, mutant=None):
    ga, be = L["gamma"].float()[0], L["beta"].float()[0]
    res = {}
    Kp = rup(c.K, 2048)
    for i, r in enumerate(c.rows):
        a = L[f"a_{i}"].float()
        ao = (a * ga).to(BF)
        x, y = torch.zeros(r, Kp), torch.zeros(r, Kp)
        x[:, :c.K], y[:, :c.K] = ao.float(), a * be
        out = []
        for v in (x, y):
            v = v.view(r, Kp // 2048, 256, 8)
            acc = torch.zeros(r, 256)
            for j in range(Kp // 2048):
                for e in range(8):
                    acc = acc + v[:, j, :, e]
            acc = acc.view(r, 4, 64)
            o = 32
            while o:
                acc = acc + acc[:, :, torch.arange(64) ^ o]
                o //= 2
            out.append(((acc[:, 0, 0] + acc[:, 1, 0]) + (acc[:, 2, 0] + acc[:, 3, 0]))[None])
        res.update({f"a_out_{i}": ao, f"s_{i}": out[0], f"c_{i}": out[1]})
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# elementwise: COPY, ADD, UPSAMPLE_BWD, COLSUM
# ---------------------------------------------------------------------------------------------------------------------------
def _ew_rows(c):
    """(rows of a, rows of out)"""
    if c.op == "upsample":
        B, h, w = c.geo
        return 4 * B * h * w, B * h * w
    if c.op == "colsum":
        return c.geo[0] * c.geo[1], c.geo[0]
    return c.M, c.M


def ew_bufs(c):
    ra, ro = _ew_rows(c)
    pa, pb, po = c.pads
    if c.op == "colsum":
        return [Buf("a", ra, c.C, c.C + pa, BF, "in"), Buf("out", ro, c.C, c.C + 4, F32, "acc")]
    if c.op == "add_inplace":
        return [Buf("a", ra, c.C, c.C + pa, BF, "acc"), Buf("b", ra, c.C, c.C + pb, BF, "in")]
    b = [Buf("a", ra, c.C, c.C + pa, BF, "in")]
    if c.op == "add":
        b.append(Buf("b", ra, c.C, c.C + pb, BF, "in"))
    return b + [Buf("out", ro, c.C, c.C + po, BF, "out")]


def ew_inputs(c, dev, seed):
    g = _gen(dev, seed)
    ra, ro = _ew_rows(c)
    L = {"a": _rn(g, ra, c.C, off=1.0 if "o" in c.cls else 0.0)}
    if c.op in ("add", "add_inplace"):
        L["b"] = _rn(g, ra, c.C)
    if c.op == "colsum":
        L["out"] = _rn(g, ro, c.C, dtype=F32)
    return L


def ew_descs(c, base=FAKE_BASE, off=None):
    bufs = {b.name: b for b in ew_bufs(c)}
    off = off if off is not None else layout(ew_bufs(c))[0]
    ra, ro = _ew_rows(c)
    out = "a" if c.op == "add_inplace" else "out"
    kw = dict(a=base + off["a"], out=base + off[out], M=ra if c.op == "colsum" else ro, C=c.C, lda=bufs["a"].ld, ldo=bufs[out].ld,
              op={"copy": lib.EW_COPY, "add": lib.EW_ADD, "add_inplace": lib.EW_ADD, "upsample": lib.EW_UPSAMPLE_BWD, "colsum": lib.EW_COLSUM}[c.op])
    if "b" in bufs:
        kw.update(b=base + off["b"], ldb=bufs["b"].ld)
    if c.op == "upsample":
        kw.update(iarg=c.geo[2], iarg2=c.geo[1] * c.geo[2])
    if c.op == "colsum":
        kw["iarg2"] = c.geo[1]
    return [(lib.OP_ELEMENTWISE, lib.EwDesc(**kw))]


def ew_form(c) -> str:
    return {"copy": "ew COPY", "add": "ew ADD", "add_inplace": "ew ADD", "upsample": "ew UPSAMPLE_BWD", "colsum": "colsum"}[c.op]


def ew_reference(c, L):
    """COPY: bit-exact.  ADD: bf16(fl32(a + b)) - one fp32 add in front of the output rounding: n = 1, S = |a| + |b|, rel = u.
    UPSAMPLE_BWD: the sum of a 2 x 2 block in fp32, n = 4, rel = u.  COLSUM: out0 + the column sum of the sample's hw rows; row lanes,
    the eight of a workgroup and the workgroups of 512 rows (atomics, any order) are joined in fp32, and out0 is one more term:
    n = hw + 1, S = sum |a| + |out0|, rel = 0."""
    a = L["a"].double()
    if c.op == "copy":
        return {"out": (L["a"], None)}
    if c.op in ("add", "add_inplace"):
        b = L["b"].double()
        return {("a" if c.op == "add_inplace" else "out"): (a + b, elementwise_bound(a + b, a.abs() + b.abs(), 1))}
    if c.op == "upsample":
        B, h, w = c.geo
        blk = lambda t: t.reshape(B, h, 2, w, 2, c.C).sum((2, 4)).reshape(B * h * w, c.C)
        return {"out": (blk(a), elementwise_bound(blk(a), blk(a.abs()), 4))}
    B, hw = c.geo
    o0 = L["out"].double()
    ref = o0 + a.reshape(B, hw, c.C).sum(1)
    return {"out": (ref, elementwise_bound(ref, a.abs().reshape(B, hw, c.C).sum(1) + o0.abs(), hw + 1, rel=0.0))}


def ew_standin(c, L, mutant=None):
    assert mutant is None or mutant in MUTANTS["ew"]
    a = L["a"].float()
    if c.op == "copy":
        return {"out": L["a"].clone()}
    if c.op in ("add", "add_inplace"):
        return {("a" if c.op == "add_inplace" else "out"): (a + L["b"].float()).to(BF)}
    if c.op == "upsample":
        B, h, w = c.geo
        v = a.reshape(B, h, 2, w, 2, c.C)
        return {"out": (((v[:, :, 0, :, 0] + v[:, :, 0, :, 1]) + v[:, :, 1, :, 0]) + v[:, :, 1, :, 1]).reshape(B * h * w, c.C).to(BF)}
    B, hw = c.geo
    nblk = (hw + 511) // 512
    ap = torch.zeros(B, nblk * 512, c.C)
    ap[:, :hw] = a.reshape(B, hw, c.C)
    ap = ap.view(B, nblk, 64, 8, c.C)
    o = L["out"].clone()
    for k in range(1 if mutant == "colsum_first_512_rows" else nblk):
        acc = torch.zeros(B, 8, c.C)
        for j in range(64):
            acc = acc + ap[:, k, j]
        t = torch.zeros(B, c.C)
        for y in range(8):
            t = t + acc[:, y]
        o = o + t
    return {"out": o}


# ---------------------------------------------------------------------------------------------------------------------------
# the table of kinds
# ---------------------------------------------------------------------------------------------------------------------------
KINDS = {
    "skinny": dict(bufs=skinny_bufs, inputs=skinny_inputs, reference=skinny_reference, standin=skinny_standin, form=skinny_form),
    "gemv": dict(bufs=gemv_bufs, inputs=gemv_inputs, reference=gemv_reference, standin=gemv_standin, form=lambda c: "gemv"),
    "wgrad": dict(bufs=wgrad_bufs, inputs=wgrad_inputs, reference=wgrad_reference, standin=wgrad_standin, form=wgrad_form),
    "cdgrad": dict(bufs=cdgrad_bufs, inputs=cdgrad_inputs, reference=cdgrad_reference, standin=cdgrad_standin, form=cdgrad_form),
    "temb": dict(bufs=temb_bufs, inputs=temb_inputs, reference=temb_reference, standin=temb_standin, form=lambda c: "temb_lora_bwd"),
    "lnfold": dict(bufs=lnfold_bufs, inputs=lnfold_inputs, reference=lnfold_reference, standin=lnfold_standin, form=lambda c: "lora_ln_fold"),
    "ew": dict(bufs=ew_bufs, inputs=ew_inputs, reference=ew_reference, standin=ew_standin, form=ew_form),
}

CASES: List[Case] = _cases()

SKINNY_FORMS = [f"skinny<{r},{l}>" for r in (4, 12, 16) for l in (64, 16)]
WGRAD_FORMS = [f"wgrad_kernel<{R}> kind {k}" for R in (4, 12) for k in (0, 1)] + [f"wgrad_batch_kernel<{R}> kind {k}" for R in (4, 12) for k in (0, 2)]
FORMS = SKINNY_FORMS + WGRAD_FORMS + ["gemv", "lora_conv_dgrad stride 1", "lora_conv_dgrad stride 2", "temb_lora_bwd", "lora_ln_fold", "ew COPY",
                                      "ew ADD", "ew UPSAMPLE_BWD", "colsum"]


def form_of(c: Case) -> str:
    return KINDS[c.kind]["form"](c)


def has_atomics(c: Case) -> bool:
    """the case's result depends on the order in which fp32 atomics commit: more than one M split without slabs, or a column sum over
    more than one 512-row workgroup.  The weight-gradient splits are the library's answer; the 512 rows per colsum workgroup are
    restated from colsum_kernel (no query exists for it): if that constant grew, a case above it would merely be compared within its
    bound instead of bit for bit - the weaker of the two checks, never a false alarm."""
    if c.kind == "wgrad":
        return wgrad_kind(c) == 0 and any(g[1] > 1 for g in wgrad_geometry(c))
    return c.kind == "ew" and c.op == "colsum" and c.geo[1] > 512


# where each mutant of the CPU proof is caught on the device: the id of a listed case whose stand-in, so mutated, leaves its bound
def _find(kind, **kw):
    for c in CASES:
        if c.kind == kind and all(getattr(c, k) == v for k, v in kw.items()):
            return c
    raise KeyError((kind, kw))


def mutant_cases() -> Dict[str, Case]:
    wg = lambda f: next(c for c in CASES if c.kind == "wgrad" and f(c))
    return {
        "skinny/drop_last_partial_step": _find("skinny", ca=(520, 0), R=5),
        "skinny/row_ge_R_into_row0": _find("skinny", R=13, ca=(64, 0)),
        "skinny/no_bias": _find("skinny", M=333, R=4, ca=(8, 16)),
        "wgrad/ignore_vgroup": wg(lambda c: c.probs[0]["vg"] and c.form == "batch_slab"),
        "wgrad/taps_as_stride1": wg(lambda c: len(c.probs) == 1 and c.probs[0]["conv"] == (2, 7, 5) and c.probs[0]["stride"] == 2 and c.probs[0]["xform"] == 0),
        "wgrad/no_scale": wg(lambda c: c.form == "slab" and c.R == 12),
        "wgrad/assign_not_add": wg(lambda c: c.form == "atomic" and c.R == 4),
        "cdgrad/no_oy_check": _find("cdgrad", B=3, hl=8, wl=6, stride=2, cin=64),
        "cdgrad/no_parity_check": _find("cdgrad", hl=8, wl=6, stride=2, cin=8, B=1, acc=0),
        "gemv/ignore_tcol": _find("gemv", nb=8, K=520),
        "gemv/mask_last_sample": _find("gemv", nb=8, K=1280),
        "ew/colsum_first_512_rows": _find("ew", op="colsum", geo=(3, 513)),
    }
