"""The attention kernels (csrc/attention.hip, csrc/attention_bwd.hip) element by element: the case matrix, the input classes, float64
references with derived per-element bounds, and plain-torch stand-ins of each kernel's arithmetic.  Importable without a GPU.

tests/test_attention_matrix_gpu.py runs every case on the device inside a fenced, NaN-prefilled arena; tests/test_host.py proves on the
CPU that the bounds admit the stand-ins (an honest implementation: 64-key tiles, fp32 accumulation, bf16 P and dS, running maximum,
key-split merge) and reject mutants of them, and that the matrix reaches every instantiation the library names
(lib.attn_fwd_kernel_name / lib.attn_bwd_kernel_names - the dispatch code itself answers, no rule is restated here).

Notation: eps = 2^-24 (one fp32 rounding; an n-term fp32 sum in any order is within n eps (sum of |terms|)), u = 2^-8 (bf16 round to
nearest).  s_j = scale (q . k_j) are the logits in natural-log units, M = max_j |s_j| of the row, c = scale log2(e).
"""
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from sliders_amd import lib
from tests.util import BF16_RND, FP32_EPS, elementwise_bound

BF, F32 = torch.bfloat16, torch.float32
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
FLUSH = 2.0 ** -126          # raw v_exp_f32 flushes results below the smallest normal to zero


def rup(x, q):
    return (x + q - 1) // q * q


def f32(x: float) -> float:
    """x as the float the descriptor carries"""
    return float(torch.tensor(x, dtype=F32))


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class FwdCase:
    B: int
    H: int
    Tq: int
    Tk: int
    D: int
    cls: str                  # input classes, letters of INPUT_CLASSES ("bc": peaked logits and a V offset)
    pack: str = "sep"         # "qkv": q|k|v columns of one [B T][3C] buffer (self-attention); "sep": three buffers
    ldo_pad: int = 0          # ldo = C + ldo_pad; the padding columns hold a NaN pattern that must survive
    vt_extra: int = 0         # vt_batch_heads = H + vt_extra: the layer's heads start one head into a wider transposed array
    pf: bool = False          # also run with pf_ptr / pf_bytes set: bit-identical results

    @property
    def id(self):
        x = ("" if self.pack == "sep" else " qkv") + (f" ldo+{self.ldo_pad}" if self.ldo_pad else "") + (f" vt+{self.vt_extra}" if self.vt_extra else "")
        return f"fwd B{self.B} H{self.H} Tq{self.Tq} Tk{self.Tk} D{self.D} [{self.cls}]{x}"


@dataclass(frozen=True)
class BwdCase:
    B: int
    H: int
    Tq: int
    Tk: int
    D: int
    cls: str
    do_cls: str = "n"         # dO: "n" randn, "o" randn + 1 (an offset: delta and dV no longer average out)
    need_dkv: int = 1
    pack: str = "sep"         # "qkv": q|k|v in one 3C buffer AND dq|dk|dv in one 3C gradient buffer (lddq = lddk = lddv = 3C)
    chained: bool = False     # o and lse come from the forward KERNEL (test_attention_matrix_gpu only): rel-L2 1.5e-2 instead of bounds

    @property
    def id(self):
        x = ("" if self.pack == "sep" else " qkv") + ("" if self.need_dkv else " dq-only") + (" chained" if self.chained else "")
        return f"bwd B{self.B} H{self.H} Tq{self.Tq} Tk{self.Tk} D{self.D} [{self.cls}/{self.do_cls}]{x}"


INPUT_CLASSES = {
    "a": "randn q, k, v",
    "b": "peaked: q x 5, logits with a standard deviation of 5",
    "c": "V = 0.5 randn + 1: |o| about 1, so the rounding statistic applies",
    "d": "q and k share an offset mu per channel, mu^2 sqrt(D) = 72: |s| up to about 90",
    "e": "rising maximum: key tile t carries an offset worth +12 t in the exponent, the row maximum moves in every tile",
    "f": "falling maximum: (e) reversed, the maximum is in tile 0 and alpha is exactly 1 afterwards",
    "g": "dominant last key: key Tk-1 leads every other key of its row by more than 30 in the exponent",
}

# Forward.  NW = 4 needs ceil(Tq / 128) H B >= 512; the key-split form D = 64, Tq % 64 == 0, Tk % 128 == 0, Tk >= 256 and a 64-query
# grid of 129..768 workgroups with fewer than 512 128-query workgroups - which form each case takes is asked of the library.
FWD_CASES: List[FwdCase] = [
    # --- 128-query workgroups (NW = 4): every DT x TAIL
    FwdCase(4, 16, 1024, 77, 64, "ac"),                     # <4, 1, true>: the cross-attention launch of the large latent levels
    FwdCase(4, 16, 1024, 64, 64, "ac"),                     # <4, 1, false>, a single tile
    FwdCase(4, 16, 1024, 192, 64, "bc", ldo_pad=8),         # <4, 1, false>, odd tile count
    FwdCase(4, 16, 1024, 77, 80, "ac", vt_extra=2),         # <4, 2, true>
    FwdCase(4, 16, 1024, 192, 80, "bc"),                    # <4, 2, false>
    FwdCase(4, 16, 1024, 77, 160, "ac"),                    # <4, 3, true>
    FwdCase(8, 64, 100, 77, 160, "g"),
    FwdCase(4, 16, 1024, 64, 160, "dc"),                    # <4, 3, false>
    FwdCase(4, 16, 1024, 192, 40, "ec"),                    # <4, 1, false>, D < 64
    # the last workgroup has whole waves without a valid row
    FwdCase(8, 64, 33, 65, 64, "g"),
    FwdCase(8, 64, 100, 5, 80, "b"),
    FwdCase(4, 64, 129, 77, 40, "a", ldo_pad=4),
    FwdCase(8, 32, 200, 128, 64, "d"),
    FwdCase(4, 16, 1057, 127, 64, "fc"),
    # --- 64-query workgroups (NW = 2)
    FwdCase(1, 3, 192, 192, 64, "a", pack="qkv"),           # <2, 1, false>, Tq = 64 * 3
    FwdCase(2, 4, 256, 192, 64, "bc"),
    FwdCase(2, 4, 256, 77, 64, "ac"),                       # <2, 1, true>
    FwdCase(1, 2, 100, 333, 64, "b"),
    FwdCase(2, 2, 33, 1, 64, "a"),                          # Tk = 1: softmax = 1, o = v exactly
    FwdCase(2, 2, 200, 1, 160, "d"),
    FwdCase(1, 2, 129, 5, 40, "b"),
    FwdCase(1, 2, 200, 65, 64, "g"),                        # one live key in the tail tile, and it dominates
    FwdCase(3, 4, 320, 127, 80, "ac"),                      # <2, 2, true>
    FwdCase(1, 2, 200, 77, 80, "g"),
    FwdCase(4, 4, 128, 128, 80, "bc", pack="qkv", ldo_pad=8),   # <2, 2, false>
    FwdCase(4, 4, 192, 127, 160, "ac"),                     # <2, 3, true>
    FwdCase(4, 4, 200, 64, 160, "bc", vt_extra=1),          # <2, 3, false>
    FwdCase(1, 4, 320, 1024, 64, "e"),                      # 16 tiles, the maximum moves in every one
    FwdCase(1, 4, 320, 1024, 64, "f"),                      # ... and in none but the first
    FwdCase(1, 4, 320, 1024, 64, "d"),
    FwdCase(2, 2, 1024, 1024, 160, "bc", pack="qkv"),
    FwdCase(1, 2, 448, 333, 80, "e"),
    # --- key split
    FwdCase(2, 10, 1024, 1024, 64, "ac", pack="qkv", pf=True),
    FwdCase(2, 10, 512, 256, 64, "bc", pf=True),
    FwdCase(1, 43, 192, 384, 64, "e", pf=True),             # exactly 129 workgroups, Tq = 64 * 3, three tiles per half
    FwdCase(6, 64, 128, 256, 64, "d"),                      # exactly 768 workgroups
    FwdCase(1, 30, 320, 384, 64, "f", pack="sep"),          # Tq = 64 * 5, three tiles per half
    FwdCase(1, 30, 320, 384, 64, "gc", ldo_pad=8, vt_extra=2),
    FwdCase(2, 5, 1024, 1024, 64, "e"),
    # either side of the 129..768 window: the plain forms
    FwdCase(1, 128, 64, 256, 64, "a"),                      # 128 workgroups
    FwdCase(1, 769, 64, 256, 64, "a"),                      # 769
]

BWD_CASES: List[BwdCase] = [
    # many trips through the dkv double buffer / the single-buffer DT = 3 loop, B > 1 and H > 1 for every DT
    BwdCase(2, 3, 1024, 1024, 64, "a", "n", pack="qkv"),
    BwdCase(2, 2, 1024, 1024, 80, "a", "o", pack="qkv"),
    BwdCase(2, 2, 1024, 1024, 160, "a", "n", pack="qkv"),
    # the rounding statistic applies: peaked logits make |dq|, |dk|, |dv| of order 1, no offset anywhere (bwd_takes_statistic)
    BwdCase(2, 4, 256, 256, 64, "b", "n", pack="qkv"),
    BwdCase(2, 4, 256, 256, 80, "b", "n"),
    BwdCase(2, 2, 256, 256, 160, "b", "n", pack="qkv"),
    # ragged Tq with dK / dV: the dkv kernel reads lse / delta past Tq (for the last head: the NaN padding)
    BwdCase(2, 2, 100, 100, 64, "a", "n", pack="qkv"),
    BwdCase(1, 3, 200, 333, 80, "b", "o"),
    BwdCase(2, 2, 129, 65, 160, "g", "n"),
    BwdCase(1, 1, 33, 192, 64, "d", "n"),
    BwdCase(2, 2, 1000, 77, 64, "gc", "o"),
    # ragged Tk, cross-attention (dq only) and with dK / dV
    BwdCase(2, 4, 256, 77, 64, "bc", "o", need_dkv=0),
    BwdCase(1, 2, 100, 77, 160, "a", "n", need_dkv=0),
    BwdCase(2, 2, 192, 5, 80, "b", "n", need_dkv=0),
    BwdCase(2, 2, 64, 1, 64, "a", "o", need_dkv=1),
    BwdCase(1, 2, 320, 448, 64, "e", "n"),
    BwdCase(1, 2, 320, 448, 80, "f", "o"),
    BwdCase(1, 2, 256, 256, 160, "d", "n", pack="qkv"),
    # chained forward -> backward, one per DT: the kernel's own o and lse, the former whole-tensor criterion
    BwdCase(2, 3, 320, 320, 64, "a", "n", pack="qkv", chained=True),
    BwdCase(2, 2, 200, 200, 80, "a", "n", pack="qkv", chained=True),
    BwdCase(2, 2, 192, 77, 160, "a", "n", chained=True),
]

FWD_NAMES = [f"attn_fwd_kernel<{nw}, {dt}, {tl}>" for nw in (2, 4) for dt in (1, 2, 3) for tl in ("false", "true")] + ["attn_fwd_ks_kernel"]
BWD_DQ_NAMES = [f"attn_bwd_dq_kernel<{dt}>" for dt in (1, 2, 3)]
BWD_DKV_NAMES = ["attn_bwd_dkv_kernel<1, 2>", "attn_bwd_dkv_kernel<2, 2>", "attn_bwd_dkv_kernel<3, 1>"]
TQ_EDGES = {"multiple of 128": lambda t: t % 128 == 0, "64 * odd": lambda t: t % 128 == 64, "33": lambda t: t == 33, "100": lambda t: t == 100,
            "129": lambda t: t == 129, "200": lambda t: t == 200}
TK_EDGES = (1, 5, 64, 65, 77, 127, 128, 192, 333, 256, 384, 1024)


# ---------------------------------------------------------------------------------------------------------------------------
# buffers, descriptors
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class Buf:
    name: str
    rows: int
    cols: int                 # valid columns of a row
    ld: int
    dtype: torch.dtype
    role: str                 # "in"; "out" (NaN pre-fill, every valid element must be written); "t" (a transposed copy: NaN pre-fill,
    #                           written by slh_transpose_heads before the run, an input afterwards)
    wrows: Optional[int] = None   # "out": only the first wrows rows are writable (lse / delta: the 64-float padding is not)


_ESIZE = {BF: 2, F32: 4, torch.uint8: 1}
FENCE = 4096
FAKE_BASE = 0x7F0000000000


def fwd_bufs(c: FwdCase) -> List[Buf]:
    C, Dp, Tkp = c.H * c.D, rup(c.D, 64), rup(c.Tk, 64)
    HV = c.H + c.vt_extra
    b = []
    if c.pack == "qkv":
        assert c.Tq == c.Tk and not c.vt_extra
        b.append(Buf("qkv", c.B * c.Tq, 3 * C, 3 * C, BF, "in"))
    else:
        b += [Buf("q", c.B * c.Tq, C, C, BF, "in"), Buf("k", c.B * c.Tk, C, C, BF, "in"), Buf("v", c.B * c.Tk, HV * c.D, HV * c.D, BF, "in")]
    b += [Buf("vt", c.B * HV * Dp, Tkp, Tkp, BF, "t"), Buf("o", c.B * c.Tq, C, C + c.ldo_pad, BF, "out"),
          Buf("lse", c.B * c.H * c.Tq + 64, 1, 1, F32, "out", wrows=c.B * c.H * c.Tq)]
    if c.pf:
        b.append(Buf("pf", 1, 3_000_017, 3_000_032, torch.uint8, "in"))
    return b


def bwd_bufs(c: BwdCase) -> List[Buf]:
    C, Dp, Tkp, Tqp = c.H * c.D, rup(c.D, 64), rup(c.Tk, 64), rup(c.Tq, 64)
    n = c.B * c.H * c.Tq
    b = []
    if c.pack == "qkv":
        assert c.Tq == c.Tk and c.need_dkv
        b.append(Buf("qkv", c.B * c.Tq, 3 * C, 3 * C, BF, "in"))
    else:
        b += [Buf("q", c.B * c.Tq, C, C, BF, "in"), Buf("k", c.B * c.Tk, C, C, BF, "in"), Buf("v", c.B * c.Tk, C, C, BF, "in")]
    b += [Buf("o", c.B * c.Tq, C, C, BF, "in"), Buf("do", c.B * c.Tq, C, C, BF, "in"), Buf("kt", c.B * c.H * Dp, Tkp, Tkp, BF, "t"),
          Buf("lse", n + 64, 1, 1, F32, "in"), Buf("delta", n + 64, 1, 1, F32, "out", wrows=n)]
    if c.need_dkv:
        b += [Buf("qt", c.B * c.H * Dp, Tqp, Tqp, BF, "t"), Buf("dot", c.B * c.H * Dp, Tqp, Tqp, BF, "t")]
    if c.pack == "qkv":
        b.append(Buf("dqkv", c.B * c.Tq, 3 * C, 3 * C, BF, "out"))
    else:
        b.append(Buf("dq", c.B * c.Tq, C, C, BF, "out"))
        if c.need_dkv:
            b += [Buf("dk", c.B * c.Tk, C, C, BF, "out"), Buf("dv", c.B * c.Tk, C, C, BF, "out")]
    return b


def layout(bufs: List[Buf]) -> Tuple[Dict[str, int], int]:
    """byte offset of every buffer in the case's one allocation (256-byte aligned, >= 4 KiB of fence on each side), and its size"""
    off, pos = {}, FENCE
    for b in bufs:
        off[b.name] = pos
        pos = rup(pos + b.rows * b.ld * _ESIZE[b.dtype] + FENCE, 256)
    return off, pos


def fwd_desc(c: FwdCase, base: int = FAKE_BASE, off: Optional[Dict[str, int]] = None, pf: bool = False):
    off = off if off is not None else layout(fwd_bufs(c))[0]
    C, Dp, Tkp = c.H * c.D, rup(c.D, 64), rup(c.Tk, 64)
    if c.pack == "qkv":
        q, k, ldq, ldk = base + off["qkv"], base + off["qkv"] + 2 * C, 3 * C, 3 * C
    else:
        q, k, ldq, ldk = base + off["q"], base + off["k"], C, C
    first = 1 if c.vt_extra else 0
    return lib.AttnDesc(q=q, k=k, vt=base + off["vt"] + 2 * first * Dp * Tkp, o=base + off["o"], lse=base + off["lse"], B=c.B, H=c.H, Tq=c.Tq,
                        Tk=c.Tk, ldq=ldq, ldk=ldk, ldvt=Tkp, ldo=C + c.ldo_pad, scale=c.D ** -0.5, D=c.D,
                        vt_batch_heads=(c.H + c.vt_extra) if c.vt_extra else 0,
                        pf_ptr=(base + off["pf"]) if pf else 0, pf_bytes=3_000_017 if pf else 0)


def bwd_desc(c: BwdCase, base: int = FAKE_BASE, off: Optional[Dict[str, int]] = None):
    off = off if off is not None else layout(bwd_bufs(c))[0]
    C, Tkp, Tqp = c.H * c.D, rup(c.Tk, 64), rup(c.Tq, 64)
    at = lambda n, col=0: base + off[n] + 2 * col
    if c.pack == "qkv":
        kw = dict(q=at("qkv"), k=at("qkv", C), v=at("qkv", 2 * C), ldq=3 * C, ldk=3 * C, ldv=3 * C,
                  dq=at("dqkv"), dk=at("dqkv", C), dv=at("dqkv", 2 * C), lddq=3 * C, lddk=3 * C, lddv=3 * C)
    else:
        kw = dict(q=at("q"), k=at("k"), v=at("v"), ldq=C, ldk=C, ldv=C, dq=at("dq"), lddq=C, lddk=C, lddv=C)
        if c.need_dkv:
            kw.update(dk=at("dk"), dv=at("dv"))
    if c.need_dkv:
        kw.update(qt=at("qt"), dot=at("dot"))
    return lib.AttnBwdDesc(o=at("o"), d_o=at("do"), kt=at("kt"), lse=at("lse"), delta=at("delta"), B=c.B, H=c.H, Tq=c.Tq, Tk=c.Tk, ldo=C,
                           lddo=C, ldkt=Tkp, ldqt=Tqp, scale=c.D ** -0.5, need_dkv=c.need_dkv, D=c.D, **kw)


def fwd_name(c: FwdCase) -> str:
    return lib.attn_fwd_kernel_name(fwd_desc(c))


def bwd_names(c: BwdCase) -> Tuple[str, str]:
    return lib.attn_bwd_kernel_names(bwd_desc(c))


_NAN16, _NAN32 = 0x7FC1, 0x7FC00001


class Arena:
    """One allocation per case: the byte pattern 0xA5 everywhere, the case's buffers as views into it with 4 KiB fences between them."""

    def __init__(self, bufs: List[Buf], dev):
        self.bufs = {b.name: b for b in bufs}
        self.off, self.size = layout(bufs)
        self.mem = torch.empty(self.size, dtype=torch.uint8, device=dev)
        self.mem.fill_(0xA5)
        self.base = self.mem.data_ptr()
        assert self.base % 256 == 0 or str(dev) == "cpu"
        self.writable = torch.zeros(self.size, dtype=torch.bool, device=dev)
        for b in bufs:
            if b.role == "out":
                self._bytes(b, self.writable, b.wrows)[:, :b.cols * _ESIZE[b.dtype]] = True
            if b.role in ("out", "t"):
                self.nan_fill(b.name)
        self.snap = None

    def _bytes(self, b: Buf, mem, rows=None):
        rows = b.rows if rows is None else rows
        es = _ESIZE[b.dtype]
        return mem[self.off[b.name]:self.off[b.name] + rows * b.ld * es].view(rows, b.ld * es)

    def full(self, name):
        """[rows][ld] view, padding columns (and padding rows) included"""
        b = self.bufs[name]
        return self._bytes(b, self.mem).view(b.dtype)

    def view(self, name):
        """the writable / valid part: [wrows or rows][cols]"""
        b = self.bufs[name]
        return self.full(name)[:b.wrows if b.wrows is not None else b.rows, :b.cols]

    def nan_fill(self, name):
        """the whole buffer, padding included, to a recognisable NaN pattern"""
        b = self.bufs[name]
        if b.dtype == BF:
            self.full(name).view(torch.int16).fill_(_NAN16)
        else:
            self.full(name).view(torch.int32).fill_(_NAN32)

    def refill_outputs(self):
        for b in self.bufs.values():
            if b.role == "out":
                self.nan_fill(b.name)

    def freeze(self):
        self.snap = self.mem.clone()

    def untouched_outside_outputs(self) -> bool:
        keep = ~self.writable
        return bool(torch.equal(self.mem[keep], self.snap[keep]))


# ---------------------------------------------------------------------------------------------------------------------------
# inputs.  Everything is rounded to bf16 here, before any reference sees it.  Tensors are [B][T][H][D].
# ---------------------------------------------------------------------------------------------------------------------------
def make_inputs(c, dev, seed: int) -> Dict[str, torch.Tensor]:
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev, dtype=F32)
    B, H, Tq, Tk, D = c.B, c.H, c.Tq, c.Tk, c.D
    q, k, v = rn(B, Tq, H, D), rn(B, Tk, H, D), rn(B, Tk, H, D)
    rD = math.sqrt(D)
    tile = (torch.arange(Tk, device=dev) // 64).to(F32).view(1, Tk, 1, 1)
    for ch in c.cls:
        assert ch in INPUT_CLASSES, ch
    if "b" in c.cls:
        q = q * 5.0
    if "c" in c.cls:
        v = v * 0.5 + 1.0
    if "d" in c.cls:
        mu = math.sqrt(72.0 / rD)                       # s = scale (q . k) ~ scale D mu^2 = 72, plus noise of a few mu
        q, k = q + mu, k + mu
    if "e" in c.cls or "f" in c.cls:
        # q = x/2 + 4, k_j = y_j/4 + delta t_j: s_ij = delta t_j (4 sqrt(D) + z_i / 2) + O(1), with delta = 12 / (4 sqrt(D)) a step of
        # about 12 per tile for every row (z_i ~ N(0, 1)); (f) numbers the tiles backwards
        t = tile if "e" in c.cls else (tile.max() - tile)
        q = q * 0.5 + 4.0
        k = k * 0.25 + (12.0 / (4.0 * rD)) * t
    if "g" in c.cls:
        # q = x + 2; the last key gets + eta with eta (2 sqrt(D) + z_i) ~ 60: the others reach scale (2 sum y + x . y) ~ N(0, 5), so the
        # lead stays above 30 (the reference itself is asked in the CPU proof)
        q = q + 2.0
        k = k.clone()
        k[:, Tk - 1] += 60.0 / (2.0 * rD)
    out = {"q": q.to(BF), "k": k.to(BF), "v": v.to(BF)}
    if isinstance(c, BwdCase):
        do = rn(B, Tq, H, D)
        out["do"] = (do + 1.0 if c.do_cls == "o" else do).to(BF)
    return out


def bwd_takes_statistic(c: BwdCase) -> bool:
    """The rounding statistic presumes errors that are independent from element to element.  dK_j = scale sum_q dS_qj Q_q: with an
    offset mu shared by the channels of q (classes d - g) every Q_q is close to mu (1, ..., 1), so the D elements of a dK row share ONE
    error term, sum_q err(dS_qj), and there are B H Tk independent samples, not B H Tk D; the same holds for dQ with an offset in k and
    for dV = P^T dO with an offset in dO.  (An honest stand-in reaches |b| = 0.06 on class d at D = 160 that way.)  So the statistic is
    taken where q, k and dO are centred: classes a, b, c with dO of class n.  The forward output always takes it: V's offset (class c)
    ties the D elements of an o row together as well, but every forward case that counts on it has at least 2048 rows."""
    return set(c.cls) <= set("abc") and c.do_cls == "n"


def heads(t):
    """[B][T][H][D] -> [B][H][T][D]"""
    return t.permute(0, 2, 1, 3)


def rows(t):
    """[B][H][T][D] -> [B T][H D]"""
    B, H, T, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * T, H * D)


# ---------------------------------------------------------------------------------------------------------------------------
# references and bounds (float64, on whatever device the inputs live on, a few heads at a time)
# ---------------------------------------------------------------------------------------------------------------------------
def _chunks(BH: int, Tq: int, Tk: int):
    per = max(1, (6 << 20) // max(1, Tq * rup(Tk, 64)))       # <= 6 M score elements (48 MB in float64) per temporary
    return [(i, min(BH, i + per)) for i in range(0, BH, per)]


def forward_reference(q, k, v, scale: float):
    """q [B][H][Tq][D], k, v [B][H][Tk][D] (bf16 values) -> (o, bound_o, lse2, bound_lse) in float64; o [B][H][Tq][D], lse2 [B][H][Tq] in
    the log2 domain.  The reference is softmax(scale q k^T) v with the fp32 value of scale the descriptor carries.

    What the kernels (attn_fwd_kernel, attn_fwd_ks_kernel) do per row, over nt = ceil(Tk / 64) key tiles: raw scores r_j = q . k_j as
    fp32 MFMA sums of D products (each exact), the running maximum m over the tiles seen, p_j = v_exp(fma(r_j, c, -fl(m c))), the
    denominator l = l alpha + sum p_j from the UNROUNDED p_j, o = o alpha + bf16(p_j) v_j by MFMA, alpha = v_exp(fl(fl(m_old - m) c)),
    at the end o / l as o * fl(1 / l), rounded to bf16, and lse2 = fl(m c) + log2f(l).  The key-split form runs two such chains over the
    two halves of the keys and merges them with one more pair of alphas.

    Exponent error of key j, in natural-log units, against s_j - (whatever is common to the row - a common shift cancels between
    numerator and denominator):
      (i)   r_j is a D-term fp32 sum (D + 2 counted: the MFMA's own accumulate order is not specified)  scale (D + 2) eps |q| . |k_j|
      (ii)  c = fl(scale * fl(log2 e)) carries two roundings, acting on s_j - m: 2 eps (|s_j| + M); fl(m c) rounds once: eps M;
            the fma rounds once: eps (|s_j| + M)                                                         <= 4 eps (|s_j| + M)
      (iii) v_exp_f32 is accurate to 1 ulp: 2 eps relative to p_j, i.e. 2 eps in the exponent            2 eps
      (iv)  each later tile multiplies what key j contributed by alpha: fl(m_old - m) rounds (eps 2M), the product with c rounds and c
            carries two roundings (3 eps 2M), v_exp 2 eps: at most 8 eps M + 2 eps per tile, nt of them (the first alpha is exactly 0
            times 0; the key-split merge is one more, and each half has at most nt / 2 tiles)            nt (8 eps M + 2 eps)
      Delta = the row maximum over j of (i) + (ii) + (iii) + (iv).
    Every unnormalised weight is then off by a factor within e^{+-Delta}, so is their sum, so every normalised weight w_j by a factor
    within e^{+-2 Delta}:  |do| <= (e^{2 Delta} - 1) A,  A = sum_j w_j |v_j|.
    bf16 rounding of p_j in front of P.V: u e^{2 Delta} A.
    fp32 arithmetic behind it, each step relative to A: the P.V sum over Tkp = 64 nt keys (Tkp), one rounding per tile for o alpha (nt),
    the denominator - 32 + 1 adds per lane and tile, the two half rows joined at the end (Tkp / 2 + 1), l alpha + ps two roundings per
    tile (2 nt) -, the reciprocal (v_rcp_f32 is accurate to 1 ulp: 2) and the final product (1), the merge of the key-split form o a0 + o' a1 and
    l a0 + l' a1 (6):
        n = 1.5 Tkp + 3 nt + 10.
    A p_j below 2^-126 is flushed to zero by v_exp: 2^-126 |v_j| each, relative to l >= 1 (the row's maximum has p = 1).
    Output rounding: u |ref|.
        |got - ref| <= u |ref| + (expm1(2 Delta) + u e^{2 Delta} + n eps) A + 2^-126 sum_j |v_j|

    lse2 = log2 sum_j 2^{s_j log2 e}: every term's exponent is off by at most Delta (now as an absolute error: (i) - (iv) cover the score,
    c, the fma, the independently rounded fl(m c) inside and outside the exponent, and the alpha chain), the fp32 sum of the positive p_j
    adds n_l eps relative with n_l = Tkp / 2 + 2 nt + 4 (lane sums, l alpha + ps, the join, the key-split merge), both times log2 e in the
    log2 domain; fl(m c) outside: 3 eps |s_max| log2 e; log2f is accurate to 1 ulp: 2 eps |log2 l|; the final add rounds once: eps |lse2|.
        |got - ref| <= log2 e (Delta + n_l eps) + 2 eps |log2 l| + 3 eps |s_max| log2 e + eps |ref|"""
    B, H, Tq, D = q.shape
    Tk = k.shape[2]
    Tkp, nt = rup(Tk, 64), rup(Tk, 64) // 64
    sc, eps = f32(scale), FP32_EPS
    qd, kd, vd = (t.reshape(B * H, -1, D).double() for t in (q, k, v))
    o, bo = torch.empty_like(qd), torch.empty_like(qd)
    ls, bl = torch.empty(B * H, Tq, dtype=torch.float64, device=q.device), torch.empty(B * H, Tq, dtype=torch.float64, device=q.device)
    n_o, n_l = 1.5 * Tkp + 3 * nt + 10, Tkp / 2 + 2 * nt + 4
    for a, b in _chunks(B * H, Tq, Tk):
        qq, kk, vv = qd[a:b], kd[a:b], vd[a:b]
        s = (qq @ kk.transpose(-1, -2)) * sc
        M = s.abs().amax(-1, keepdim=True)
        dl = sc * (D + 2) * eps * (qq.abs() @ kk.abs().transpose(-1, -2)) + 4 * eps * (s.abs() + M) + 2 * eps + nt * (8 * eps * M + 2 * eps)
        Dl = dl.amax(-1, keepdim=True)
        del dl
        w = torch.softmax(s, -1)
        ref, A = w @ vv, w @ vv.abs()
        o[a:b] = ref
        bo[a:b] = BF16_RND * ref.abs() + (torch.expm1(2 * Dl) + BF16_RND * torch.exp(2 * Dl) + n_o * eps) * A + FLUSH * vv.abs().sum(-2, keepdim=True)
        lse = torch.logsumexp(s, -1) * LOG2E
        smax = s.amax(-1)
        ls[a:b] = lse
        bl[a:b] = LOG2E * (Dl[..., 0] + n_l * eps) + 2 * eps * (lse - smax * LOG2E).abs() + 3 * eps * smax.abs() * LOG2E + eps * lse.abs()
    return o.view(B, H, Tq, D), bo.view(B, H, Tq, D), ls.view(B, H, Tq), bl.view(B, H, Tq)


def backward_reference(q, k, v, o, do, lse2, scale: float, need_dkv: bool = True):
    """The float64 formula of csrc/attention_bwd.hip's header on exactly the tensors the kernel is given - q, k, v, o, dO in bf16 and
    lse2 in fp32, all [B][H][T][D] / [B][H][Tq]:
        delta_q = sum_d dO o,  P = 2^{S c - lse2},  dP = dO V^T,  dS = P (dP - delta),  dQ = scale dS K,  dK = scale dS^T Q,  dV = P^T dO
    -> {name: (ref, bound)} for delta, dq and (need_dkv) dk, dv.

    What the kernels do: delta as a D-term fp32 sum of exact products (attn_delta_kernel); per 64 x 32 score tile r = q . k and dP as
    D-term fp32 MFMA sums, p = v_exp(fl(r c) - lse2) (or the fused form), ds = bf16(fl(p fl(dP - delta))), p to bf16 for dV; then
    dQ / dK / dV as fp32 MFMA sums over all keys / queries of the padded tiles, times scale for dQ and dK, rounded to bf16.
      e_delta = D eps sum_d |dO| |o|                              (also the bound on the delta output itself)
      exponent of p, natural-log units: the score (D + 2) eps scale |q| . |k|; c's two roundings, the product and the subtraction:
          eps (4 |s| + ln 2 |lse2|); v_exp 2 eps                 -> Delta_p, |p^ - p| <= expm1(Delta_p) p
      e_dP = (D + 2) eps |dO| . |v|
      ds before its bf16 rounding: |p^ x^ - p x| <= expm1(Delta_p) |ds| + e^{Delta_p} p (e_dP + e_delta) and three fp32 roundings (the
          subtraction, the product; 4 eps e^{Delta_p} |ds| counted)  =: e_pre;   E_ds = u |ds| + (1 + u) e_pre
      E_p = u p + (1 + u) expm1(Delta_p) p
      dQ: |got - ref| <= u |ref| + (Tkp + 2) eps scale (|ds| + E_ds) |K| + scale E_ds |K|       (Tkp-term fp32 sum, the product with scale)
      dK: the same over the queries, Tqp + 2;   dV: u |ref| + (Tqp + 1) eps (p + E_p)^T |dO| + E_p^T |dO|"""
    B, H, Tq, D = q.shape
    Tk = k.shape[2]
    Tkp, Tqp = rup(Tk, 64), rup(Tq, 64)
    sc, eps = f32(scale), FP32_EPS
    dev = q.device
    qd, kd, vd, od, gd = (t.reshape(B * H, -1, D).double() for t in (q, k, v, o, do))
    ld = lse2.reshape(B * H, Tq).double()
    z = lambda T: (torch.empty(B * H, T, D, dtype=torch.float64, device=dev), torch.empty(B * H, T, D, dtype=torch.float64, device=dev))
    dq, bq = z(Tq)
    dk, bk = z(Tk)
    dv, bv = z(Tk)
    delta = (gd * od).sum(-1)
    e_delta = D * eps * (gd.abs() * od.abs()).sum(-1)
    for a, b in _chunks(B * H, Tq, Tk):
        qq, kk, vv, gg = qd[a:b], kd[a:b], vd[a:b], gd[a:b]
        s = (qq @ kk.transpose(-1, -2)) * sc
        p = torch.exp2(s * LOG2E - ld[a:b, :, None])
        Dp = sc * (D + 2) * eps * (qq.abs() @ kk.abs().transpose(-1, -2)) + eps * (4 * s.abs() + LN2 * ld[a:b, :, None].abs()) + 2 * eps
        e_dp = (D + 2) * eps * (gg.abs() @ vv.abs().transpose(-1, -2))
        ds = p * (gg @ vv.transpose(-1, -2) - delta[a:b, :, None])
        e_pre = torch.expm1(Dp) * ds.abs() + torch.exp(Dp) * (p * (e_dp + e_delta[a:b, :, None]) + 4 * eps * ds.abs())
        E_ds = BF16_RND * ds.abs() + (1 + BF16_RND) * e_pre
        del e_pre, e_dp, s
        dq[a:b] = sc * (ds @ kk)
        R = sc * (E_ds @ kk.abs())
        bq[a:b] = elementwise_bound(dq[a:b], sc * (ds.abs() @ kk.abs()) + R, Tkp + 2, R)
        if need_dkv:
            dk[a:b] = sc * (ds.transpose(-1, -2) @ qq)
            R = sc * (E_ds.transpose(-1, -2) @ qq.abs())
            bk[a:b] = elementwise_bound(dk[a:b], sc * (ds.abs().transpose(-1, -2) @ qq.abs()) + R, Tqp + 2, R)
            E_p = BF16_RND * p + (1 + BF16_RND) * torch.expm1(Dp) * p
            dv[a:b] = p.transpose(-1, -2) @ gg
            R = E_p.transpose(-1, -2) @ gg.abs()
            bv[a:b] = elementwise_bound(dv[a:b], p.transpose(-1, -2) @ gg.abs() + R, Tqp + 1, R)
    sh = lambda t, T: t.view(B, H, T, D)
    out = {"delta": (delta.view(B, H, Tq), e_delta.view(B, H, Tq)), "dq": (sh(dq, Tq), sh(bq, Tq))}
    if need_dkv:
        out["dk"] = (sh(dk, Tk), sh(bk, Tk))
        out["dv"] = (sh(dv, Tk), sh(bv, Tk))
    return out


def forward_for_backward(q, k, v, scale: float):
    """the o (bf16) and lse2 (fp32) a backward case is handed: the float64 forward, rounded - so that the backward is judged on its own"""
    o, _, lse, _ = forward_reference(q, k, v, scale)
    return o.to(BF), lse.to(F32)


# ---------------------------------------------------------------------------------------------------------------------------
# stand-ins: each kernel's arithmetic in plain torch (fp32 tensors, any device); mutant = one deliberate defect
# ---------------------------------------------------------------------------------------------------------------------------
FWD_MUTANTS = ("p_trunc", "o_trunc", "drop_last_key", "no_tail_mask", "skip_rescale", "l_from_rounded_p", "ks_merge_without_a1")
BWD_MUTANTS = ("ds_trunc", "no_q_tail_zero", "ds_multiplied_not_selected", "dk_without_scale", "delta_of_next_head", "dq_no_kv_mask")


def _trunc_bf16(x):
    """fp32 -> bf16 by dropping the low 16 bits (towards zero)"""
    return (x.contiguous().view(torch.int32) & -65536).view(F32).to(BF)


def _fma(a, b, c):
    """fl32(a b + c) with one rounding"""
    return (a.double() * b.double() + c.double()).float()


def _exp2(x):
    r = torch.exp2(x.double()).float()
    return torch.where(r < FLUSH, torch.zeros_like(r), r)


def standin_forward(q, k, v, scale: float, key_split: bool = False, mutant: Optional[str] = None):
    """attn_fwd_kernel (key_split: attn_fwd_ks_kernel) in torch: q [B][H][Tq][D], k, v [B][H][Tk][D] bf16 -> (o bf16, lse2 fp32).  Keys in
    tiles of 64; the rows past Tk of the last tile are key Tk - 1 again (the loader clamps) with V^T zero there, and masked to -1e30."""
    assert mutant is None or mutant in FWD_MUTANTS
    B, H, Tq, D = q.shape
    Tk = k.shape[2]
    Tkp, nt = rup(Tk, 64), rup(Tk, 64) // 64
    qf = q.float()
    kf = torch.cat([k.float(), k.float()[:, :, Tk - 1:Tk].expand(B, H, Tkp - Tk, D)], 2)
    vf = torch.cat([v.float(), torch.zeros(B, H, Tkp - Tk, D, device=q.device)], 2)
    c = torch.tensor(f32(scale), dtype=F32, device=q.device) * torch.tensor(LOG2E, dtype=F32, device=q.device)
    r = qf @ kf.transpose(-1, -2)
    if mutant == "drop_last_key":
        r[..., Tk - 1:] = -1e30
    elif mutant != "no_tail_mask":
        r[..., Tk:] = -1e30

    def chain(t0, t1):
        m = torch.full((B, H, Tq), -1e30, device=q.device)
        l = torch.zeros(B, H, Tq, device=q.device)
        o = torch.zeros(B, H, Tq, D, device=q.device)
        for t in range(t0, t1):
            st = r[..., t * 64:(t + 1) * 64]
            m_new = torch.maximum(m, st.amax(-1))
            alpha = _exp2((m - m_new) * c)
            mc = m_new * c
            m = m_new
            p = _exp2(_fma(st, c, -mc[..., None]))
            pb = _trunc_bf16(p) if mutant == "p_trunc" else p.to(BF)
            l = l * alpha + (pb.float() if mutant == "l_from_rounded_p" else p).sum(-1)
            if not (mutant == "skip_rescale" and t == t0 + 1):
                o = o * alpha[..., None]
            o = o + pb.float() @ vf[:, :, t * 64:(t + 1) * 64]
        return m, l, o

    if key_split:
        assert Tk % 128 == 0
        m0, l0, o0 = chain(0, nt // 2)
        m1, l1, o1 = chain(nt // 2, nt)
        m = torch.maximum(m0, m1)
        a0, a1 = _exp2((m0 - m) * c), _exp2((m1 - m) * c)
        if mutant == "ks_merge_without_a1":
            a1 = torch.ones_like(a1)
        l = l0 * a0 + l1 * a1
        o = o0 * a0[..., None] + o1 * a1[..., None]
    else:
        m, l, o = chain(0, nt)
    o = o * (1.0 / l)[..., None]
    return (_trunc_bf16(o) if mutant == "o_trunc" else o.to(BF)), m * c + torch.log2(l)


def standin_backward(q, k, v, o, do, lse_flat, delta_pad, scale: float, need_dkv: bool = True, mutant: Optional[str] = None):
    """attn_delta_kernel + attn_bwd_dq_kernel + attn_bwd_dkv_kernel in torch.  q, k, v, o, do [B][H][T][D] bf16; lse_flat: the fp32 array
    [B H Tq + 64] the kernel is handed, padding included; delta_pad: what the 64 floats behind delta hold.  The dkv kernel walks the
    queries in tiles of 64 and reads lse / delta at flat index (b H + h) Tq + q for q up to the padded Tq: the next head's values, or the
    padding.  Q and dO of those rows are row Tq - 1 again, Q^T and dO^T are zero there (slh_transpose_heads); likewise K / V rows past
    Tk in the dq kernel, with K^T zero there.  -> {"delta", "dq", "dk", "dv"} (delta fp32 [B][H][Tq], the rest bf16)."""
    assert mutant is None or mutant in BWD_MUTANTS
    B, H, Tq, D = q.shape
    Tk = k.shape[2]
    Tkp, Tqp = rup(Tk, 64), rup(Tq, 64)
    dev = q.device
    sc = torch.tensor(f32(scale), dtype=F32, device=dev)
    c = sc * torch.tensor(LOG2E, dtype=F32, device=dev)
    qf, kf, vf, gf = q.float(), k.float(), v.float(), do.float()
    delta = (gf * o.float()).sum(-1)
    lse = lse_flat[:B * H * Tq].view(B, H, Tq)
    dl = delta.roll(-1, 1) if mutant == "delta_of_next_head" else delta
    rnd = _trunc_bf16 if mutant == "ds_trunc" else (lambda x: x.to(BF))
    # dq: keys padded by repeating key Tk - 1, K^T zero there
    kc = torch.cat([kf, kf[:, :, Tk - 1:Tk].expand(B, H, Tkp - Tk, D)], 2)
    vc = torch.cat([vf, vf[:, :, Tk - 1:Tk].expand(B, H, Tkp - Tk, D)], 2)
    kz = torch.cat([kf, torch.zeros(B, H, Tkp - Tk, D, device=dev)], 2)
    p = _exp2((qf @ kc.transpose(-1, -2)) * c - lse[..., None])
    if mutant != "dq_no_kv_mask":
        p[..., Tk:] = 0.0
    ds = rnd(p * (gf @ vc.transpose(-1, -2) - dl[..., None])).float()
    out = {"delta": delta, "dq": ((ds @ kz) * sc).to(BF)}
    if need_dkv:
        # dkv: queries padded by repeating row Tq - 1, Q^T / dO^T zero there, lse / delta read on past the head's Tq values
        idx = (torch.arange(B * H, device=dev)[:, None] * Tq + torch.arange(Tqp, device=dev)[None]).view(B, H, Tqp)
        lp = lse_flat[idx]
        dp_ = torch.cat([dl.reshape(-1), delta_pad.to(dev).float()])[idx]
        qc = torch.cat([qf, qf[:, :, Tq - 1:Tq].expand(B, H, Tqp - Tq, D)], 2)
        gc = torch.cat([gf, gf[:, :, Tq - 1:Tq].expand(B, H, Tqp - Tq, D)], 2)
        qz = torch.cat([qf, torch.zeros(B, H, Tqp - Tq, D, device=dev)], 2)
        gz = torch.cat([gf, torch.zeros(B, H, Tqp - Tq, D, device=dev)], 2)
        p = _exp2((qc @ kf.transpose(-1, -2)) * c - lp[..., None])           # [B][H][Tqp][Tk]
        if mutant != "no_q_tail_zero":
            p[:, :, Tq:] = 0.0
        x = p * (gc @ vf.transpose(-1, -2) - dp_[..., None])
        if mutant not in ("ds_multiplied_not_selected", "no_q_tail_zero"):
            x[:, :, Tq:] = 0.0
        ds = rnd(x).float()
        dk = ds.transpose(-1, -2) @ qz
        out["dk"] = (dk if mutant == "dk_without_scale" else dk * sc).to(BF)
        out["dv"] = (p.to(BF).float().transpose(-1, -2) @ gz).to(BF)
    return out
