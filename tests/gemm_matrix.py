"""The slh_gemm test matrix: tile x recipe x shape, asked of the library's own capability rule.

enumerate_cases() builds one descriptor per (recipe, tile, split-K factor, weight layout, shape class) and asks slh_gemm_tile_ok
which of them the library accepts (no device needed: the rule only looks at shapes, flags and pointer alignment, so the CPU side
hands it made-up 256-byte aligned addresses - the alignment every fenced GPU buffer has too).  tests/test_gemm_matrix_gpu.py runs
every accepted case and one refused case per (tile, recipe); tests/test_host.py pins the accept matrix to
tests/data/gemm_capability.json (`python -m tests.gemm_matrix --write` records it) and the launch each accepted case and each product
of the dry-run plans would make - kernel, grid, block size, argument bytes - to tests/data/gemm_dispatch.json (`--write-dispatch`;
`--dispatch KEY` prints the tuples behind one of its digests).

A case is described without data first (plan_case: scalar descriptor fields + the list of buffers), then materialised into ONE
device allocation (Arena): every buffer is a slice with at least 4 KiB of pattern on each side and pattern in its padding
columns, outputs pre-filled with NaN.  reference() restates the operation in float64 from the same bf16-rounded inputs and returns,
per output, the reference and the element-wise bound of tests/util.py:

    |got - ref| <= 2^-8 |ref| + n 2^-24 S + R

S = the expression of ref on absolute values, n = number of summed terms, R = what an internal bf16 rounding adds.  The
derivations of the non-linear recipes are in _geglu_forward / _geglu_backward / _cross_attention.
"""
import functools
import hashlib
import json
import math
import os
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from sliders_amd import lib
from tests.util import BF16_RND, FP32_EPS, elementwise_bound

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "gemm_capability.json")
DISPATCH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "gemm_dispatch.json")

# ---------------------------------------------------------------------------------------------------------------------------
# tiles: every code the dispatch of csrc/gemm.hip, gemm8p.hip, gemm5.hip, gemm7.hip instantiates (the tuning tables and the
# existing tests name a subset of these; test_host.py checks that)
# ---------------------------------------------------------------------------------------------------------------------------
_RING = [(mi << 4) | ni for mi in (1, 2) for ni in (1, 2)]
TILES_R2 = [st << 8 | t for st in (0, 3, 4) for t in _RING]                                # 4 waves: 64 MI x 64 NI
TILES_R4 = [0x4000 | st << 8 | t for st in (0, 3, 4) for t in (0x11, 0x12, 0x22)]           # 8 waves: 128 MI x 64 NI
TILES_PP = [0x8042, 0x8013, 0x8014, 0x8015]                                                # ping-pong K loops
TILES_G5 = [0x5425, 0x5525]                                                                # 64 x 160
TILES_G7 = [0x7648, 0x7645, 0x748A]                                                        # 128 x 256, 128 x 160, 256 x 320
TILES = [0] + TILES_R2 + TILES_R4 + TILES_PP + TILES_G5 + TILES_G7
FAMILIES = ("auto", "r2", "r4", "pp", "g5", "g7")


def family(tile: int) -> str:
    t = tile & 0xFFFF
    if t == 0:
        return "auto"
    return {0: "r2", 4: "r4", 8: "pp", 5: "g5", 7: "g7"}[(t >> 12) & 15]


def block(tile: int) -> Tuple[int, int]:
    """(rows, columns) of the block tile; the heuristic's choice (tile 0) is treated as 128 x 128 for shape purposes"""
    t, fam = tile & 0xFFFF, family(tile)
    mi, ni = (t >> 4) & 15, t & 15
    if fam == "auto":
        return 128, 128
    if fam == "r2":
        return 64 * mi, 64 * ni
    if fam == "r4":
        return 128 * mi, 64 * ni
    if fam == "pp":
        return (256, 256) if mi == 4 else (128, 64 * ni)
    if fam == "g5":
        return 64, 160
    return 32 * mi, 32 * ni


# ---------------------------------------------------------------------------------------------------------------------------
# recipes
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Recipe:
    name: str
    bias: bool = False
    res: Optional[str] = None            # "alias": the residual IS c (in place), "sep": its own buffer with ld_res > N
    rowbias: bool = False                # per-sample row bias, the sample boundary inside a tile
    two_src: bool = False                # K split over two sources, lda1 != ca1
    lora: Optional[str] = None           # "ext": T from outside (lora_t), "fused": lora_down inside the launch
    groups: int = 1
    rmajor: int = 0                      # > 0: backward-data form, total rank
    t_out: bool = False
    geglu: int = 0
    pre: bool = False
    vt: int = 0                          # 1: vt_out, 2: + vt_also_c
    ln_out: bool = False
    ln_in: int = 0                       # chunk width 64 | 80
    ln_off: float = 0.0                  # row mean of the LayerNorm input
    mr_out: bool = False
    xa: int = 0                          # cross-attention keys
    conv: Optional[Tuple[int, int]] = None   # (stride, src_xform)
    pf: bool = False
    families: Tuple[str, ...] = ()       # families the header says take the recipe (checked against the rule on the CPU)


_ALL = ("auto", "r2", "r4", "pp", "g5", "g7")
_GEN = ("auto", "r2", "r4", "pp")        # gemm.hip + gemm8p.hip: everything the header lists without a family restriction


def _recipes() -> List[Recipe]:
    r = [Recipe("bare", families=_ALL),
         Recipe("bias_res_alias", bias=True, res="alias", families=_ALL),
         Recipe("bias_res_sep", bias=True, res="sep", families=_ALL),
         Recipe("rowbias", rowbias=True, families=_GEN),
         Recipe("two_src", two_src=True, bias=True, families=_GEN),
         Recipe("pf_touch", pf=True, families=_ALL)]
    for g in (1, 2, 3):
        r.append(Recipe(f"ext_t_g{g}", lora="ext", groups=g, bias=True, families=_GEN))
    for rk in (4, 8, 12):
        r.append(Recipe(f"ext_t_rmajor{rk}", lora="ext", rmajor=rk, families=_GEN))
    r.append(Recipe("fused_g1", lora="fused", groups=1, bias=True, t_out=True, families=("auto", "r2", "r4", "pp", "g5", "g7")))
    for g in (2, 3):
        r.append(Recipe(f"fused_g{g}", lora="fused", groups=g, bias=True, t_out=True, families=("auto", "r2", "r4", "pp", "g7")))
    for rk in (4, 12):
        r.append(Recipe(f"fused_rmajor{rk}", lora="fused", rmajor=rk, t_out=True, families=_GEN))
    r += [Recipe("geglu1", geglu=1, bias=True, families=_GEN),
          Recipe("geglu1_pre", geglu=1, bias=True, pre=True, families=_GEN),
          Recipe("geglu2", geglu=2, pre=True, families=_GEN),
          Recipe("geglu3", geglu=3, bias=True, families=("auto", "r2", "r4", "pp", "g7")),
          Recipe("vt", vt=1, families=("auto", "r2", "r4", "pp", "g7")),
          Recipe("vt_also_c", vt=2, bias=True, families=("auto", "r2", "r4", "pp", "g7")),
          Recipe("vt_fused_g3", vt=1, lora="fused", groups=3, families=("auto", "r2", "r4", "pp", "g7")),
          Recipe("ln_out", ln_out=True, bias=True, res="sep", families=_ALL)]
    for cw in (64, 80):
        for off in (0.0, 20.0):
            r.append(Recipe(f"ln_in{cw}_off{int(off)}", ln_in=cw, ln_off=off, mr_out=True, families=_ALL))
    r += [Recipe("ln_in_ln_out", ln_in=64, ln_out=True, res="sep", families=_ALL),
          Recipe("ln_in_geglu3", ln_in=64, geglu=3, families=("auto", "r2", "r4", "pp", "g7")),
          Recipe("ln_in_fused_g3", ln_in=64, ln_off=20.0, lora="fused", groups=3, families=("pp", "g7"))]
    for tk in (5, 64, 77, 96):
        r.append(Recipe(f"xa_tk{tk}", xa=tk, bias=True, families=("r4",)))
        r.append(Recipe(f"xa_tk{tk}_ln_in", xa=tk, ln_in=64, families=("r4",)))
    for stride, xf in ((1, 0), (2, 0), (1, 1), (1, 2)):
        r.append(Recipe(f"conv_s{stride}_x{xf}", conv=(stride, xf), bias=True, families=_GEN))
    r += [Recipe("conv_two_src", conv=(1, 0), two_src=True, families=_GEN),
          Recipe("conv_bias_rowbias_res", conv=(1, 0), bias=True, rowbias=True, res="sep", families=_GEN),
          Recipe("conv_s2_fused", conv=(2, 0), lora="fused", groups=1, t_out=True, bias=True, families=_GEN)]
    return r


RECIPES: List[Recipe] = _recipes()
RECIPE = {r.name: r for r in RECIPES}

# shape classes: (a) exact multiple of the block tile, 2 x 2 tiles, K = 320 (5 K tiles: S = 2 cuts 3 + 2, S = 3 cuts 2 + 2 + 1);
# (b) ragged M / N and every leading dimension wider than its row, K = 320; (kmin) K at the ring's minimum, never split;
# (kbig) K >= 2560 (41 K tiles: S = 2 cuts 21 + 20, S = 3 cuts 14 + 14 + 13; every ring slot wraps inside a slice);
# (small) N = 4, M = 24, K = 192 (S = 2 cuts 2 + 1)
SHAPE_CLASSES = ("a", "b", "kmin", "kbig", "small")
# (shape class, split-K factor, weight layout) combinations run per (tile, recipe)
AXES = [("a", 0, 0), ("a", 0, 1), ("a", 2, 0), ("a", 3, 1), ("b", 0, 0), ("b", 0, 1), ("b", 2, 1), ("b", 3, 0), ("kmin", 0, 0), ("kmin", 0, 1),
        ("kbig", 0, 1), ("kbig", 2, 0), ("kbig", 3, 0), ("kbig", 3, 1), ("small", 0, 0), ("small", 2, 1)]


def _rup(x, q):
    return (x + q - 1) // q * q


def _pp_ragged_n(n0: int, bn: int, q: int) -> int:
    """The widest ragged N <= n0 (a multiple of q, no multiple of the tile width bn, more than one tile) whose tile grid rounded up
    to bn still fits the split-K slab contract of the header, roundup(N, 128) columns - the ping-pong tiles are 192 - 320 columns
    wide, so most N just past a tile boundary do not (and are refused under split-K)."""
    n = n0
    while n > bn:
        if n % bn and _rup(n, bn) <= _rup(n, 128):
            return n
        n -= q
    return n0


def _dims(r: Recipe, tile: int, cls: str) -> Optional[dict]:
    """Shape of recipe r on this tile in shape class cls (None: the class does not exist for the recipe)."""
    bm, bn = block(tile)
    fam = family(tile)
    exact = fam in ("g5", "g7")                     # these families take whole tiles only: their (b) keeps M, N exact, pads the lds
    g = r.groups if r.lora and not r.rmajor else 1
    nq = 4 * g
    if r.geglu == 1 or r.ln_out or r.xa:
        nq = 64
    elif r.geglu in (2, 3):
        nq = 32
    d = dict(pad=cls == "b")
    if cls == "small":
        if nq != 4 or r.vt or r.conv or r.ln_in or exact:
            return None
        d.update(M=24, N=4, K=192)             # 3 K tiles: S = 2 cuts them 2 + 1
    elif cls == "a":
        d.update(M=2 * bm, N=max(2, g) * bn, K=320)          # 5 K tiles: S = 2 cuts them 3 + 2, S = 3 cuts them 2 + 2 + 1
    elif cls == "b":
        d.update(M=3 * bm if exact else 2 * bm + 40, N=(3 if g == 3 else 2) * bn + (0 if exact else nq), K=320)
        if fam == "pp":
            d["N"] = _pp_ragged_n(d["N"], bn, nq)
    elif cls == "kmin":
        d.update(M=2 * bm, N=max(2, g) * bn, K=64)
        if fam == "g7":
            d["K"] = 192 if ((tile >> 8) & 15) == 6 else 128
    else:
        # (ping-pong tiles: N a whole number of tiles, so that split-K's rounded tile grid fits the slab contract)
        d.update(M=bm if exact else bm + 8, N=g * bn if exact or fam == "pp" else g * bn + nq, K=2624)
    if r.two_src and not r.conv:
        d["K"] = max(d["K"], 128)
    if r.ln_in:
        if cls == "kbig":
            d["K"] = 1280
        if r.ln_in == 80:
            if cls == "kmin":
                return None
            d["K"] = 1280 if cls == "kbig" else 320
        if fam == "g7" and cls == "kmin":
            d["K"] = 192 if r.ln_in == 64 else 320
    if r.geglu == 2:
        d["N"] = _rup(d["N"], 32)
    if r.vt:
        if cls == "small":
            return None
        C = 320 if bn in (160, 320) else (256 if bn == 256 else 128)
        T = 256 if (exact and cls == "b") else (max(bm, 64) if cls in ("a", "kmin") or exact else max(bm, 64) + 8)
        d.update(N=3 * C, vt_C=C, vt_B=2, vt_T=T, M=2 * T)
    if r.xa:
        Tq = 256 if cls == "b" else 128
        d.update(M=2 * Tq, xa_tq=Tq, N=320 if cls in ("b", "kbig") else 256)
    if r.conv:
        stride, xf = r.conv
        cin = {"a": 64, "b": 128, "kmin": 64, "kbig": 320}[cls]
        if r.two_src:
            cin = max(cin, 128)
        if cls in ("a", "kmin"):
            ho, wo = 16, 16
        elif cls == "b":
            ho, wo = 9, 13
        else:
            ho, wo = 6, 11
        if xf:
            ho, wo = ho + ho % 2, wo + wo % 2
            hs, ws = ho // 2, wo // 2
        elif stride == 2:
            hs, ws = 2 * ho - 1, 2 * wo          # odd source height: the last output row reads one row of padding
        else:
            hs, ws = ho, wo
        if cls in ("a", "kmin"):
            B = max(1, 2 * bm // 256)
        else:
            B = 3
        d.update(batch=B, hs=hs, ws=ws, ho=ho, wo=wo, cin=cin, K=9 * cin, M=B * ho * wo)
    return d


@dataclass
class Buf:
    name: str
    rows: int
    cols: int
    ld: int
    dtype: torch.dtype
    role: str                 # "in", "out" (NaN pre-fill, every element must be written), "ws" (scratch, any contents), "zero" (tickets)
    fields: Tuple[str, ...] = ()      # descriptor pointer fields that point at this buffer
    col0: int = 0             # the pointer is handed over col0 elements into the row (a column window of a wider matrix)


@dataclass
class Case:
    recipe: Recipe
    tile: int                 # with the split-K factor in bits 16-19
    w_layout: int
    cls: str
    dims: dict
    fields: Dict[str, object] = field(default_factory=dict)
    bufs: List[Buf] = field(default_factory=list)
    ptr_off: Dict[str, Tuple[str, int]] = field(default_factory=dict)    # extra pointer fields: field -> (buffer, element offset)

    @property
    def key(self):
        return (self.recipe.name, self.cls, self.w_layout, (self.tile >> 16) & 15)

    @property
    def id(self):
        d = self.dims
        return f"{self.recipe.name} tile 0x{self.tile:x} wl{self.w_layout} {self.cls} M{d['M']} N{d['N']} K{d['K']}"

    def buf(self, name) -> Buf:
        return next(b for b in self.bufs if b.name == name)


BF, F32 = torch.bfloat16, torch.float32


def plan_case(r: Recipe, tile: int, S: int, wl: int, cls: str) -> Optional[Case]:
    """The case without data: descriptor scalars and the buffers it needs."""
    d = _dims(r, tile, cls)
    if d is None:
        return None
    M, N, K, pad = d["M"], d["N"], d["K"], d["pad"]
    c = Case(r, tile | (S << 16), wl, cls, d)
    f, bufs = c.fields, c.bufs
    px = 8 if pad else 0                                    # padding columns (elements) of every leading dimension
    f.update(M=M, N=N, K=K, mode=0, stride=1, rows_per_sample=M, tile=c.tile, w_layout=wl)
    # --- A operand
    if r.conv:
        stride, xf = r.conv
        cin, B = d["cin"], d["batch"]
        rows = B * d["hs"] * d["ws"]
        f.update(mode=1, batch=B, hs=d["hs"], ws=d["ws"], ho=d["ho"], wo=d["wo"], stride=stride, src_xform=xf,
                 rows_per_sample=d["ho"] * d["wo"])
        c0 = cin - 64 if r.two_src else cin
        bufs.append(Buf("a0", rows, c0, c0 + px, BF, "in", ("a0",)))
        f.update(lda0=c0 + px, ca0=c0)
        if r.two_src:
            bufs.append(Buf("a1", rows, 64, 128, BF, "in", ("a1",), col0=64))     # a column window: lda1 != ca1
            f.update(lda1=128, ca1=64)
    else:
        c0 = K - 64 if r.two_src else K
        bufs.append(Buf("a0", M, c0, c0 + px, BF, "in", ("a0",)))
        f.update(lda0=c0 + px, ca0=c0)
        if r.two_src:
            bufs.append(Buf("a1", M, 64, 128, BF, "in", ("a1",), col0=64))
            f.update(lda1=128, ca1=64)
    # --- weights
    if wl == 1:
        bufs.append(Buf("w", 1, _rup(N, 64) * K, _rup(N, 64) * K, BF, "in", ("w",)))
        f.update(ldw=0)
    else:
        bufs.append(Buf("w", N, K, K + px, BF, "in", ("w",)))
        f.update(ldw=K + px)
    # --- output
    ncols = 2 * N if r.geglu == 2 else (N // 2 if r.geglu else N)
    ldc = ncols + px
    bufs.append(Buf("c", M, ncols, ldc, BF, "out", ("c", "residual") if r.res == "alias" else ("c",)))
    f.update(ldc=ldc)
    if r.res == "alias":
        f.update(ld_res=ldc)
    elif r.res == "sep":
        bufs.append(Buf("res", M, N, N + 2 * px + 4, BF, "in", ("residual",)))
        f.update(ld_res=N + 2 * px + 4)
    if r.bias:
        bufs.append(Buf("bias", 1, N, N, BF, "in", ("bias",)))
    if r.rowbias:
        # three samples whose boundaries fall inside a 32-row block; the pointer is a column window of a wider matrix
        rps = d["ho"] * d["wo"] if r.conv else -(-M // 3) | 1
        nb = -(-M // rps)
        ldrb = _rup(N, 4) + 64
        bufs.append(Buf("rowbias", nb, N, ldrb, BF, "in", ("rowbias",), col0=32))
        f.update(ld_rowbias=ldrb, rows_per_sample=rps)
    # --- adapters
    if r.lora:
        rank = r.rmajor or 4 * r.groups
        ldt = rank + (4 if pad else 0)
        bufs.append(Buf("scale", 1, 1, 64, F32, "in", ("lora_scale",)))
        if r.rmajor:
            bufs.append(Buf("up", rank, N, N, BF, "in", ("lora_up",)))          # [rank][N]: the down matrices as stored
            f.update(lora_up_rmajor=1, lora_groups=1, lora_rank=rank)
        else:
            bufs.append(Buf("up", N, 4, 4, BF, "in", ("lora_up",)))
            f.update(lora_groups=r.groups, lora_rank=rank)
        f.update(ld_t=ldt)
        if r.lora == "ext":
            bufs.append(Buf("T", M, rank, ldt, F32, "in", ("lora_t",)))
        else:
            bufs.append(Buf("down", rank, K, K, BF, "in", ("lora_down",)))
            if r.t_out:
                bufs.append(Buf("t_out", M, rank, ldt, F32, "out", ("lora_t_out",)))
            if r.ln_in:
                bufs.append(Buf("ln_lora_s", 1, rank, 16, F32, "in", ("ln_lora_s",)))
                bufs.append(Buf("ln_lora_c", 1, rank, 16, F32, "in", ("ln_lora_c",)))
    # --- GEGLU
    if r.pre:
        wpre = 2 * N if r.geglu == 2 else N
        bufs.append(Buf("pre", M, wpre, wpre + px, BF, "in" if r.geglu == 2 else "out", ("geglu_pre",)))
        f.update(ld_pre=wpre + px)
    f.update(geglu=r.geglu)
    # --- head-transposed V
    if r.vt:
        C, B, T = d["vt_C"], d["vt_B"], d["vt_T"]
        vld = T                                            # vt_ld == vt_tokens (the rule refuses padding columns)
        bufs.append(Buf("vt", B * (C // 64) * 64, T, vld, BF, "out", ("vt_out",)))
        f.update(vt_col0=2 * C, vt_D=64, vt_heads=C // 64, vt_tokens=T, vt_ld=vld, vt_also_c=int(r.vt == 2), rows_per_sample=T)
    # --- LayerNorm fold
    if r.ln_out:
        bufs.append(Buf("ln_out", 1, 0, 0, F32, "out", ("ln_out",)))            # sized once the tile's chunk width is known
    if r.ln_in:
        chunks = K // r.ln_in
        bufs.append(Buf("ln_in", chunks * M, 2, 2, F32, "in", ("ln_in",)))
        bufs.append(Buf("ln_s", 1, N, N, F32, "in", ("ln_s",)))
        bufs.append(Buf("ln_b", 1, N, N, F32, "in", ("ln_b",)))
        f.update(ln_in_chunks=chunks, ln_eps=1e-5)
        if r.mr_out:
            bufs.append(Buf("mr", M, 2, 2, F32, "out", ("ln_mr_out",)))
    # --- cross-attention
    if r.xa:
        H, B, tk = N // 64, M // d["xa_tq"], r.xa
        ldk = N + 64
        bufs.append(Buf("xa_k", B * tk, N, ldk, BF, "in", ("xa_k",), col0=32))
        bufs.append(Buf("xa_vt", B * (H + 3) * 64, 128, 128, BF, "in"))
        c.ptr_off["xa_vt"] = ("xa_vt", 2 * 64 * 128)                              # this layer's first head inside a wider array
        f.update(xa_tk=tk, xa_tq=d["xa_tq"], xa_ldk=ldk, xa_ldvt=128, xa_vt_heads=H + 3, xa_scale=0.125)
    # --- split-K workspace: one slab more than the launch may use (it must stay untouched)
    if S > 1:
        slab = _rup(M, 256) * _rup(N, 128)
        bufs.append(Buf("slabs", S + 1, slab, slab, F32, "ws", ("splitk_c32",)))
        bufs.append(Buf("tickets", 1, _rup(M, 64) // 64 * (_rup(N, 64) // 64), _rup(M, 64) // 64 * (_rup(N, 64) // 64), torch.int64, "zero",
                        ("splitk_ticket",)))
        f.update(splitk_slabs=S)
        if r.lora == "fused":
            rank = r.rmajor or 4 * r.groups
            n32 = _rup(N, 64) // 64 * 2 * S * M * f["ld_t"]
            bufs.append(Buf("t32", 1, n32, n32, F32, "ws", ("splitk_t32",)))
    if r.pf:
        bufs.append(Buf("pf", 1, 40961, 40961, torch.uint8, "in", ("pf_ptr",)))
        f.update(pf_bytes=40961)
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# descriptors and the enumeration
# ---------------------------------------------------------------------------------------------------------------------------
_ESIZE = {BF: 2, F32: 4, torch.int64: 8, torch.uint8: 1}
FENCE = 4096


def layout(case: Case) -> Tuple[Dict[str, int], int]:
    """Byte offset of every buffer inside the case's single allocation (256-byte aligned, >= 4 KiB of fence on each side) and the
    allocation's size.  ln_out must have been sized (size_ln_out) first."""
    off, pos = {}, FENCE
    for b in case.bufs:
        off[b.name] = pos
        pos = _rup(pos + b.rows * b.ld * _ESIZE[b.dtype] + FENCE, 256)
    return off, pos


def make_desc(case: Case, base: int, off: Dict[str, int], tile: Optional[int] = None):
    kw = dict(case.fields)
    if tile is not None:
        kw["tile"] = tile
    for b in case.bufs:
        for fld in b.fields:
            kw[fld] = base + off[b.name] + b.col0 * _ESIZE[b.dtype]
    for fld, (bn, eo) in case.ptr_off.items():
        kw[fld] = base + off[bn] + eo * _ESIZE[case.buf(bn).dtype]
    return lib.GemmDesc(**kw)


_FAKE_BASE = 0x7F0000000000        # a made-up, 4 KiB aligned address: the rule only looks at alignment


def size_ln_out(case: Case) -> None:
    """ln_out is [N / width][M][2] with the width the TILE writes (slh_gemm_ln_chunk_cols); 64 where the rule refuses the case"""
    if not case.recipe.ln_out:
        return
    b = case.buf("ln_out")
    b.rows, b.cols, b.ld = 1, 2, 2                      # any non-null, aligned pointer for the query
    off, _ = layout(case)
    cw = lib.gemm_ln_chunk_cols(make_desc(case, _FAKE_BASE, off)) or 64
    case.dims["ln_cw"] = cw
    M, N = case.dims["M"], case.dims["N"]
    b.rows, b.cols, b.ld = -(-N // cw) * M, 2, 2


def accepted(case: Case) -> bool:
    off, _ = layout(case)
    return lib.gemm_tile_ok(make_desc(case, _FAKE_BASE, off))


@functools.lru_cache(maxsize=1)
def enumerate_cases() -> Tuple[List[Case], List[Case]]:
    """(accepted, refused) cases of the whole matrix, in a fixed order (computed once per process)"""
    acc, ref = [], []
    for r in RECIPES:
        for tile in TILES:
            for cls, S, wl in AXES:
                c = plan_case(r, tile, S, wl, cls)
                if c is None:
                    continue
                size_ln_out(c)
                (acc if accepted(c) else ref).append(c)
    return acc, ref


def capability_table(acc: List[Case]) -> Dict[str, List[str]]:
    t: Dict[str, List[str]] = {}
    for c in acc:
        rn, cls, wl, S = c.key
        t.setdefault(f"{rn}|{cls}|wl{wl}|S{S}", []).append(f"0x{c.tile & 0xFFFF:x}")
    return {k: sorted(v, key=lambda s: int(s, 16)) for k, v in sorted(t.items())}


# ---------------------------------------------------------------------------------------------------------------------------
# the launch behind every accepted case and every product of the dry-run plans (slh_gemm_launch_query: no device needed)
# ---------------------------------------------------------------------------------------------------------------------------
PLAN_CASES = [("tiny_sdxl", 16, "noxattn"), ("tiny_sd1", 16, "full"), ("sdxl", 128, "noxattn"), ("sdxl", 64, "noxattn")]
PLAN_MODES = ("off", "on", "train")


def _launch_line(tile: int, q) -> str:
    name, grid, block, h = q
    return f"0x{tile:x} {name} grid {grid} block {block} args {h:016x}"


def dispatch_matrix(acc: List[Case]) -> Dict[str, List[str]]:
    """capability-table key -> the sorted (tile, kernel name, grid, block, args hash) lines of its accepted cases"""
    t: Dict[str, List[Tuple[int, str]]] = {}
    for c in acc:
        rn, cls, wl, S = c.key
        off, _ = layout(c)
        q = lib.gemm_launch_query(make_desc(c, _FAKE_BASE, off))
        t.setdefault(f"{rn}|{cls}|wl{wl}|S{S}", []).append((c.tile, _launch_line(c.tile, q)))
    return {k: [ln for _, ln in sorted(v)] for k, v in sorted(t.items())}


def dispatch_plans() -> Dict[str, List[str]]:
    """dry-run plan (tests/plan_digest.py: every pointer a function of what it names) -> the launch lines of its OP_GEMM descriptors in
    program order, the backward program behind the training forward"""
    from tests import plan_digest
    out = {}
    for name, hw, method in PLAN_CASES:
        for mode in PLAN_MODES:
            p, bw, _, _ = plan_digest.plan(name, hw, method, mode)
            progs = [p.prog] + ([bw.prog] if bw is not None else [])
            out[f"{name}|{hw}|{method}|{mode}"] = [_launch_line(d.tile, lib.gemm_launch_query(d))
                                                  for pr in progs for o, d in pr.ops if o == lib.OP_GEMM]
    return out


def dispatch_lines(acc: List[Case]) -> Dict[str, Dict[str, List[str]]]:
    return {"matrix": dispatch_matrix(acc), "plans": dispatch_plans()}


def dispatch_digests(acc: List[Case]) -> Dict[str, Dict[str, str]]:
    """what tests/data/gemm_dispatch.json holds: one SHA-256 per key over its launch lines"""
    return {sec: {k: hashlib.sha256("\n".join(v).encode()).hexdigest() for k, v in rows.items()}
            for sec, rows in dispatch_lines(acc).items()}


# ---------------------------------------------------------------------------------------------------------------------------
# data (GPU side)
# ---------------------------------------------------------------------------------------------------------------------------
_NAN_BYTES = {BF: 0x7FC1, F32: 0x7FC00001}


class Arena:
    """One allocation per case: pattern everywhere, the buffers of the case as views into it."""

    def __init__(self, case: Case, dev):
        self.case = case
        self.off, self.size = layout(case)
        self.mem = torch.empty(self.size, dtype=torch.uint8, device=dev)
        self.mem.fill_(0xA5)
        self.base = self.mem.data_ptr()
        assert self.base % 256 == 0 or dev == "cpu", "the allocator's 256-byte alignment is what the CPU-side enumeration assumed"
        self.writable = torch.zeros(self.size, dtype=torch.bool, device=dev)
        for b in case.bufs:
            if b.role in ("out", "ws"):
                rows = b.rows - 1 if b.name == "slabs" else b.rows        # the slab beyond splitk_slabs must stay untouched
                self._bytes(b, self.writable, rows)[:, :b.cols * _ESIZE[b.dtype]] = True
            if b.role == "zero":
                self.view(b.name).zero_()
        self.snap = None
        self.res0 = None

    def _bytes(self, b: Buf, mem, rows=None):
        rows = b.rows if rows is None else rows
        es = _ESIZE[b.dtype]
        return mem[self.off[b.name]:self.off[b.name] + rows * b.ld * es].view(rows, b.ld * es)

    def full(self, name):
        """[rows][ld] view (padding columns included)"""
        b = self.case.buf(name)
        return self._bytes(b, self.mem).view(b.dtype)

    def view(self, name):
        """[rows][cols] view of the valid elements"""
        b = self.case.buf(name)
        return self.full(name)[:, :b.cols]

    def fill_outputs(self):
        for b in self.case.bufs:
            if b.role == "out":
                if b.name == "c" and self.case.recipe.res == "alias" and self.res0 is not None:
                    self.view("c").copy_(self.res0)             # the residual is read from c itself
                elif b.dtype == BF:
                    self.view(b.name).view(torch.int16).fill_(0x7FC1)
                else:
                    self.view(b.name).view(torch.int32).fill_(0x7FC00001)
            elif b.role == "ws":
                self.view(b.name).fill_(float("nan"))

    def freeze(self):
        self.snap = self.mem.clone()

    def untouched_outside_outputs(self) -> bool:
        keep = ~self.writable
        return bool(torch.equal(self.mem[keep], self.snap[keep]))

    def desc(self, tile=None):
        return make_desc(self.case, self.base, self.off, tile)


def _bf(t):
    return t.to(BF)


def _geglu_perm_rows(t, blk):
    """rows [values | gates] -> blocks of 2 blk rows [blk values | blk gates] (sliders_amd.weights._geglu_perm / _geglu_perm16)"""
    n = t.shape[0] // 2
    a, g = t[:n], t[n:]
    rest = t.shape[1:]
    return torch.stack([a.reshape(n // blk, blk, *rest), g.reshape(n // blk, blk, *rest)], 1).reshape(2 * n, *rest).contiguous()


def fill_inputs(ar: Arena, seed: int) -> dict:
    """Seeded bf16 / fp32 inputs written into the arena; returns the logical (unpermuted, unpacked) tensors the reference needs."""
    from sliders_amd.weights import pack_gemm_w
    case, r, d = ar.case, ar.case.recipe, ar.case.dims
    dev = ar.mem.device
    g = torch.Generator(device=dev).manual_seed(seed)
    M, N, K = d["M"], d["N"], d["K"]
    L = {}

    def rn(*shape, scale=1.0, shift=0.0):
        return torch.randn(*shape, device=dev, generator=g) * scale + shift

    ascale, ashift = (1.5, r.ln_off) if r.ln_in else (1.0, 0.0)
    for nm in ("a0", "a1"):
        if any(b.name == nm for b in case.bufs):
            b = case.buf(nm)
            x = _bf(rn(b.rows, b.cols, scale=ascale, shift=ashift))
            ar.full(nm)[:, b.col0:b.col0 + b.cols].copy_(x)
            L[nm] = x
    w = _bf(rn(N, K) / math.sqrt(K))
    if r.ln_in:
        # consumer side of the fold: w holds W * gamma (rounded), ln_s its row sums, ln_b = bias + W . beta (weights.fold_layernorm)
        gamma, beta = _bf(rn(K, scale=0.5, shift=1.0)), _bf(rn(K, scale=0.3))
        bias0 = _bf(rn(N))
        w = _bf(w.float() * gamma.float()[None, :])
        ln_s = w.float().sum(1)
        ln_b = (w.float() / gamma.float()[None, :]) @ beta.float() + bias0.float()
        L.update(ln_s=ln_s, ln_b=ln_b)
    L["w"] = w                                     # logical row order: [values | gates] for the GEGLU recipes
    wk = w
    if r.geglu in (1, 3):
        wk = _geglu_perm_rows(w, 32 if r.geglu == 1 else 16)
    if case.w_layout == 1:
        ar.view("w").copy_(pack_gemm_w(wk).view(1, -1))
    else:
        ar.view("w").copy_(wk)
    if r.ln_in:
        lns, lnb = L["ln_s"], L["ln_b"]
        if r.geglu in (1, 3):
            blk = 32 if r.geglu == 1 else 16
            lns, lnb = _geglu_perm_rows(lns, blk), _geglu_perm_rows(lnb, blk)
        ar.view("ln_s").copy_(lns.view(1, -1))
        ar.view("ln_b").copy_(lnb.view(1, -1))
        # the producer's chunk statistics of the rows: (mean, M2) per chunk, chunk-major [K / width][M][2], fp32
        xc = L["a0"].double().view(M, K // r.ln_in, r.ln_in)
        mean = xc.mean(-1)
        m2 = ((xc - mean[..., None]) ** 2).sum(-1)
        ch = torch.stack([mean, m2], -1).permute(1, 0, 2).contiguous().float()
        ar.view("ln_in").copy_(ch.view(-1, 2))
        L["chunks"] = ch
    if r.bias:
        bias = _bf(rn(N))
        L["bias"] = bias
        bk = _geglu_perm_rows(bias, 32 if r.geglu == 1 else 16) if r.geglu in (1, 3) else bias
        ar.view("bias").copy_(bk.view(1, -1))
    if r.res:
        res = _bf(rn(M, N))
        L["res"] = res
        if r.res == "sep":
            ar.view("res").copy_(res)
        else:
            ar.res0 = res
    if r.rowbias:
        b = case.buf("rowbias")
        rb = _bf(rn(b.rows, N))
        ar.full("rowbias")[:, b.col0:b.col0 + N].copy_(rb)
        L["rowbias"] = rb
    if r.lora:
        rank = r.rmajor or 4 * r.groups
        ar.view("scale").fill_(0.25)
        L["scale"] = 0.25
        up = _bf(rn(*((rank, N) if r.rmajor else (N, 4))))
        ar.view("up").copy_(up)
        L["up"] = up
        if r.lora == "ext":
            T = rn(M, rank)
            ar.view("T").copy_(T)
            L["T"] = T
        else:
            down = _bf(rn(rank, K) / math.sqrt(K))
            if r.ln_in:
                # adapter side of the fold (slh_lora_ln_fold): lora_down holds A . gamma (rounded), ln_lora_s its row sums, ln_lora_c = A . beta
                down = _bf(down.float() * gamma.float()[None, :])
                ls = down.float().sum(1)
                lc = (down.float() / gamma.float()[None, :]) @ beta.float()
                ar.view("ln_lora_s").copy_(ls.view(1, -1))
                ar.view("ln_lora_c").copy_(lc.view(1, -1))
                L.update(ln_lora_s=ls, ln_lora_c=lc)
            ar.view("down").copy_(down)
            L["down"] = down
    if r.geglu == 2:
        pre = _bf(rn(M, 2 * N))
        ar.view("pre").copy_(pre)
        L["pre"] = pre
    if r.xa:
        B, tk, H = M // d["xa_tq"], r.xa, N // 64
        b = case.buf("xa_k")
        kk = _bf(rn(B * tk, N))
        ar.full("xa_k")[:, b.col0:b.col0 + N].copy_(kk)
        vv = _bf(rn(B, tk, H, 64))
        vt = torch.zeros(B, H + 3, 64, 128, device=dev, dtype=BF)                # key columns >= tk zero
        vt[:, 2:2 + H, :, :tk] = vv.permute(0, 2, 3, 1)
        vt[:, :2] = _bf(rn(B, 2, 64, 128))                                       # other layers' heads around this layer's
        vt[:, 2 + H:] = _bf(rn(B, 1, 64, 128))
        ar.view("xa_vt").copy_(vt.view(-1, 128))
        L.update(xa_k=kk.view(B, tk, H, 64), xa_v=vv)
    return L


# ---------------------------------------------------------------------------------------------------------------------------
# references (float64, on the inputs' device)
# ---------------------------------------------------------------------------------------------------------------------------
def _a_full(case: Case, L: dict):
    """The A operand as a dense float64 [M][K] matrix (two sources concatenated; mode 1: the gathered 3 x 3 patches, K index =
    tap * Cin + c, through F.unfold of the transformed image)"""
    r, d = case.recipe, case.dims
    srcs = [L["a0"].double()] + ([L["a1"].double()] if "a1" in L else [])
    x = torch.cat(srcs, 1)
    if not r.conv:
        return x
    stride, xf = r.conv
    B, hs, ws, cin = d["batch"], d["hs"], d["ws"], d["cin"]
    img = x.view(B, hs, ws, cin).permute(0, 3, 1, 2)
    if xf == 1:
        img = F.interpolate(img, scale_factor=2.0, mode="nearest")
    elif xf == 2:
        z = torch.zeros(B, cin, 2 * hs, 2 * ws, dtype=img.dtype, device=img.device)
        z[:, :, ::2, ::2] = img
        img = z
    cols = F.unfold(img, 3, padding=1, stride=stride)                    # [B][cin * 9][L], row index c * 9 + tap
    Lo = cols.shape[-1]
    assert Lo == d["ho"] * d["wo"], (Lo, d)
    return cols.view(B, cin, 9, Lo).permute(0, 3, 2, 1).reshape(B * Lo, 9 * cin)


def _rnd(x64):
    """bf16 round-to-nearest-even of a float64 tensor, back in float64 (through fp32: exact for every value an fp32 kernel holds)"""
    return x64.float().to(BF).double()


def _flip(x64, e):
    """How far bf16(x') can be from bf16(x) for any |x' - x| <= e: rounding is monotonic, so the two ends of the interval decide."""
    c = _rnd(x64)
    return torch.maximum((_rnd(x64 + e) - c).abs(), (_rnd(x64 - e) - c).abs())


_GELU_FAST_ABS = 4.4e-6      # csrc/common.h, gelu_erf_fast_f: within 4.4e-6 of the float64 x Phi(x) for |x| < 6, fp32-exact beyond
_GELU_LIP = 1.13             # max |d/dx x Phi(x)| = 1.129


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def _geglu_forward(val, e_acc):
    """geglu = 1 / 3.  The kernel computes, per output column j with value column a and gate column g of proj = val:
        out = bf16( bf16(a) * bf16(gelu(bf16(g))) )
    (header: proj(x) is rounded to bf16 - it is what geglu_pre receives - before the gate; the gelu output is a bf16 tensor as in
    the reference).  The reference restates the three inner roundings on the float64 val.  Bound, with e the accumulate error of
    val (n 2^-24 S): the kernel's bf16(a) differs from the reference's by at most fa = flip(a, e_a) (monotone rounding: zero
    unless a lies within e of a rounding boundary); its gelu argument by fg = flip(g, e_g), so its gelu VALUE by at most
    1.13 fg + 4.4e-6 (Lipschitz constant of x Phi(x); stated accuracy of the kernel's erfc fit), which the rounding to bf16 turns
    into fh = flip(gelu(g_ref), 1.13 fg + 4.4e-6).  Then
        |a' h' - a h| <= fa |h| + |a| fh + fa fh,   one fp32 product rounding (2^-24 |a h|), and the output rounding 2^-8 |ref|."""
    n2 = val.shape[1] // 2
    va, vg = val[:, :n2], val[:, n2:]
    ea, eg = e_acc[:, :n2], e_acc[:, n2:]
    a, gq = _rnd(va), _rnd(vg)
    h_exact = _gelu(gq)
    h = _rnd(h_exact)
    fa, fg = _flip(va, ea), _flip(vg, eg)
    fh = _flip(h_exact, _GELU_LIP * fg + _GELU_FAST_ABS)
    ref = a * h
    bound = BF16_RND * ref.abs() + fa * h.abs() + a.abs() * fh + fa * fh + 2 * FP32_EPS * ref.abs()
    return ref, bound


def _geglu_backward(val, e_acc, pre):
    """geglu = 2 (csrc/gemm_common.h, the GEGLU_BWD arithmetic of slh_elementwise): with dd = bf16(val), h / g the value / gate halves of
    the forward's bf16 pre-activation,
        d_h = bf16( dd * bf16(g Phi(g)) ),   d_g = bf16( bf16(dd * h) * (Phi(g) + g phi(g)) )
    leaving in proj's blocked column order (64-column blocks [32 d_h | 32 d_g]).  fd = flip(val, e) bounds the kernel's dd against
    the reference's.  g Phi(g) is evaluated in fp32 by the kernel (erff form: a few fp32 roundings, 8 2^-24 (|g| + 1) allowed), so its
    bf16 may flip: fq = flip(g Phi(g), that).  dd * h is exact in fp32 (two bf16 factors), so bf16(dd h) moves by at most
    fp = flip(dd h, fd |h|); the derivative factor D = Phi + g phi (|D| <= 1.13) carries 8 2^-24 of fp32 evaluation error.
        |d_h' - d_h| <= fd |q| + |dd| fq + fd fq + 2^-24 |d_h| + 2^-8 |d_h|
        |d_g' - d_g| <= fp |D| + |bf16(dd h)| 8 2^-24 (|D| + 1) + 2^-8 |d_g|"""
    N = val.shape[1]
    M = val.shape[0]
    pb = pre.double().view(M, N // 32, 2, 32)                       # proj's blocked column order: 64-column blocks [32 h | 32 g]
    h, g = pb[:, :, 0].reshape(M, N), pb[:, :, 1].reshape(M, N)
    dd = _rnd(val)
    fd = _flip(val, e_acc)
    cdf = 0.5 * (1.0 + torch.erf(g * 0.7071067811865476))
    pdf = torch.exp(-0.5 * g * g) * 0.3989422804014327
    q_exact = g * cdf
    q = _rnd(q_exact)
    fq = _flip(q_exact, 8 * FP32_EPS * (g.abs() + 1.0))
    dh = dd * q
    b_dh = fd * q.abs() + dd.abs() * fq + fd * fq + FP32_EPS * dh.abs() + BF16_RND * dh.abs()
    ph_exact = dd * h
    ph = _rnd(ph_exact)
    fp = _flip(ph_exact, fd * h.abs())
    D = cdf + g * pdf
    dg = ph * D
    b_dg = fp * D.abs() + (ph.abs() + fp) * 8 * FP32_EPS * (D.abs() + 1.0) + BF16_RND * dg.abs()
    blocked = lambda x, y: torch.stack([x.reshape(M, N // 32, 32), y.reshape(M, N // 32, 32)], 2).reshape(M, 2 * N)
    return blocked(dh, dg), blocked(b_dh, b_dg)


def _cross_attention(case, L, val, e_acc):
    """xa_k: Q = bf16(val) (header: Q rounded to bf16), then per (sample, head) o = sum_j w_j v_j, w = softmax(Q K^T scale) over the xa_tk
    keys.  The kernel (csrc/gemm_common.h) takes raw scores r_j = Q . K_j as 64-term fp32 MFMA sums, p_j = exp2(fma(r_j, c, -r_max c)) with
    c = scale log2(e), rounds p_j to bf16 for the P.V MFMA, sums the UNROUNDED p_j for the denominator and multiplies by its reciprocal.
    Error of the exponent, in natural-log units, against the reference's s_j - s_max (s = r scale):
      (i)   Q: the kernel's bf16 Q differs from the reference's by at most fq = flip(val, e)       -> scale sum_d fq_d |K_jd|
      (ii)  the 64-term fp32 sum r_j (64 roundings) and the products' exactness                      -> scale 64 2^-24 sum_d |Q_d||K_jd|
            (66 is used: two more roundings for c = scale * log2 e and its product)
      (iii) the exponent fma(r_j, c, -r_max c): c carries one rounding (2^-24 |s_j - s_max|), r_max c is a rounded product
            (2^-24 |s_max|), the fma rounds once (2^-24 |s_j - s_max|); with |s_j - s_max| <= |s_j| + |s_max| that is at most
            3 2^-24 (|s_j| + |s_max|).  v_exp_f32 is accurate to 1 ulp: a relative 2^-23 of p_j, i.e. 2^-23 in the exponent.
            Allowed here: 2^-21 (|s_j| + |s_max|) + 2^-23  (8 roundings instead of the 3 counted: the masking and max steps are exact)
      D = the row maximum over j of (i) + (ii) + (iii).
    Every unnormalised p_j is then off by a factor within e^{+-D}, so is their sum, so every w_j by a factor within e^{+-2D}:
        |do| <= (e^{2D} - 1) A,   A = sum_j w_j |v_j|
    bf16 rounding of p_j ahead of P.V: 2^-8 e^{2D} A.  fp32 arithmetic behind it: the P.V MFMA sums 96 terms (96 2^-24 A); the denominator
    is a 96-term sum of positive p_j (relative 96 2^-24, and it scales o with |o| <= A: 96 2^-24 A); the reciprocal and the final product
    round once each (2 2^-24 A) - 194 2^-24 A in all, 200 used.  Output rounding: 2^-8 |ref|."""
    d = case.dims
    M, N = val.shape
    Tq, tk = d["xa_tq"], case.recipe.xa
    B, H = M // Tq, N // 64
    scale = case.fields["xa_scale"]
    q = _rnd(val).view(B, Tq, H, 64).permute(0, 2, 1, 3)
    fq = _flip(val, e_acc).view(B, Tq, H, 64).permute(0, 2, 1, 3)
    k = L["xa_k"].double().permute(0, 2, 1, 3)                     # [B][H][tk][64]
    v = L["xa_v"].double().permute(0, 2, 1, 3)
    s = q @ k.transpose(-1, -2) * scale
    ds = scale * (fq @ k.abs().transpose(-1, -2) + 66 * FP32_EPS * (q.abs() @ k.abs().transpose(-1, -2)))
    ds = ds + 2.0 ** -21 * (s.abs() + s.abs().amax(-1, keepdim=True)) + 2.0 ** -23
    D = ds.amax(-1, keepdim=True)
    w = torch.softmax(s, -1)
    ref = w @ v
    A = w @ v.abs()
    bound = BF16_RND * ref.abs() + (torch.expm1(2 * D) + BF16_RND * torch.exp(2 * D) + 200 * FP32_EPS) * A
    back = lambda t: t.permute(0, 2, 1, 3).reshape(M, N)
    return back(ref), back(bound)


def reference(case: Case, L: dict) -> List[Tuple[str, torch.Tensor, torch.Tensor, bool]]:
    """[(output buffer, float64 reference, float64 bound, take the rounding statistic)] for every output of the case.  Linear recipes:
    val = A W^T (+ LayerNorm fold) + bias + row bias + adapter + residual, S the same on absolute values, n = K + the epilogue's
    addends; the fused forward adapter rounds scale * T to bf16 ahead of its MFMA (R = 2^-8 |scale T| |B|^T; the reference keeps T
    unrounded), and its T carries its own accumulate error K 2^-24 |A||A_d|^T into the product."""
    r, d = case.recipe, case.dims
    M, N, K = d["M"], d["N"], d["K"]
    A = _a_full(case, L)
    W = L["w"].double()
    val = A @ W.t()
    Aabs = A.abs()
    sabs = Aabs @ W.abs().t()
    n = K
    extra = torch.zeros_like(val)
    outs = []
    mean = rstd = None
    if r.ln_in:
        # the rows' mean / rstd merged from the chunk statistics (all chunks the same width: the mean of means, M2 by Chan's update)
        ch = L["chunks"].double()                            # [chunks][M][2]
        cw = r.ln_in
        mean = ch[..., 0].mean(0)
        m2 = ch[..., 1].sum(0) + cw * ((ch[..., 0] - mean[None]) ** 2).sum(0)
        rstd = 1.0 / torch.sqrt(m2 / K + case.fields["ln_eps"])
        s, b = L["ln_s"].double(), L["ln_b"].double()
        val = rstd[:, None] * (val - mean[:, None] * s[None]) + b[None]
        # the merge itself costs a few fp32 roundings of mean and rstd: 2 chunks + 4 more terms
        sabs = rstd[:, None] * (sabs + mean.abs()[:, None] * s.abs()[None]) + b.abs()[None]
        n += 2 * (K // cw) + 4
        # fp32 merge of the chunks: the mean is a sum of K / cw chunk means (S = mean |mean_c|); the variance a sum of positive terms
        # whose (mean_c - mean) factors cancel: d var <= n 2^-24 (var + 2 |mean| sigma), so d rstd = rstd^3 d var / 2
        # <= n 2^-24 rstd (1 + |mean| rstd)   (var rstd^2 <= 1, sigma rstd <= 1)
        nmr = 2 * (K // cw) + 8
        mr_s = torch.stack([ch[..., 0].abs().mean(0), rstd * (1.0 + mean.abs() * rstd)], -1)
        e_rstd = nmr * FP32_EPS * mr_s[:, 1]
        extra = extra + e_rstd[:, None] * (sabs - b.abs()[None]) / rstd[:, None]
        if r.mr_out:
            mr_ref = torch.stack([mean, rstd], -1)
            outs.append(("mr", mr_ref, elementwise_bound(mr_ref, mr_s, nmr, rel=0.0), False))
    if r.bias:
        b = L["bias"].double()
        val, sabs, n = val + b[None], sabs + b.abs()[None], n + 1
    if r.rowbias:
        rps = case.fields["rows_per_sample"]
        rb = L["rowbias"].double()[torch.arange(M, device=val.device) // rps]
        val, sabs, n = val + rb, sabs + rb.abs(), n + 1
    if r.lora:
        sc = L["scale"]
        rank = r.rmajor or 4 * r.groups
        if r.lora == "ext":
            T, Tabs, eT = L["T"].double(), L["T"].double().abs(), None
        else:
            Dn = L["down"].double()
            T, Tabs = A @ Dn.t(), Aabs @ Dn.abs().t()
            nT = K
            if r.ln_in:
                ls, lc = L["ln_lora_s"].double(), L["ln_lora_c"].double()
                T = rstd[:, None] * (T - mean[:, None] * ls[None]) + lc[None]
                Tabs = rstd[:, None] * (Tabs + mean.abs()[:, None] * ls.abs()[None]) + lc.abs()[None]
                nT += 2 * (K // r.ln_in) + 4
            eT = nT * FP32_EPS * Tabs
            if r.t_out:
                outs.append(("t_out", T, elementwise_bound(T, Tabs, nT, rel=0.0), False))
        up = L["up"].double()
        if r.rmajor:
            term, tabs = sc * T @ up, sc * Tabs @ up.abs()
            eterm = None if eT is None else sc * eT @ up.abs()
        else:
            ng = N // r.groups
            term, tabs, eterm = torch.zeros_like(val), torch.zeros_like(val), torch.zeros_like(val)
            for g in range(r.groups):
                cs, ts = slice(g * ng, (g + 1) * ng), slice(4 * g, 4 * g + 4)
                term[:, cs] = sc * T[:, ts] @ up[cs].t()
                tabs[:, cs] = sc * Tabs[:, ts] @ up[cs].abs().t()
                if eT is not None:
                    eterm[:, cs] = sc * eT[:, ts] @ up[cs].abs().t()
            if eT is None:
                eterm = None
        val, sabs, n = val + term, sabs + tabs, n + rank + 1
        if eterm is not None:
            extra = extra + eterm
        if r.lora == "fused" and not r.rmajor:
            extra = extra + BF16_RND * tabs                  # R: scale * T rounded to bf16 ahead of the up-projection MFMA
    if r.res:
        rs = L["res"].double()
        val, sabs, n = val + rs, sabs + rs.abs(), n + 1
    e_acc = n * FP32_EPS * sabs + extra
    if r.xa:
        ref, bound = _cross_attention(case, L, val, e_acc)
        outs.append(("c", ref, bound, True))
        return outs
    if r.geglu in (1, 3):
        ref, bound = _geglu_forward(val, e_acc)
        outs.append(("c", ref, bound, True))
        if r.pre:
            # geglu_pre: proj(x) in THIS product's column order (the permuted weights' order), an ordinary bf16 output
            blk = 32
            perm = lambda x: _geglu_perm_rows(x.t().contiguous(), blk).t().contiguous()
            outs.append(("pre", perm(val), perm(BF16_RND * val.abs() + e_acc), True))
        return outs
    if r.geglu == 2:
        ref, bound = _geglu_backward(val, e_acc, L["pre"])
        outs.append(("c", ref, bound, True))
        return outs
    bound = BF16_RND * val.abs() + e_acc
    if r.vt:
        C, B, T = d["vt_C"], d["vt_B"], d["vt_T"]
        tr = lambda x: x[:, 2 * C:].reshape(B, T, C // 64, 64).permute(0, 2, 3, 1).reshape(-1, T)
        outs.append(("vt", tr(val), tr(bound), True))
        outs.append(("c", val, bound, True))                 # (the caller masks the V columns of c when vt_also_c is off)
    else:
        outs.append(("c", val, bound, True))
    return outs


def ln_out_reference(case: Case, c_stored: torch.Tensor):
    """(mean, M2) of every chunk of every row of the STORED bf16 result, float64, chunk-major [N / width][M][2], with the accumulate
    bound of an fp32 evaluation shifted by a pivot k inside the chunk (sums of x - k and (x - k)^2, |x - k| <= spread = max - min):
    mean = k + sum / width within n 2^-24 (spread + |mean|); M2 = sq - sum^2 / width, both at most width spread^2, within
    n 2^-24 width spread^2; n = 2 width + 8 (the two sums and the merges across lanes)."""
    cw = case.dims["ln_cw"]
    M, N = c_stored.shape
    x = c_stored.double().view(M, N // cw, cw)
    mean = x.mean(-1)
    dev = x - mean[..., None]
    m2 = (dev ** 2).sum(-1)
    ref = torch.stack([mean, m2], -1).permute(1, 0, 2).reshape(-1, 2)
    # the kernel accumulates values shifted by a row-local pivot k (one stored element of the chunk): sums of (x - k) and (x - k)^2
    spread = (x.amax(-1) - x.amin(-1))
    s_mean = spread + mean.abs()
    s_m2 = cw * spread ** 2
    sab = torch.stack([s_mean, s_m2], -1).permute(1, 0, 2).reshape(-1, 2)
    return ref, elementwise_bound(ref, sab, 2 * cw + 8, rel=0.0)


def _main(argv):
    acc, ref = enumerate_cases()
    table = capability_table(acc)
    print(f"{len(acc)} accepted, {len(ref)} refused, {len(table)} table rows")
    if "--write" in argv:
        os.makedirs(os.path.dirname(DATA), exist_ok=True)
        with open(DATA, "w") as fh:
            fh.write('{"accepted": %d,\n"table": {\n' % len(acc))            # one row per line: a change of the rule reads as a diff
            fh.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in table.items()))
            fh.write("\n}}\n")
        print(f"wrote {DATA} ({os.path.getsize(DATA)} bytes)")
    if "--write-dispatch" in argv:
        dig = dispatch_digests(acc)
        with open(DISPATCH, "w") as fh:                                        # one key per line
            fh.write("{\n" + ",\n".join('%s: {\n%s\n}' % (json.dumps(sec), ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in rows.items()))
                                        for sec, rows in dig.items()) + "\n}\n")
        print(f"wrote {DISPATCH} ({os.path.getsize(DISPATCH)} bytes)")
    if "--dispatch" in argv:              # the launches behind one digest: --dispatch 'bare|a|wl1|S0' or --dispatch 'sdxl|64|noxattn|on'
        key = argv[argv.index("--dispatch") + 1]
        rows = dispatch_lines(acc)
        found = [ln for sec in rows.values() for ln in sec.get(key, [])]
        print("\n".join(found) if found else f"no such key: {key}")


if __name__ == "__main__":
    _main(sys.argv[1:])
