"""Tile choice for slh_gemm: the measured table (written by scripts/tune_gemm.py on an MI355X) and choose_tile, which gives every
GEMM the planner records its tile.

The C library has a fill-the-chip heuristic; the planner overrides it with the measured best tile for every (shape, addressing mode)
it has an entry for.  Tables live in sliders_amd/tuning/*.json and are merged.  What a tile can run is the library's rule
(slh_gemm_tile_ok); what the planner wants of it - table entries, untuned defaults, optional epilogue extras - is decided here.
"""
from __future__ import annotations

import glob
import json
import os
from typing import Dict, NamedTuple, Optional

from . import lib

_TABLE: Optional[Dict[str, int]] = None

TILE_RING = 0x4412        # the 128 x 128 8-wave ring tile: the fused cross-attention's, and the tile the 64 x 160 / four-wave entries replaced

SPLITK_MAX_MN = 6 << 20          # output elements up to which split-K is considered (one 24 MB fp32 slab per slice at most)
SPLITK_MIN_K = int(os.environ.get("SLIDERS_SPLITK_MIN_K", "2048"))
SPLITK_TUNING_SLABS = 8          # slabs provisioned per candidate when the in-situ tuner may try any split factor


class TileFields(NamedTuple):
    splitk: int        # bits 16-19: split-K factor (0 | 1: none)
    family: int        # bits 12-15: 0 (4-wave ring; the alias 2 reads as 0), 4 (8-wave ring), 8 (ping-pong), 5 (64 x 160), 7 (gemm7.hip)
    slots: int         # bits 8-11: ring slots
    mi: int            # bits 4-7: MI (gemm7.hip: XB)
    ni: int            # bits 0-3: NI (gemm7.hip: WB)
    bm: int            # block tile rows, columns; 0 x 0 for an all-zero code (the library's heuristic picks)
    bn: int


def tile_fields(tile: int) -> TileFields:
    """A tile code (slh_gemm_desc.tile) taken apart - the only place in Python that reads its bits; which codes name a kernel is the
    library's knowledge (slh_gemm_tile_ok)."""
    s, fam, st, mi, ni = (tile >> 16) & 15, (tile >> 12) & 15, (tile >> 8) & 15, (tile >> 4) & 15, tile & 15
    fam = 0 if fam == 2 else fam
    if not tile & 0xFFFF:
        bm, bn = 0, 0
    elif fam == 5:
        bm, bn = 64, 160
    elif fam == 7:
        bm, bn = 32 * mi, 32 * ni
    elif fam == 8:
        bm, bn = (256, 256) if mi == 4 else (128, 64 * ni)
    else:
        bm, bn = (128 if fam == 4 else 64) * mi, 64 * ni
    return TileFields(s, fam, st, mi, ni, bm, bn)


def gemm_key(d, with_lora: bool = False) -> str:
    k = f"{d.M},{d.N},{d.K},m{d.mode},s{d.stride},x{d.src_xform},g{d.geglu}"
    if with_lora:     # the fused adapter changes the LDS footprint and the MFMA count per k-step: tuned separately
        k += f",l{1 if d.lora_down else 0}"
        # folded LayerNorm: the producer side needs a 128-column tile, the consumer side carries a prologue - both tuned
        # apart from the plain product of the same shape
        if getattr(d, "ln_out", None):
            k += ",no"
        if getattr(d, "ln_in", None):
            k += ",ni"
    return k


def tile_ok(d, tile: int) -> bool:
    """Can slh_gemm run descriptor d with this tile code?  The library's own rule (slh_gemm_tile_ok), asked with d.tile = tile: used
    by the tuner to skip candidates and by choose_tile."""
    q = type(d).from_buffer_copy(d)
    q.tile = tile
    return lib.gemm_tile_ok(q)


def splitk_tuning() -> bool:
    """Tuning mode (SLIDERS_NO_TUNING: scripts/tune_insitu.py tries split-K tiles on every candidate) or SLIDERS_SPLITK_ALL"""
    return bool(os.environ.get("SLIDERS_NO_TUNING") or os.environ.get("SLIDERS_SPLITK_ALL"))


def splitk_candidate(d) -> bool:
    """Few output tiles and a long reduction (the 1280-channel convolutions at 8x8 / 16x16 of SD-1.x and of SDXL at
    512x512: 10-40 tiles for 256 CUs, 29 MB of weights each): such a product gets a zeroed fp32 workspace so that
    slh_gemm may cut K into slices (tile bits 16-19, chosen by the tuner or by default_splitk below)."""
    return d.M * d.N <= SPLITK_MAX_MN and d.K >= SPLITK_MIN_K and not d.geglu and d.N % 4 == 0


def splitk_wanted(d) -> bool:
    """The tile that will run splits K: the tuned tile says so, or there is no tuned tile and the default would; in tuning mode
    every candidate."""
    if not splitk_candidate(d):
        return False
    if splitk_tuning():
        return True
    return tile_fields(d.tile).splitk > 1 if d.tile else bool(default_splitk(d))


def default_splitk(d) -> int:
    """Untuned shape: slices so that tiles x slices is about one workgroup per CU, at least 8 K tiles per slice."""
    tiles = ((d.M + 127) // 128) * ((d.N + 63) // 64)
    if tiles >= 128 or d.K < 4096:
        return 0
    s = min(8, max(1, 256 // tiles), d.K // 512)
    return 0 if s < 2 else (s << 16) | 0x412


def splitk_slabs(d) -> int:
    """Slabs of split-K workspace for d with its chosen tile (0: none): one per K slice, SPLITK_TUNING_SLABS in tuning mode."""
    if not splitk_wanted(d):
        return 0
    slabs = max(SPLITK_TUNING_SLABS if splitk_tuning() else 0, tile_fields(d.tile).splitk)
    return slabs if slabs >= 2 else 0


def table() -> Dict[str, int]:
    global _TABLE
    if _TABLE is None:
        _TABLE = {}
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuning")
        paths = sorted(glob.glob(os.path.join(here, "*.json")))
        if os.environ.get("SLIDERS_TUNING_OVERRIDE"):          # same-box A/B of table variants: entries of this file win
            paths.append(os.environ["SLIDERS_TUNING_OVERRIDE"])
        for path in paths:
            with open(path) as f:
                _TABLE.update({k: int(v) for k, v in json.load(f).items()})
    return _TABLE


def _fits(d, tile: int) -> bool:
    """tile_ok and a policy: a folded LayerNorm runs without split-K (the ring tiles could: the last slice normalises the sums)"""
    return tile_ok(d, tile) and not (d.ln_in and tile_fields(tile).splitk > 1)


def tuned_tile(d) -> int:
    """The measured tile for d as it stands (0: no entry, the library heuristic)."""
    if os.environ.get("SLIDERS_NO_TUNING"):
        return 0
    tb = table()
    # (the GEGLU backward form, geglu = 2, is looked up as the plain backward-data product it extends)
    full, plain = (k.replace(",g2", ",g0") for k in (gemm_key(d, True), gemm_key(d)))
    base = full.replace(",no", "").replace(",ni", "")          # entries measured before the LayerNorm folding existed
    t = tb.get(full, tb.get(base, tb.get(plain, 0)))
    if not t and d.geglu == 3:     # GEGLU in 16 | 16 blocks takes any tile: unmeasured shapes run the tile measured for the 32 | 32 form
        g1 = lambda k: k.replace(",g3", ",g1")
        t = tb.get(g1(full), tb.get(g1(base), tb.get(g1(plain), 0)))
    if not t and d.lora_down:      # adapter fused in but only the plain product was measured (backward-data GEMMs): same tile
        t = tb.get(base[:-1] + "0", 0)
    if t and not _fits(d, t):
        # an entry names a shape, not a feature set (the key does not see row bias, adapters, training outputs): a 64 x 160 or
        # four-wave entry gives way to the ring tile it replaced, any other to the library's heuristic
        t = TILE_RING if tile_fields(t).family in (5, 7) and tile_ok(d, TILE_RING) else 0
    force = os.environ.get("SLIDERS_FORCE_STAGES")     # experiment knob: 2 or 3 for every non-128x128 tile
    if force and t and tile_fields(t)[3:5] != (2, 2):
        t = (t & 0xFF) | (int(force) << 8 if force == "3" else 0)
    return t


def _put(d, fields: dict):
    for k, v in fields.items():
        setattr(d, k, v)


def choose_tile(d, ln_out: bool = False, vt: Optional[dict] = None, xa: Optional[dict] = None,
                backward: bool = False) -> Optional[int]:
    """Set d.tile for a GEMM about to be recorded - d carries every feature the launch needs; nothing changes d.tile afterwards - and
    attach the optional extras that tile takes, with placeholder pointers the caller replaces once it has allocated their buffers:
      ln_out   chunk statistics of the result for a LayerNorm folded into the next product (ln_out = 8)
      vt       the vt_* fields of a head-transposed V^T / dO^T store (vt_out = 16)
      xa       the xa_* fields of the cross-attention fused behind a query projection (real pointers)
    backward: a backward-data product (untuned, it keeps the library's heuristic where a forward product would take 0x12).
    Returns the width of the statistics' chunks (0: no ln_out), or None when the LayerNorm d folds (ln_in) cannot run on the tile it
    gets - the caller then records the LayerNorm launch and the plain product."""
    if ln_out:
        d.ln_out = 8               # the producer side has table entries of its own (",no"), and the entry must take the statistics
    t = tuned_tile(d)
    d.ln_out = 0
    if not t and not backward and d.M <= 192 and d.N >= 4096:
        t = 0x12                   # few rows, very wide: 64-row tiles waste the least of the short M
    if xa is not None and (t == TILE_RING or os.environ.get("SLIDERS_XATTN_ALL")):
        # (where the table prefers another tile for the query projection - the 640-channel level - the two launches stay)
        _put(d, xa)
        if tile_ok(d, TILE_RING):
            t = TILE_RING
        else:
            _put(d, dict.fromkeys(xa, 0))
    d.tile = t
    if d.ln_in:
        if (not t and splitk_wanted(d)) or not _fits(d, t):
            return None            # (a product the untuned default would split keeps its LayerNorm launch)
    elif not t and splitk_wanted(d) and d.M * d.N <= (1 << 20):
        d.tile = default_splitk(d)         # the untuned default only for the small products it was measured on
    if ln_out and not splitk_slabs(d):     # (no statistics from a product with split-K slabs)
        d.ln_out = 8
        if not lib.gemm_ln_chunk_cols(d):
            d.ln_out = 0
    if vt is not None and not tile_fields(d.tile).splitk:
        _put(d, dict(vt, vt_out=16))
        if not lib.gemm_tile_ok(d):
            # V^T policy: a 64 x 160 or four-wave entry gives way to the ring tile it replaced (its entry names a shape, not a
            # feature set); any other tile is kept and the store dropped
            if tile_fields(d.tile).family in (5, 7) and tile_ok(d, TILE_RING):
                d.tile = TILE_RING
            else:
                _put(d, dict.fromkeys(list(vt) + ["vt_out"], 0))
    return lib.gemm_ln_chunk_cols(d) if d.ln_out else 0
