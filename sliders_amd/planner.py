"""Static planner: turns one UNet2DConditionModel forward (and, for the training pass, its backward through
the frozen net into the LoRA adapters) into a flat command buffer for libsliders_hip.so.

Op order follows diffusers-0.20.2 UNet2DConditionModel.forward as called by the reference at
trainscripts/textsliders/train_util.py:159-163 / 242-247, re-expressed on pixel-major
activations [B*H*W][C]:
  * every Linear / 1x1 conv / 3x3 conv is slh_gemm (implicit GEMM for 3x3, channel concat and nearest-2x
    upsample folded into the A-operand addressing),
  * the LoRA branch of lora.py:108-112 is slh_skinny (down) + a rank-4 epilogue term (up) - skipped entirely
    when the adapters are switched off (multiplier 0 adds an exact 0 in the reference),
  * q/k/v (and cross k/v) projections are fused into one GEMM, all time_emb_proj layers into one GEMV.
Modes: "off" (LoRA disabled), "on" (LoRA enabled, no grad), "train" (LoRA enabled, activations kept, GEGLU
unfused so its pre-activation is available; the pass leaves a tape of typed records, from which backward.BackwardPlan
emits the backward program).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field, fields
from typing import Dict, List, Optional, Tuple, Union

import torch

from . import lib
from .arena import Arena, Buf
from .config import UNetConfig
from .lora_store import LoraEntry, LoraStore
from .tuning import TILE_RING, choose_tile, splitk_slabs, splitk_tuning, tile_fields
from .weights import WeightStore


@dataclass
class Act:
    """Pixel-major activation view: rows = B*H*W pixels, C channels, row stride ld (elements)."""
    ptr: int
    B: int
    H: int
    W: int
    C: int
    ld: int
    buf: Optional[Buf] = None
    name: str = ""
    ln: Optional[tuple] = None     # (Buf of per-row 64-column chunk statistics written by the producing GEMM, chunks): folded LayerNorm
    vt: Optional[tuple] = None     # q|k|v projection whose epilogue also stored V head-transposed: (pointer, 0) as attention()'s vt_pre
    attended: bool = False         # attn2.to_q whose epilogue ran the cross-attention: this IS the attention output

    @property
    def HW(self) -> int:
        return self.H * self.W

    @property
    def M(self) -> int:
        return self.B * self.H * self.W

    def cols(self, c0: int, c: int) -> "Act":
        return Act(self.ptr + 2 * c0, self.B, self.H, self.W, c, self.ld, self.buf, self.name + f"[:,{c0}:{c0 + c}]")

    def sample(self, b: int, nb: int = 1) -> "Act":
        return Act(self.ptr + 2 * b * self.HW * self.ld, nb, self.H, self.W, self.C, self.ld, self.buf,
                   self.name + f"[b{b}]")

    def tensor(self) -> torch.Tensor:
        """Debug view (real arenas only): [M][C] strided tensor."""
        base = self.buf.tensor.view(-1)
        off = (self.ptr - self.buf.ptr) // 2
        return base.as_strided((self.M, self.C), (self.ld, 1), off)


Src = Union[Act, Tuple[Act, Act]]

PH = 0x1000                      # placeholder for a pointer _emit fills in (aligned like every arena buffer: the tile rule looks)


def src_parts(x: Src):
    return x if isinstance(x, tuple) else (x, None)


def sources(x0: Act, x1: Optional[Act], p: str, ld: str, c: str) -> dict:
    """The two-source operand fields of a descriptor (a channel concat folded into the operand addressing), by field-name
    prefix: pointers p0 / p1, row strides ld0 / ld1, widths c0 / c1; all zero for a second source that is not there."""
    return {p + "0": x0.ptr, p + "1": x1.ptr if x1 else 0, ld + "0": x0.ld, ld + "1": x1.ld if x1 else 0,
            c + "0": x0.C, c + "1": x1.C if x1 else 0}


def head_t(D: int, T: int) -> Tuple[int, int]:
    """(Dp, ldt) of a head-transposed [B][heads][Dp][ldt] array: head dim and tokens rounded up to whole 64s"""
    return (D + 63) // 64 * 64, (T + 63) // 64 * 64


@dataclass(frozen=True)
class Conv3:
    """A product that is a 3x3 convolution (pad 1); None stands for a Linear / 1x1 convolution."""
    stride: int = 1
    xform: int = 0                 # 1: the source is read nearest-2x upsampled


def conv_fields(d, conv: Conv3, src: Act, Ho: int, Wo: int):
    """The implicit-GEMM fields of a descriptor (slh_gemm, slh_skinny, slh_lora_wgrad) that reads src as a 3x3 convolution does"""
    d.mode = 1
    d.batch, d.hs, d.ws = src.B, src.H, src.W
    d.src_xform, d.stride = conv.xform, conv.stride
    d.ho, d.wo = Ho, Wo


# The tape of a training forward: one record per differentiable step, in launch order, each with exactly what the backward reads
# (backward.BackwardPlan.HANDLERS has one handler per type).
@dataclass
class GemmRec:
    name: str
    x: Src
    wname: str
    N: int
    K: int
    Ho: int
    Wo: int
    conv: Optional[Conv3]
    grp: Optional[List[LoraEntry]]         # the adapter group
    residual: Optional[Act]
    temb_path: Optional[str]               # the resnet whose time_emb_proj row is this product's per-sample bias
    out: Optional[Act] = None              # the output and the adapter's T: what _emit allocates, set before the record is appended
    T: Optional[Buf] = None


@dataclass
class GnRec:
    name: str
    x: Src
    out: Act
    wname: str
    eps: float
    act: int
    stats: Buf


@dataclass
class LnRec:
    name: str
    x: Act
    out: Act
    wname: str
    mr: Buf


@dataclass
class AttnRec:
    name: str
    q: Act
    k: Act
    v: Act
    o: Act
    lse: Buf
    Tk: int
    heads: int


@dataclass
class GegluRec:
    name: str
    pre: Act
    out: Act


@dataclass
class ConvOutRec:
    x: Act


@dataclass
class Product:
    """One slh_gemm launch as UNetPlan._decide settled it.  d says the rest: d.vt_out - V^T / dO^T is stored, d.xa_k - the
    cross-attention rides in the epilogue, d.tile, d.ln_in."""
    d: "lib.GemmDesc"              # complete but for the pointers of what _emit allocates: output, T, statistics, V^T (placeholders)
    ln_cols: int                   # chunk width of the row statistics left for a folded LayerNorm (0: none)
    fused: bool                    # the adapter's down-projection runs inside the launch
    geglu_pre: Optional[Act]
    ln_norm: Optional[str]         # LayerNorm folded into the adapter's down-projection as well
    rec: GemmRec                   # its tape record (rec.x: the product's input)

    def behind_ln_record(self, stand_in: Act, mr: Buf):
        """Training LayerNorm fold: the tape keeps the LayerNorm as a record of its own, so this product's record reads the
        stand-in for the normalised tensor, and the launch leaves the rows' (mean, rstd) for the LayerNorm backward in mr."""
        self.d.ln_mr_out, self.rec.x = mr.ptr, stand_in


SPLITK_TICKETS = 4096            # 64-bit arrival tickets per plan (one per output tile of the largest split-K product)


def _sw(env: str, parse: str = "set"):
    return field(default=False, metadata=dict(env=env, parse=parse))


@dataclass(frozen=True)
class Switches:
    """Every environment switch of the planner: A/B knobs of closed experiments, all off by default.  Read once per forward plan
    (from_env, at the head of UNetPlan.__init__); the BackwardPlan of a plan uses the same copy.  parse: "set" = the variable exists
    (any value), "truthy" = it is non-empty, "zero" = it is exactly "0"."""
    no_weight_touch: bool = _sw("SLIDERS_NO_WEIGHT_TOUCH")   # no weight touch from idle workgroup slots: 24.35 / 24.32 ms a pass against 24.18 / 24.09
    no_attn_touch: bool = _sw("SLIDERS_NO_ATTN_TOUCH")   # the key-split self-attention carries no touch: 23.34 ms against 23.21 / 23.26
    touch_farthest: bool = _sw("SLIDERS_TOUCH_FARTHEST", "truthy")   # farthest carrier in the window first: 25.05 ms against 24.95 nearest-first
    lora_unfused: bool = _sw("SLIDERS_LORA_UNFUSED")   # the adapters' down-projection as a launch of its own ahead of every product
    train_no_ln_fold: bool = _sw("SLIDERS_TRAIN_NO_LN_FOLD")   # training passes keep every LayerNorm launch
    no_fused_vt: bool = _sw("SLIDERS_NO_FUSED_VT")   # V^T by a transpose launch instead of the q|k|v epilogue
    train_no_fused_vt: bool = _sw("SLIDERS_TRAIN_NO_FUSED_VT")   # the same for training passes only
    gn_split_slab: bool = _sw("SLIDERS_GN_ONE", "zero")   # =0: two launches for a GroupNorm over a cache-resident slab: 24.44 / 24.37 ms against 24.32 / 24.40
    gn_two_launch: bool = _sw("SLIDERS_GN_TWO_LAUNCH")   # two launches for every GroupNorm
    no_lora_ln_fold: bool = _sw("SLIDERS_NO_LORA_LN_FOLD")   # adapter-carrying q|k|v keeps its LayerNorm launch
    no_fused_xattn: bool = _sw("SLIDERS_NO_FUSED_XATTN")   # cross-attention as its own launch behind attn2.to_q
    train_unfused_geglu: bool = _sw("SLIDERS_TRAIN_UNFUSED_GEGLU")   # training forward: GEGLU as an elementwise launch behind ff.net.0.proj
    train_kv_per_block: bool = _sw("SLIDERS_TRAIN_KV_PER_BLOCK", "truthy")   # training forward: text K/V projected per block (the form of rounds 1-2)
    bwd_dot_launch: bool = _sw("SLIDERS_BWD_DOT_LAUNCH")   # dO^T of a self-attention by a transpose launch instead of the dgrad epilogue
    bwd_unfused_geglu: bool = _sw("SLIDERS_BWD_UNFUSED_GEGLU")   # GEGLU backward as an elementwise launch instead of ff.net.2's dgrad epilogue
    bwd_unbatched: bool = _sw("SLIDERS_BWD_UNBATCHED")   # one launch per head transpose and weight gradient instead of the batched ones
    wgrad_atomic: bool = _sw("SLIDERS_WGRAD_ATOMIC")   # weight gradients by fp32 atomics (not bit-reproducible) instead of slabs + tickets
    bwd_unfused_u: bool = _sw("SLIDERS_BWD_UNFUSED_U")   # U = dY . B as skinny launches instead of inside the dgrad product

    @classmethod
    def from_env(cls) -> "Switches":
        read = {"set": lambda v: v is not None, "truthy": bool, "zero": lambda v: v == "0"}
        return cls(**{f.name: read[f.metadata["parse"]](os.environ.get(f.metadata["env"])) for f in fields(cls)})


class Plan:
    """What the forward and the backward plan share: the arenas, the weights and the switches; the op list, serialised once; the
    split-K workspace; and the memset at the head of the program that zeroes the span of the zero arena the plan used."""

    def __init__(self, w, arena: Arena, zarena: Arena, sw: Switches):
        self.w, self.arena, self.zarena, self.sw = w, arena, zarena, sw
        self.ops: List[tuple] = []                # (opcode, descriptor, name) in launch order
        self._splitk_tickets = None
        self.zmark = zarena.mark()

    @property
    def w_layout(self) -> int:
        return 1 if self.w.packed else 0

    def add(self, opcode: int, desc, name: str):
        self.ops.append((opcode, desc, name))

    def _tickets(self, n: int) -> int:
        """The arrival tickets of a plan's split-K products: ONE array per plan - every launch leaves its tickets zero and the
        launches of a plan are ordered on one stream.  Lives in the zero-init arena (zeroed at the head of the program)."""
        assert n <= SPLITK_TICKETS, f"split-K product with {n} output tiles"
        if self._splitk_tickets is None:
            self._splitk_tickets = self.zarena.alloc((2 * SPLITK_TICKETS,), torch.float32, "splitk.tickets")
        return self._splitk_tickets.ptr

    def provision_splitk(self, d, name: str):
        """Give a product whose tile splits K (or, in tuning mode, may) its slab workspace: one fp32 slab (M, N rounded up to whole
        tiles) per K slice (each slice writes its own, the last slice of a tile to arrive adds them in slice order inside the launch
        - bit-reproducible) and, with a fused adapter, two [M][ld_t] slabs per slice for T."""
        slabs = splitk_slabs(d)
        if not slabs:
            return
        d.splitk_slabs = slabs
        d.splitk_c32 = self.arena.alloc((slabs, (d.M + 255) // 256 * 256, (d.N + 127) // 128 * 128), torch.float32, name + ".splitk").ptr
        d.splitk_ticket = self._tickets(((d.M + 63) // 64) * ((d.N + 63) // 64))
        if d.lora_down:
            # one pair of T slabs per slice and per COLUMN TILE (each column tile's last slice reduces its own copy); sized for
            # the narrowest tile (64 columns) unless the tile is fixed
            ni = tile_fields(d.tile).ni if (d.tile and not splitk_tuning()) else 1
            tiles_n = (d.N + 64 * ni - 1) // (64 * ni)
            d.splitk_t32 = self.arena.alloc((tiles_n * 2 * slabs, d.M, d.ld_t), torch.float32, name + ".splitk_T").ptr

    def put_head(self, zero_name: str, head: List[tuple]):
        """Close the op list: ahead of what was collected go the memset of the zero arena's span this plan allocated (fp32
        accumulators, arrival tickets) and then `head`, the plan's own launches that must precede everything."""
        self.zend = self.zarena.mark()
        zero = []
        if self.zend > self.zmark:
            p, n = self.zarena.region(self.zmark, self.zend)
            zero.append((lib.OP_MEMSET, lib.MemsetDesc(ptr=p, nbytes=n, value=0, pad=0), zero_name))
        self.ops = zero + head + self.ops

    def program(self, skip=()) -> "lib.Program":
        """The op list as a command buffer, without the ops named in skip"""
        prog = lib.Program()
        for o, d, nm in self.ops:
            if nm not in skip:
                prog.add(o, d, nm)
        return prog


PREFETCH_MIN_BYTES = int(os.environ.get("SLIDERS_PREFETCH_MIN", str(6 << 20)))
PREFETCH_MAX_BYTES = 96 << 20

TOUCH_WINDOW = 6      # ops a weight touch may ride ahead of the product that needs the weights


def attach_weight_touch(ops: List[tuple], sw: Switches):
    """The product path's weight prefetch (slh_gemm_desc.pf_*): every GEMM whose packed weights are 6-96 MB (GEGLU.proj 26 MB,
    ff.net.2 13 MB, q|k|v 10 MB at the 1280-channel level) has those bytes touched by the idle workgroup slots of an EARLIER
    launch that leaves >= 64 CUs free - the 160-tile products on the 128 x 128 ring tile (attention out-projections, attn2.to_q,
    ff.net.2 itself) - or, round 6, of the key-split self-attention launch (slh_attn_desc.pf_*: three workgroups per CU, 640 of 768
    slots taken) - the nearest such carrier within TOUCH_WINDOW ops that does not carry a touch yet.  No extra launch, no
    second stream.  ops = the (opcode, descriptor, name) list of a plan, before it is serialised: the carriers' pf_* are set in place."""
    if sw.no_weight_touch:
        return

    def carrier(o, d, _):
        if o == lib.OP_ATTN_FWD:          # round 6: the key-split self-attention of the 32 x 32 level (its workgroups leave a slot per CU)
            return not sw.no_attn_touch and lib.attn_carries_touch(d)
        if o != lib.OP_GEMM or d.mode != 0 or d.tile != TILE_RING:
            return False
        return ((d.M + 127) // 128) * ((d.N + 127) // 128) <= 192
    used = set()
    for i, (o, d, _) in enumerate(ops):
        if o != lib.OP_GEMM or d.w_layout != 1:
            continue
        nb = (d.N + 63) // 64 * 64 * d.K * 2
        if not (PREFETCH_MIN_BYTES <= nb <= PREFETCH_MAX_BYTES):
            continue
        cand = reversed(range(max(0, i - TOUCH_WINDOW), i))     # nearest first (measured: 24.95 ms against 25.05 farthest-first, 25.27 without)
        if sw.touch_farthest:
            cand = range(max(0, i - TOUCH_WINDOW), i)
        for j in cand:
            if j not in used and carrier(*ops[j]):
                ops[j][1].pf_ptr, ops[j][1].pf_bytes = d.w, nb
                used.add(j)
                break


@dataclass(frozen=True)
class AttnMapSpec:
    """Which cross-attention layers of a no-grad plan record a per-token attention map (slh_xattn_map): every attn2 whose query grid
    is the latent grid divided by a factor <= max_factor.  4 gives SDXL both of its attention levels, SD-1.x its 1x / 2x / 4x levels
    without the 8x level and the mid block."""
    max_factor: int = 4

    @classmethod
    def of(cls, spec) -> Optional["AttnMapSpec"]:
        """None, an AttnMapSpec, a dict of its fields or a bare max_factor"""
        if spec is None or isinstance(spec, cls):
            return spec
        s = cls(**spec) if isinstance(spec, dict) else cls(int(spec))
        if int(s.max_factor) != s.max_factor or s.max_factor < 1:
            raise ValueError(f"attn_maps: max_factor = {s.max_factor}: expected an integer >= 1")
        return s


class UNetPlan(Plan):
    def __init__(self, cfg: UNetConfig, weights: WeightStore, arena: Arena, zarena: Arena, B: int, H: int, W: int,
                 ctx_len: int = 77, lora: Optional[LoraStore] = None, mode: str = "off",
                 lora_scale_ptr: int = 0, io: Optional[dict] = None, attn_maps=None):
        assert mode in ("off", "on", "train")
        assert mode == "off" or lora is not None
        self.attn_maps = AttnMapSpec.of(attn_maps)
        if self.attn_maps is not None and mode == "train":
            raise ValueError("attn_maps: attention maps are collected in the no-grad plans (mode 'off' / 'on'), not in 'train'")
        self.map_ops: Dict[int, list] = {}        # factor -> the slh_xattn_map descriptors of that level, in plan order
        super().__init__(weights, arena, zarena, Switches.from_env())
        self.cfg = cfg
        self.B, self.H, self.W, self.ctx_len = B, H, W, ctx_len
        self.lora = lora if mode != "off" else None
        self.mode = mode
        self.train = mode == "train"
        self.lora_scale_ptr = lora_scale_ptr
        self.tape: list = []                      # GemmRec, GnRec ... of a training pass, in launch order
        self.lnfold_items: List[tuple] = []       # adapter sides of LayerNorm folds (slh_lora_lnfold_item as int64 words)
        self._build_io(io)
        self._forward()
        self._finish_maps()
        head = []
        if self.lnfold_items:
            self._lnfold_table = torch.tensor(self.lnfold_items, dtype=torch.int64, device=self.lora.params.device)
            head.append((lib.OP_LORA_LN_FOLD, lib.LoraLnFoldDesc(items=self._lnfold_table.data_ptr(), n=len(self.lnfold_items)),
                         "lora_ln_fold"))
        self.put_head("zero_stats", head)
        attach_weight_touch(self.ops, self.sw)
        self.prog = self.program()
        # The text K/V of every cross-attention block depend only on the prompt embeddings (and frozen weights): inside a
        # denoise loop (train_util.py:263-294: same embeddings for every timestep) steps 2.. replay the pass without
        # the batched K/V projection and its head transpose.  Valid only while no other plan ran in between (plans
        # share the arena) and io["ctx"] is unchanged - the caller's responsibility (trainer / sampler loops).
        self.prog_text_cached = None
        if self.kv_all is not None:
            skip = {"attn2_kv_all", "attn2_vt_all", "lora_ln_fold"}     # (the adapters do not change inside a denoise loop either)
            self.prog_text_cached = self.program(skip)

    # ------------------------------------------------------------------------------------------------
    # buffers
    # ------------------------------------------------------------------------------------------------
    def _build_io(self, io):
        cfg, B = self.cfg, self.B
        a = self.arena
        if io is not None:
            self.io = io
            self._build_map_io()
            return
        self.io = {
            "sample": a.alloc((B, cfg.in_channels, self.H, self.W), torch.bfloat16, "in.sample"),
            "t": a.alloc((B, 1), torch.float32, "in.t"),
            "ctx": a.alloc((B, self.ctx_len, cfg.cross_attention_dim), torch.bfloat16, "in.ctx"),
            "eps": a.alloc((B, cfg.out_channels, self.H, self.W), torch.bfloat16, "out.eps"),
        }
        if cfg.is_xl:
            self.io["time_ids"] = a.alloc((B, 6), torch.float32, "in.time_ids")
            self.io["add_in"] = a.alloc((B, cfg.projection_class_embeddings_input_dim), torch.bfloat16, "in.add_in")
        self._build_map_io()

    def _map_factor(self, h: Act) -> Optional[int]:
        """The level of a transformer block's tokens (latent grid / query grid) where this plan collects its map, else None"""
        if self.attn_maps is None or self.H % h.H or self.W % h.W or self.H // h.H != self.W // h.W:
            return None
        f = self.H // h.H
        return f if f <= self.attn_maps.max_factor else None

    def _build_map_io(self):
        """xattn_wt [B/2][ctx_len] and one xattn_map.<factor> [B/2][T_level] per collected level (fp32): the key weights the caller
        writes and the maps it reads, for the text half of the CFG pair"""
        if self.attn_maps is None:
            return
        cfg, B = self.cfg, self.B
        if B % 2:
            raise ValueError(f"attn_maps: B = {B}: the maps are those of the text half of a CFG pair (an even batch)")
        # the levels with a transformer: the attention down blocks (the up blocks mirror them) and the mid block, at the last level
        levels = {i for i, t in enumerate(cfg.down_block_types) if t != "DownBlock2D"} | {len(cfg.down_block_types) - 1}
        levels = sorted(i for i in levels if 2 ** i <= self.attn_maps.max_factor)
        if not levels:
            raise ValueError(f"attn_maps: no cross-attention level of this model has a factor <= {self.attn_maps.max_factor}")
        fmax = 2 ** max(levels)
        if self.H % fmax or self.W % fmax:
            raise ValueError(f"attn_maps: a {self.H} x {self.W} latent is not divisible by {fmax}, the coarsest collected level")
        self.io.setdefault("xattn_wt", self.arena.alloc((B // 2, self.ctx_len), torch.float32, "in.xattn_wt"))
        for i in levels:
            f = 2 ** i
            self.io.setdefault(f"xattn_map.{f}", self.arena.alloc((B // 2, (self.H // f) * (self.W // f)), torch.float32, f"out.xattn_map.{f}"))

    def _record_map(self, q: Act, k: Act, heads: int, factor: int, name: str):
        """One slh_xattn_map behind a collected cross-attention, while its q and k are live; coef and accumulate are set once the
        level's layers are counted (_finish_maps)"""
        B = self.B
        d = lib.XattnMapDesc(q=q.ptr, k=k.ptr, wt=self.io["xattn_wt"].ptr, out=self.io[f"xattn_map.{factor}"].ptr, B=B, b0=B // 2,
                             nb=B // 2, H=heads, D=q.C // heads, Tq=q.HW, Tk=self.ctx_len, ldq=q.ld, ldk=k.ld,
                             scale=(q.C // heads) ** -0.5)
        self.map_ops.setdefault(factor, []).append(d)
        self.add(lib.OP_XATTN_MAP, d, name)

    def _finish_maps(self):
        """The first map op of a level writes, the others add; coef = 1 / (heads * layers of the level): the last one leaves the mean"""
        for descs in self.map_ops.values():
            for n, d in enumerate(descs):
                d.accumulate = 1 if n else 0
                d.coef = 1.0 / (d.H * len(descs))

    def act(self, B, H, W, C, name="") -> Act:
        buf = self.arena.alloc((B * H * W, C), torch.bfloat16, name)
        return Act(buf.ptr, B, H, W, C, C, buf, name)

    def key_act(self, B, H, W, C, name="") -> Act:
        """An activation that is never written or read - a tape KEY for the gradient chain (the backward keys gradient buffers on
        the forward buffer's address): one aligned granule of the arena instead of a B*H*W x C tensor."""
        buf = self.arena.alloc((128,), torch.bfloat16, name)
        return Act(buf.ptr, B, H, W, C, C, buf, name)

    def f32(self, shape, name="", zero=False) -> Buf:
        return (self.zarena if zero else self.arena).alloc(shape, torch.float32, name)

    # ------------------------------------------------------------------------------------------------
    # op emitters
    # ------------------------------------------------------------------------------------------------
    def _lora_group(self, paths: List[str]) -> Optional[List[LoraEntry]]:
        if self.lora is None:
            return None
        return self.lora.fused_group(paths)

    def skinny(self, x: Src, w_ptr: int, R: int, K: int, conv: Optional[Conv3], Mout: int, Ho: int, Wo: int,
               name: str, out: Optional[Buf] = None, bias_ptr: int = 0, out_kind: int = 0) -> Buf:
        x0, x1 = src_parts(x)
        if out is None:
            out = self.f32((Mout, R), name + ".T")
        d = lib.SkinnyDesc(**sources(x0, x1, "a", "lda", "ca"), w=w_ptr, bias=bias_ptr, out=out.ptr,
                           M=Mout, R=R, K=K, ldo=R, out_kind=out_kind, stride=1)
        if conv is not None:
            conv_fields(d, conv, x0, Ho, Wo)
        self.add(lib.OP_SKINNY, d, name)
        return out

    def gemm(self, x: Src, wname: str, N: int, name: str, **kw) -> Act:
        """y = x . W^T (+bias)(+rowbias per sample)(+LoRA)(+residual): decide the product's form, then allocate and record it (the
        keywords are _decide's).  A product that folds a LayerNorm may be refused and goes through ln_gemm instead."""
        p = self._decide(x, wname, N, name, **kw)
        assert p is not None, f"{name}: no tile takes this product"
        return self._emit(p)

    def _decide(self, x: Src, wname: str, N: int, name: str, bias: bool = True, conv: Optional[Conv3] = None,
                rowbias: Optional[Tuple[int, int]] = None, residual: Optional[Act] = None,
                lora_paths: Optional[List[str]] = None, geglu: bool = False, vt_heads: Optional[int] = None,
                ln_stats: bool = False, ln_fold: Optional[Act] = None, geglu_pre: Optional[Act] = None,
                ln_mr: bool = False, geglu16: bool = False, xattn: Optional[dict] = None,
                ln_norm: Optional[str] = None, temb_path: Optional[str] = None) -> Optional[Product]:
        """The form of one product, settled before anything is allocated or recorded: builds the descriptor - placeholder pointers
        (PH, 8, 16) for what _emit will allocate - and asks choose_tile.  Touches no arena, no tape, no list of the plan.  Returns None
        when the LayerNorm it was asked to fold (ln_fold) cannot be folded on the tile that would run: the caller (ln_gemm) then
        records the LayerNorm launch and the plain product.
        conv: the product is a 3x3 convolution.  temb_path: the resnet whose time_emb_proj output rowbias is (kept for the backward).
        vt_heads: the product is a fused q|k|v projection of that many heads; where the kernel supports it (head_dim % 64 == 0) its
        V third is written head-transposed for slh_attn_fwd straight from the epilogue (Product.d.vt_out; the returned
        activation's .vt names the buffer) - one launch and one HBM round trip of V less per self-attention.
        ln_stats: also leave per-row statistics of the result for a LayerNorm folded into the NEXT product (the returned
        activation's .ln, only when the tile that will run supports it).  ln_fold = the un-normalised activation x whose producer
        left such statistics: this product computes Linear(LayerNorm(x)) from x itself with the gamma-scaled copy of the weights
        (weights.py _put_ln_folded).
        Training passes: geglu_pre receives proj(x) itself next to the GEGLU output (the backward's pre-activation; the tape
        records this product with it as its output); ln_mr: the product also leaves the rows' (mean, rstd) of the folded LayerNorm
        (the caller allocates the buffer once the fold is accepted).
        xattn = {k, vt_ptr, vt_heads, Tk, Tq, scale}: the product is attn2.to_q and, when the tile that runs is the 128 x 128 ring
        tile, the cross-attention behind it happens in its epilogue (slh_gemm_desc.xa_*): the returned activation is then the
        attention output (.attended).
        ln_fold together with lora_paths (ln_norm = the LayerNorm's weight name): the adapter's down-projection is folded as well
        (slh_gemm_desc.ln_lora_*; A . gamma and its row sums / offsets are rebuilt from the live parameters by ONE
        slh_lora_ln_fold launch at the head of the program) - only on the ping-pong tiles; None when another tile would run."""
        x0, x1 = src_parts(x)
        cin = x0.C + (x1.C if x1 else 0)
        if conv is not None:
            sh = 1 if conv.xform else 0
            HL, WL = x0.H << sh, x0.W << sh
            Ho, Wo = (HL - 1) // conv.stride + 1, (WL - 1) // conv.stride + 1   # 3x3, pad 1
            K = 9 * cin
        else:
            Ho, Wo, K = x0.H, x0.W, cin
        M = x0.B * Ho * Wo
        grp = self._lora_group(lora_paths) if lora_paths else None
        fused = grp is not None and not self.sw.lora_unfused       # lora_down rides inside the GEMM (third operand tile)
        if ln_fold is not None and grp is not None and (not fused or ln_norm is None):
            return None                       # (the adapter's fold needs the fused adapter and the LayerNorm's parameters)
        sfx = "16" if geglu16 else ""      # GEGLU.proj in the 16 | 16 block order (slh_gemm_desc.geglu = 3)
        assert not geglu16 or (geglu and geglu_pre is None and not lora_paths)
        fold = ln_fold is not None
        d = lib.GemmDesc(**sources(x0, x1, "a", "lda", "ca"), w=self.w.ptr(wname + (".lnw" if fold else ".w") + sfx),
                         bias=self.w.ptr(wname + ".b" + sfx) if (bias and not fold) else 0,
                         rowbias=rowbias[0] if rowbias else 0,
                         lora_t=PH if (grp is not None and not fused) else 0, lora_up=self.lora.up_ptr(grp[0]) if grp else 0,
                         lora_down=self.lora.down_ptr(grp[0]) if fused else 0,
                         lora_t_out=PH if (fused and self.train) else 0,      # (T is only written out for the backward)
                         lora_rank=(4 * len(grp)) if fused else 0,
                         lora_scale=self.lora_scale_ptr if grp else 0,
                         residual=residual.ptr if residual else 0, c=PH, mode=0, stride=1, ldw=K, M=M, N=N, K=K,
                         ld_rowbias=rowbias[1] if rowbias else 0, rows_per_sample=Ho * Wo,
                         ld_t=(4 * len(grp)) if grp else 0, lora_groups=len(grp) if grp else 0,
                         ld_res=residual.ld if residual else 0, ldc=N // 2 if geglu else N,
                         geglu=(3 if geglu16 else 1) if geglu else 0, tile=0, w_layout=self.w_layout)
        if conv is not None:
            conv_fields(d, conv, x0, Ho, Wo)
        if fold:
            d.ln_in, d.ln_in_chunks, d.ln_eps = ln_fold.ln[0].ptr, ln_fold.ln[1], 1e-5
            d.ln_s, d.ln_b = self.w.ptr(wname + ".lns" + sfx), self.w.ptr(wname + ".lnb" + sfx)
            if ln_mr:
                d.ln_mr_out = PH
        if geglu_pre is not None:
            assert geglu and geglu_pre.C == N
            d.geglu_pre, d.ld_pre = geglu_pre.ptr, geglu_pre.ld
        want_ln_out = bool(ln_stats and (not self.train or not self.sw.train_no_ln_fold) and not geglu and N % 64 == 0)
        vt = None
        if vt_heads and not geglu and conv is None and not self.sw.no_fused_vt and \
                (not self.train or not self.sw.train_no_fused_vt):
            Cq = N // 3
            Dh, Tk = Cq // vt_heads, Ho * Wo
            if Dh % 64 == 0 and (2 * Cq) % 128 == 0 and Tk % 64 == 0:
                # (training passes keep V row-major too: the backward reads it so)
                vt = dict(vt_col0=2 * Cq, vt_D=Dh, vt_heads=vt_heads, vt_tokens=Tk, vt_ld=Tk, vt_also_c=1 if self.train else 0)
        xa = None
        if xattn is not None:
            k = xattn["k"]
            xa = dict(xa_k=k.ptr, xa_vt=xattn["vt_ptr"], xa_tk=xattn["Tk"], xa_tq=xattn["Tq"], xa_ldk=k.ld, xa_ldvt=xattn["ldvt"],
                      xa_vt_heads=xattn["vt_heads"], xa_scale=xattn["scale"])
        ln_cols = choose_tile(d, ln_out=want_ln_out, vt=vt, xa=xa)
        if ln_cols is None:
            return None
        return Product(d, ln_cols, fused, geglu_pre, ln_norm, GemmRec(name, x, wname, N, K, Ho, Wo, conv, grp, residual, temb_path))

    def _emit(self, p: Product) -> Act:
        """Allocate what the product settled by _decide needs, fill in the real pointers, record the launch and its tape record.  The
        order of the allocations is part of the plan (addresses): output; T (unfused adapter: T, then the down-projection's launch);
        the folded adapter's A . gamma and sums; split-K workspace; statistics chunks; V^T."""
        d, rec = p.d, p.rec
        name, grp, M, N, K, Ho, Wo = rec.name, rec.grp, d.M, d.N, d.K, rec.Ho, rec.Wo
        B = src_parts(rec.x)[0].B
        out = self.act(B, Ho, Wo, d.ldc, name)
        d.c = out.ptr
        T = None
        if grp is not None:
            R = sum(e.target.rank for e in grp)
            if not p.fused:
                T = self.skinny(rec.x, self.lora.down_ptr(grp[0]), R, K, rec.conv, M, Ho, Wo, name + ".lora_down")
                d.lora_t = T.ptr
            elif self.train:
                T = self.f32((M, R), name + ".T")
                d.lora_t_out = T.ptr
        if d.ln_in and grp is not None:
            R = 4 * len(grp)
            a2 = self.arena.alloc((R, K), torch.bfloat16, name + ".lnA")
            sc = self.f32((2, 16), name + ".lnA_sc")
            d.lora_down, d.ln_lora_s, d.ln_lora_c = a2.ptr, sc.ptr, sc.ptr + 64
            self.lnfold_items.append(lib.lnfold_item(self.lora.down_ptr(grp[0]), self.w.ptr(p.ln_norm + ".g"), self.w.ptr(p.ln_norm + ".b"),
                                                     a2.ptr, sc.ptr, sc.ptr + 64, R, K))
        self.provision_splitk(d, name)
        if p.ln_cols:
            st = self.f32((N // p.ln_cols, M, 2), name + ".ln_chunks")
            d.ln_out = st.ptr
            out.ln = (st, N // p.ln_cols)
        if d.vt_out:
            vtb = self.arena.alloc((B, d.vt_heads, d.vt_D, d.vt_tokens), torch.bfloat16, name + ".vt")
            d.vt_out = vtb.ptr
            out.vt = (vtb.ptr, 0)
        out.attended = bool(d.xa_k)
        self.add(lib.OP_GEMM, d, name)
        if self.train:
            rec.out, rec.T = p.geglu_pre if p.geglu_pre is not None else out, T
            self.tape.append(rec)
        return out

    def groupnorm(self, x: Src, wname: str, eps: float, act: int, name: str) -> Act:
        x0, x1 = src_parts(x)
        C = x0.C + (x1.C if x1 else 0)
        B, H, W = x0.B, x0.H, x0.W
        G = self.cfg.norm_num_groups
        # statistics are reduced in a fixed order (bit-reproducible pass): per-workgroup partials + arrival tickets; only
        # the tickets need the zeroed arena
        stats = self.f32((B, G, 2), name + ".stats")
        prow, ntick = lib.gn_workspace(C, H * W, G)
        part = self.f32((B, prow, G, 2), name + ".partial")
        ticket = self.f32((B, ntick), name + ".ticket", zero=True)
        y = self.act(B, H, W, C, name)
        d = lib.GnDesc(**sources(x0, x1, "x", "ldx", "c"), gamma=self.w.ptr(wname + ".g"), beta=self.w.ptr(wname + ".b"),
                       stats=stats.ptr, y=y.ptr, batch=B, hw=H * W, groups=G, ldy=y.ld, eps=eps, act=act, partial=part.ptr,
                       ticket=ticket.ptr)
        one = lib.gn_fused_ok(C, H * W, G)      # 1: tiny tensor, one workgroup per group set; 2: cache-resident slab, sibling workgroups
        if one == 2 and self.sw.gn_split_slab:
            one = 0
        if one and not self.sw.gn_two_launch:
            self.add(lib.OP_GN_FUSED, d, name + ".fused")
        else:
            self.add(lib.OP_GN_STATS, d, name + ".stats")
            self.add(lib.OP_GN_APPLY, d, name + ".apply")
        if self.train:
            self.tape.append(GnRec(name, x, y, wname, eps, act, stats))
        return y

    def layernorm(self, x: Act, wname: str, name: str) -> Act:
        y = self.act(x.B, x.H, x.W, x.C, name)
        mr = self.f32((x.M, 2), name + ".mean_rstd") if self.train else None
        d = lib.LnDesc(x=x.ptr, gamma=self.w.ptr(wname + ".g"), beta=self.w.ptr(wname + ".b"), y=y.ptr,
                       mean_rstd=mr.ptr if mr else 0, M=x.M, C=x.C, ldx=x.ld, ldy=y.ld, eps=1e-5)
        self.add(lib.OP_LAYERNORM, d, name)
        if self.train:
            self.tape.append(LnRec(name, x, y, wname, mr))
        return y

    def ln_gemm(self, h: Act, norm: str, wname: str, N: int, bias: bool = True, lora_paths: Optional[List[str]] = None,
                geglu: bool = False, vt_heads: Optional[int] = None, geglu_pre: Optional[Act] = None, geglu16: bool = False,
                xattn: Optional[dict] = None) -> Act:
        """Linear(LayerNorm(h)): folded into one product when h's producer left row statistics and _decide finds a tile that takes
        the fold; the LayerNorm launch + the plain product otherwise.  Nothing is allocated or recorded before the fold is settled."""
        grp = self._lora_group(lora_paths) if lora_paths else None
        foldable = h.ln is not None and getattr(self.w, "ln_fold", False) and \
            self.w.has(wname + ".lnw") and h.C % 64 == 0 and h.C <= 1280 and h.ld == h.C
        p = None
        if foldable and grp is not None:
            if not self.train and not geglu and not self.sw.no_lora_ln_fold:
                # adapter-carrying consumer (q|k|v under noxattn): the fold covers the adapter's down-projection too
                p = self._decide(h, wname, N, wname, bias=False, lora_paths=lora_paths, vt_heads=vt_heads, ln_fold=h, ln_norm=norm)
        elif foldable and not self.train:
            p = self._decide(h, wname, N, wname, bias=False, geglu=geglu, vt_heads=vt_heads, ln_fold=h,
                             geglu16=geglu16 and self.w.has(wname + ".lnw16"), xattn=xattn)
        elif foldable and not self.sw.train_no_ln_fold:
            # training pass: the same fold; the product also leaves (mean, rstd) per row for the LayerNorm backward, and the
            # tape keeps the LayerNorm and the product as two records around a stand-in for the normalised tensor (a key for the
            # gradient chain: nothing reads its memory)
            p = self._decide(h, wname, N, wname, bias=False, geglu=geglu, ln_fold=h, ln_mr=True, geglu_pre=geglu_pre)
            if p is not None:
                mr = self.f32((h.M, 2), norm + ".mean_rstd")
                stand_in = self.key_act(h.B, h.H, h.W, h.C, norm + ".unwritten")
                self.tape.append(LnRec(norm, h, stand_in, norm, mr))
                p.behind_ln_record(stand_in, mr)
        if p is not None:
            return self._emit(p)
        n = self.layernorm(h, norm, norm)
        return self.gemm(n, wname, N, wname, bias=bias, lora_paths=lora_paths, geglu=geglu, vt_heads=vt_heads,
                         geglu_pre=geglu_pre, geglu16=geglu16 and geglu_pre is None and self.w.has(wname + ".w16"), xattn=xattn)

    def attention(self, q: Act, k: Act, v: Act, Tk: int, heads: int, name: str, vt_pre=None) -> Act:
        """q [B*Tq][C] view, k/v [B*Tk][C] views (any ld); returns [B*Tq][C].  vt_pre = (pointer to this layer's first
        head inside an already transposed [B][heads_total][Dp][ldt] array, heads_total)."""
        B, Tq, C = q.B, q.HW, q.C
        D = C // heads
        assert D * heads == C and D % 8 == 0 and D <= 192, f"unsupported head_dim {D}"
        Dp, ldt = head_t(D, Tk)
        if vt_pre is None:
            vt = self.arena.alloc((B, heads, Dp, ldt), torch.bfloat16, name + ".vt")
            self.add(lib.OP_TRANSPOSE_HEADS, lib.TransposeDesc(src=v.ptr, dst=vt.ptr, B=B, H=heads, T=Tk, ld=v.ld,
                                                               ldt=ldt, D=D), name + ".vt")
            vt_ptr, vt_heads = vt.ptr, 0
        else:
            vt_ptr, vt_heads = vt_pre
        o = self.act(q.B, q.H, q.W, C, name)
        lse = self.f32((B * heads * Tq + 64,), name + ".lse") if self.train else None   # padded: bwd reads by 64s
        d = lib.AttnDesc(q=q.ptr, k=k.ptr, vt=vt_ptr, o=o.ptr, lse=lse.ptr if lse else 0, B=B, H=heads, Tq=Tq, Tk=Tk,
                         ldq=q.ld, ldk=k.ld, ldvt=ldt, ldo=o.ld, scale=D ** -0.5, D=D, vt_batch_heads=vt_heads)
        self.add(lib.OP_ATTN_FWD, d, name)
        if self.train:
            self.tape.append(AttnRec(name, q, k, v, o, lse, Tk, heads))
        return o

    # ------------------------------------------------------------------------------------------------
    # network pieces
    # ------------------------------------------------------------------------------------------------
    def _embeddings(self):
        cfg, B, w = self.cfg, self.B, self.w
        ted = cfg.time_embed_dim
        c0 = cfg.block_out_channels[0]
        a = self.arena
        t_in = a.alloc((B, c0), torch.bfloat16, "temb.sin")
        self.add(lib.OP_TEMBED, lib.TembedDesc(vals=self.io["t"].ptr, out=t_in.ptr, nb=B, n_vals=1, dim=c0,
                                               ldo=c0, col0=0), "time_proj")
        h1 = a.alloc((B, ted), torch.bfloat16, "temb.h1")
        self._gemv(t_in.ptr, c0, "time_embedding.linear_1", ted, c0, h1.ptr, ted, 0, name="time_embedding.linear_1")
        emb = a.alloc((B, ted), torch.bfloat16, "temb.emb")
        self._gemv(h1.ptr, ted, "time_embedding.linear_2", ted, ted, emb.ptr, ted, 1, name="time_embedding.linear_2")
        if cfg.is_xl:
            add_in = self.io["add_in"]
            pin = cfg.projection_class_embeddings_input_dim
            self.add(lib.OP_TEMBED, lib.TembedDesc(vals=self.io["time_ids"].ptr, out=add_in.ptr, nb=B, n_vals=6,
                                                   dim=cfg.addition_time_embed_dim, ldo=pin,
                                                   col0=cfg.pooled_dim), "add_time_proj")
            g1 = a.alloc((B, ted), torch.bfloat16, "aemb.h1")
            self._gemv(add_in.ptr, pin, "add_embedding.linear_1", ted, pin, g1.ptr, ted, 0, name="add_embedding.linear_1")
            emb2 = a.alloc((B, ted), torch.bfloat16, "temb.emb_sum")
            self._gemv(g1.ptr, ted, "add_embedding.linear_2", ted, ted, emb2.ptr, ted, 1, addend=(emb.ptr, ted),
                       name="add_embedding.linear_2")
            emb = emb2
        self.emb = emb
        # every ResnetBlock2D.time_emb_proj(silu(emb)) in one launch
        tot = w.temb_total
        self.temb_all = a.alloc((B, tot), torch.bfloat16, "temb.proj_all")
        lt = None
        if self.lora is not None and self.lora.temb_entries:
            L = len(self.lora.temb_entries)
            if L != len(w.resnet_paths):
                raise NotImplementedError("time_emb_proj adapters must cover every resnet or none")
            lt = self.f32((B, 4 * L), "temb.lora_T")
            d = lib.GemvDesc(x=emb.ptr, w=self.lora.params.data_ptr() + 2 * self.lora.temb_down_off, y=lt.ptr,
                             nb=B, N=4 * L, K=ted, ldx=ted, ldy=4 * L, in_act=1, out_f32=1)
            self.add(lib.OP_GEMV, d, "temb.lora_down")
        d = lib.GemvDesc(x=emb.ptr, w=w.ptr("temb_proj.w"), bias=w.ptr("temb_proj.b"), y=self.temb_all.ptr,
                         nb=B, N=tot, K=ted, ldx=ted, ldy=tot, in_act=1, out_f32=0)
        if lt is not None:
            d.lora_t = lt.ptr
            d.ld_t = lt.shape[1]
            d.lora_tcol = self.lora.temb_tcol_table(w).data_ptr()
            d.lora_up = self.lora.params.data_ptr() + 2 * self.lora.temb_up_off
            d.lora_scale = self.lora_scale_ptr
        self.add(lib.OP_GEMV, d, "time_emb_proj_all")
        self.temb_lora_T = lt

    def _gemv(self, x_ptr, ldx, wname, N, K, y_ptr, ldy, in_act, addend=None, name=""):
        d = lib.GemvDesc(x=x_ptr, w=self.w.ptr(wname + ".w"), bias=self.w.ptr(wname + ".b"), y=y_ptr,
                         addend=addend[0] if addend else 0, ld_add=addend[1] if addend else 0,
                         nb=self.B, N=N, K=K, ldx=ldx, ldy=ldy, in_act=in_act, out_f32=0)
        self.add(lib.OP_GEMV, d, name)

    def _resnet(self, x: Src, path: str, cout: int) -> Act:
        x0, x1 = src_parts(x)
        cin = x0.C + (x1.C if x1 else 0)
        eps = self.cfg.norm_eps
        a1 = self.groupnorm(x, path + ".norm1", eps, 1, path + ".norm1")
        rb = (self.temb_all.ptr + 2 * self.w.temb_offsets[path], self.w.temb_total)
        h = self.gemm(a1, path + ".conv1", cout, path + ".conv1", conv=Conv3(), rowbias=rb, temb_path=path,
                      lora_paths=[path + ".conv1"])
        a2 = self.groupnorm(h, path + ".norm2", eps, 1, path + ".norm2")
        if cin != cout:
            sc = self.gemm(x, path + ".conv_shortcut", cout, path + ".conv_shortcut",
                           lora_paths=[path + ".conv_shortcut"])
        else:
            assert x1 is None
            sc = x0
        return self.gemm(a2, path + ".conv2", cout, path + ".conv2", conv=Conv3(), residual=sc,
                         lora_paths=[path + ".conv2"])

    def _tblock(self, h: Act, path: str, heads: int, ctx: Act) -> Act:
        C = h.C
        a1, a2 = path + ".attn1", path + ".attn2"
        # BasicTransformerBlock.norm1/2/3: in the no-grad passes a LayerNorm whose consumer carries no adapter is folded
        # into that product (ln_gemm); its producer leaves the row statistics (ln_stats)
        qkv = self.ln_gemm(h, path + ".norm1", a1 + ".qkv", 3 * C, bias=False,
                           lora_paths=[a1 + ".to_q", a1 + ".to_k", a1 + ".to_v"], vt_heads=heads)
        T = h.HW
        o1 = self.attention(qkv.cols(0, C), qkv.cols(C, C), qkv.cols(2 * C, C), T, heads, a1 + ".sdpa", vt_pre=qkv.vt)
        h1 = self.gemm(o1, a1 + ".out", C, a1 + ".out", residual=h, lora_paths=[a1 + ".to_out.0"], ln_stats=True)
        vt_pre = None
        if self.kv_all is not None:
            k_off, v_off = self.w.kv_all_offset[a2]
            k2, v2, kv = self.kv_all.cols(k_off, C), self.kv_all.cols(v_off, C), self.kv_all
            if self.vt_all is not None:
                D = C // heads
                Dp, ldt = head_t(D, self.ctx_len)
                vt_pre = (self.vt_all.ptr + 2 * ((v_off - self.w.kv_all_vbase) // D) * Dp * ldt, self.vt_all_heads)
        else:
            kv = self.gemm(ctx, a2 + ".kv", 2 * C, a2 + ".kv", bias=False, lora_paths=[a2 + ".to_k", a2 + ".to_v"])
            k2, v2 = kv.cols(0, C), kv.cols(C, C)
        if self._lora_group([a2 + ".to_k", a2 + ".to_v"]) is None:
            self.nograd_kv.add(kv.buf.ptr)      # text K/V carry no gradient unless they are adapted
        # no-grad passes, head dim 64, text keys, no adapter on to_q: the attention runs in the epilogue of the query projection
        xa = None
        D2 = C // heads
        map_factor = self._map_factor(h)          # a collected layer keeps q2 in memory: its attention is a launch of its own
        # (the gate restates slh_gemm's own checks for xa_*: head dim 64 with whole 64-column heads, 65..96 keys - two 64-key V^T
        # tiles are always staged, so xa_ldvt = roundup(ctx_len, 64) must reach 128 - and whole 128-row query tiles per sample)
        if not self.train and vt_pre is not None and D2 == 64 and C % 64 == 0 and 64 < self.ctx_len <= 96 and h.HW % 128 == 0 and \
                self._lora_group([a2 + ".to_q"]) is None and not self.sw.no_fused_xattn and map_factor is None:
            xa = dict(k=k2, vt_ptr=vt_pre[0], vt_heads=vt_pre[1], Tk=self.ctx_len, Tq=h.HW, scale=D2 ** -0.5,
                      ldvt=head_t(D2, self.ctx_len)[1])
        q2 = self.ln_gemm(h1, path + ".norm2", a2 + ".q", C, bias=False, lora_paths=[a2 + ".to_q"], xattn=xa)
        if q2.attended:
            o2 = q2
        else:
            o2 = self.attention(q2, k2, v2, self.ctx_len, heads, a2 + ".sdpa", vt_pre=vt_pre)
            if map_factor is not None:
                self._record_map(q2, k2, heads, map_factor, a2 + ".map")
        h2 = self.gemm(o2, a2 + ".out", C, a2 + ".out", residual=h1, lora_paths=[a2 + ".to_out.0"], ln_stats=True)
        if self.train and (self._lora_group([path + ".ff.net.0.proj"]) is not None or
                           self.sw.train_unfused_geglu):
            n3 = self.layernorm(h2, path + ".norm3", path + ".norm3")
            pre = self.gemm(n3, path + ".ff1", 8 * C, path + ".ff1", lora_paths=[path + ".ff.net.0.proj"])
            ff = self.act(h.B, h.H, h.W, 4 * C, path + ".geglu")
            self.add(lib.OP_ELEMENTWISE, lib.EwDesc(a=pre.ptr, out=ff.ptr, M=pre.M, C=4 * C, lda=pre.ld, ldo=ff.ld,
                                                    op=lib.EW_GEGLU_FWD), path + ".geglu")
            self.tape.append(GegluRec(path + ".geglu", pre, ff))
        elif self.train:
            # one launch: the GEGLU epilogue also stores proj(x) for the backward (and norm3 folds into it when h2's producer
            # left row statistics)
            pre = self.act(h.B, h.H, h.W, 8 * C, path + ".ff1")
            ff = self.ln_gemm(h2, path + ".norm3", path + ".ff1", 8 * C, geglu=True, geglu_pre=pre)
            self.tape.append(GegluRec(path + ".geglu", pre, ff))
        else:
            grp = self._lora_group([path + ".ff.net.0.proj"])
            if grp is not None:
                raise NotImplementedError("LoRA on GEGLU.proj is not a reference target")
            ff = self.ln_gemm(h2, path + ".norm3", path + ".ff1", 8 * C, geglu=True, geglu16=getattr(self.w, "geglu16", False))
        return self.gemm(ff, path + ".ff2", C, path + ".ff2", residual=h2, lora_paths=[path + ".ff.net.2"], ln_stats=True)

    def _transformer(self, x: Act, path: str, layers: int, heads: int) -> Act:
        g = self.groupnorm(x, path + ".norm", 1e-6, 0, path + ".norm")
        h = self.gemm(g, path + ".proj_in", x.C, path + ".proj_in", lora_paths=[path + ".proj_in"], ln_stats=True)
        for k in range(layers):
            h = self._tblock(h, f"{path}.transformer_blocks.{k}", heads, self.ctx)
        return self.gemm(h, path + ".proj_out", x.C, path + ".proj_out", residual=x, lora_paths=[path + ".proj_out"])

    def _forward(self):
        cfg, B, H, W = self.cfg, self.B, self.H, self.W
        boc = cfg.block_out_channels
        self._embeddings()
        ctxb = self.io["ctx"]
        self.ctx = Act(ctxb.ptr, B, 1, self.ctx_len, cfg.cross_attention_dim, cfg.cross_attention_dim, ctxb, "ctx")
        # every transformer block projects the same text embeddings to K/V: when those projections carry no adapter they
        # run as ONE GEMM over the concatenated weights at the head of the pass - the training forward included (rounds 1-2
        # kept per-block projections there because the batched layout exposed an LDS-DMA publish race in the attention
        # kernels: profiles/r02_lds_dma_race_fix.txt; fixed, and green on the GPU suite x2 + 0/16 on the reproducer,
        # profiles/r03_first_call.txt.  SLIDERS_TRAIN_KV_PER_BLOCK=1 restores the old form for A/B runs.)
        self.kv_all = self.vt_all = None
        kvo = getattr(self.w, "kv_all_offset", None)
        if kvo and not (self.train and self.sw.train_kv_per_block) and \
                all(self._lora_group([a + ".to_k", a + ".to_v"]) is None for a in kvo):
            n_all = self.w.gemm_shape["attn2_kv_all.w"][0]
            self.kv_all = self.gemm(self.ctx, "attn2_kv_all", n_all, "attn2_kv_all", bias=False)
            # one head dim everywhere (SDXL: 64) -> the V halves of all blocks are one [B*77][sum(C)] matrix whose
            # heads transpose in ONE launch; each block's attention then points at its own heads of that array
            dims = {boc[i] // cfg.attention_head_dim[i] for i, t in enumerate(cfg.down_block_types) if t != "DownBlock2D"}
            dims.add(boc[-1] // cfg.attention_head_dim[-1])
            if len(dims) == 1:
                D = dims.pop()
                vb = self.w.kv_all_vbase
                self.vt_all_heads = vb // D
                Dp, ldt = head_t(D, self.ctx_len)
                self.vt_all =self.arena.alloc((B, self.vt_all_heads, Dp, ldt), torch.bfloat16, "attn2_vt_all")
                self.add(lib.OP_TRANSPOSE_HEADS, lib.TransposeDesc(
                    src=self.kv_all.ptr + 2 * vb, dst=self.vt_all.ptr, B=B, H=self.vt_all_heads, T=self.ctx_len,
                    ld=self.kv_all.ld, ldt=ldt, D=D), "attn2_vt_all")
        h = self.act(B, H, W, boc[0], "conv_in")
        self.nograd = {ctxb.ptr, h.buf.ptr}     # nothing trainable upstream of these
        self.nograd_kv = set()
        self.add(lib.OP_CONV_IN, lib.ConvInDesc(x=self.io["sample"].ptr, w=self.w.ptr("conv_in.w"),
                                                bias=self.w.ptr("conv_in.b"), y=h.ptr, batch=B,
                                                cin=cfg.in_channels, h=H, wd=W, cout=boc[0], ldy=h.ld), "conv_in")
        skips = [h]
        # block name -> the activation diffusers' block returns (after its down / upsampler): read by the parity tests' per-block
        # error ledger after a pass (no buffer is reused inside a pass, so they are all still there); nothing else uses it
        self.block_out: Dict[str, Act] = {}
        for i, t in enumerate(cfg.down_block_types):
            path = f"down_blocks.{i}"
            cout = boc[i]
            final = i == len(boc) - 1
            for j in range(cfg.layers_per_block):
                h = self._resnet(h, f"{path}.resnets.{j}", cout)
                if t != "DownBlock2D":
                    h = self._transformer(h, f"{path}.attentions.{j}", cfg.transformer_layers_per_block[i],
                                          cfg.attention_head_dim[i])
                skips.append(h)
            if not final:
                p = f"{path}.downsamplers.0.conv"
                h = self.gemm(h, p, cout, p, conv=Conv3(stride=2), lora_paths=[p])
                skips.append(h)
            self.block_out[path] = h
        mp = "mid_block"
        h = self._resnet(h, mp + ".resnets.0", boc[-1])
        h = self._transformer(h, mp + ".attentions.0", cfg.transformer_layers_per_block[-1], cfg.attention_head_dim[-1])
        h = self._resnet(h, mp + ".resnets.1", boc[-1])
        self.block_out[mp] = h
        rboc = tuple(reversed(boc))
        rheads = tuple(reversed(cfg.attention_head_dim))
        rtl = tuple(reversed(cfg.transformer_layers_per_block))
        for i, t in enumerate(cfg.up_block_types):
            path = f"up_blocks.{i}"
            cout = rboc[i]
            final = i == len(boc) - 1
            for j in range(cfg.layers_per_block + 1):
                skip = skips.pop()
                h = self._resnet((h, skip), f"{path}.resnets.{j}", cout)
                if t != "UpBlock2D":
                    h = self._transformer(h, f"{path}.attentions.{j}", rtl[i], rheads[i])
            if not final:
                p = f"{path}.upsamplers.0.conv"
                h = self.gemm(h, p, cout, p, conv=Conv3(xform=1), lora_paths=[p])
            self.block_out[path] = h
        assert not skips
        g = self.groupnorm(h, "conv_norm_out", cfg.norm_eps, 1, "conv_norm_out")
        self.skinny(g, self.w.ptr("conv_out.w"), cfg.out_channels, 9 * g.C, Conv3(), g.M, g.H, g.W, "conv_out",
                    out=self.io["eps"], bias_ptr=self.w.ptr("conv_out.b"), out_kind=1)
        if self.train:
            self.tape.append(ConvOutRec(g))


def __getattr__(name):
    """`from sliders_amd.planner import BackwardPlan` keeps working: it lives in backward.py, which imports this module"""
    if name != "BackwardPlan":
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    from .backward import BackwardPlan
    return BackwardPlan

