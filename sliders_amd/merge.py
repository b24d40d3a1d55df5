"""Sampling with several sliders of any rank: the adapters are folded into the frozen weights.

During a denoise loop the adapters are constants, so

    W' = W + sum_i  s_i * (alpha_i / r_i) * B_i . A_i

is computed once (slh_lora_merge, csrc/merge.hip) and the adapter-free programs run on W': any rank, any number of
sliders, any mix of train_methods, per-slider alpha and scale - and no adapter work per step.  Training and the fused
single-slider path (rank 4, UNetEngine.attach_lora) are untouched.

The frozen weights are not plain matrices (weights.py): tile-packed with the LDS swizzle applied, q|k|v and k|v fused by
rows, every cross-attention K/V held a second time in attn2_kv_all.w, LayerNorm-folded copies with their row sums, all
time_emb_proj concatenated.  `WeightMerger` maps every adapted module to each stored copy of it, as one item (a row range
of one stored tensor) per copy; the kernel writes those layouts directly, in place, so the pointers inside plans and
captured graphs stay valid.

`SliderSet`     the sliders: factors as fp32 [out][r] / [r][K] (conv K order tap * Cin + c), alpha, rank, scale.
`WeightMerger`  the item table over a WeightStore + merge(scales) / restore().

Rounding: merging re-rounds W' to bf16, where the fused path keeps the adapter product beside W in fp32.  DESIGN.md has
the measured cost.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import lib
from .config import UNetConfig
from .modules import LORA_PREFIX_UNET, _LEAF_CLASSES, build_tree
from .weights import WeightStore


def module_names(cfg: UNetConfig) -> Dict[str, Tuple[str, object]]:
    """lora_unet_* name -> (dotted module path, leaf node) for every Linear / Conv2d of this UNet: the reference's naming
    (lora.py:206-208) over the module tree of modules.py."""
    out = {}
    for path, node in build_tree(cfg).named_modules():
        if node.cls in _LEAF_CLASSES:
            out[(LORA_PREFIX_UNET + "." + path).replace(".", "_")] = (path, node)
    return out


@dataclass
class SliderModule:
    path: str               # dotted diffusers path of the adapted Linear / Conv2d
    up: torch.Tensor        # fp32 [out][r]
    down: torch.Tensor      # fp32 [r][K], conv 3x3 in the implicit-GEMM K order tap * Cin + c
    alpha: float
    rank: int


class Slider:
    def __init__(self, modules: List[SliderModule], scale: Optional[float]):
        self.modules, self.scale = modules, scale
        self.rank = max(m.rank for m in modules)


class SliderSet:
    """sliders: [(state dict in the reference's checkpoint layout | LoraStore, scale), ...].  scale None marks the slider that
    `SliderSampler.sample_latents(scale=...)` sweeps; the others are held at their own scale.  Rank is read from
    lora_down.weight.shape[0], alpha from the `.alpha` key (absent: alpha = rank, as the reference's LoRAModule), the target from the
    key name; a key that names no Linear / Conv2d of this UNet raises."""

    def __init__(self, cfg: UNetConfig, sliders: Sequence[tuple]):
        self.cfg = cfg
        names = module_names(cfg)
        self.sliders: List[Slider] = []
        for src, scale in sliders:
            sd = src.state_dict() if hasattr(src, "state_dict") and not isinstance(src, dict) else src
            mods, unknown, seen = [], [], set()
            for key in sd:
                name = key.split(".", 1)[0]
                if name in seen:
                    continue
                seen.add(name)
                if name not in names:
                    unknown.append(key)
                    continue
                kd, ku = f"{name}.lora_down.weight", f"{name}.lora_up.weight"
                if kd not in sd or ku not in sd:
                    raise KeyError(f"slider {len(self.sliders)}: {name} needs both lora_down.weight and lora_up.weight")
                path, node = names[name]
                down, up = sd[kd].detach().to("cpu", torch.float32), sd[ku].detach().to("cpu", torch.float32)
                r = down.shape[0]
                kk = max(node.kernel, 1)
                if tuple(down.shape[:2]) != (r, node.in_dim) or down.numel() != r * node.in_dim * kk * kk \
                        or up.shape[0] != node.out_dim or up.numel() != node.out_dim * r:
                    raise ValueError(f"{name}: lora_down {tuple(down.shape)} / lora_up {tuple(up.shape)} do not fit a "
                                     f"{node.in_dim} -> {node.out_dim} module (kernel {node.kernel})")
                if down.dim() == 4:
                    down = down.permute(0, 2, 3, 1)              # (r, Cin, kh, kw) -> tap-major, once
                alpha = float(sd[f"{name}.alpha"]) if f"{name}.alpha" in sd else float(r)
                mods.append(SliderModule(path, up.reshape(node.out_dim, r).contiguous(), down.reshape(r, -1).contiguous(), alpha, r))
            if unknown:
                raise KeyError(f"slider {len(self.sliders)}: {len(unknown)} key(s) match no module of this UNet: {sorted(unknown)[:6]}")
            if not mods:
                raise ValueError(f"slider {len(self.sliders)}: no adapter weights")
            self.sliders.append(Slider(mods, None if scale is None else float(scale)))

    def __len__(self):
        return len(self.sliders)

    def scales(self, swept: float = 0.0) -> List[float]:
        return [float(swept) if s.scale is None else s.scale for s in self.sliders]


@dataclass
class MergeItem:
    """One row range of one stored tensor (slh_lora_merge_item).  `base` and `out` name tensors of WeightStore.t: out is written from
    the pristine copy of base."""
    path: str
    base: str
    out: str
    n0: int
    rows: int
    N: int
    K: int
    packed: bool
    u: torch.Tensor                 # fp32 [rows][R]: all sliders' up factors side by side
    d: torch.Tensor                 # fp32 [R][K]
    c_off: int                      # first of this module's R coefficients in WeightMerger.coef
    gamma: Optional[str] = None     # LayerNorm-folded copy: names of the norm's weight / bias, of the row sums and the folded bias
    beta: Optional[str] = None
    lns: Optional[str] = None
    lnb: Optional[str] = None

    @property
    def R(self) -> int:
        return self.d.shape[0]


class WeightMerger:
    def __init__(self, w: WeightStore, sliders: SliderSet):
        self.w, self.sliders = w, sliders
        self.items: List[MergeItem] = []
        self.merged = False
        self._pristine: Optional[Dict[str, torch.Tensor]] = None
        self._desc = self._keep = None
        by_path: Dict[str, List[Tuple[int, SliderModule]]] = {}
        for si, s in enumerate(sliders.sliders):
            for m in s.modules:
                by_path.setdefault(m.path, []).append((si, m))
        alpha, owner = [], []
        unsupported = []
        for path, mods in by_path.items():
            copies = self._copies(path)
            if copies is None:
                unsupported.append(path)
                continue
            u = torch.cat([m.up for _, m in mods], 1).contiguous().to(w.device)
            d = torch.cat([m.down for _, m in mods], 0).contiguous().to(w.device)
            c_off = len(alpha)
            for si, m in mods:
                alpha += [m.alpha / m.rank] * m.rank
                owner += [si] * m.rank
            for cp in copies:
                assert cp["rows"] == u.shape[0] and cp["K"] == d.shape[1], (path, cp, u.shape, d.shape)
                self.items.append(MergeItem(path=path, u=u, d=d, c_off=c_off, **cp))
        if unsupported:
            raise NotImplementedError(f"no stored layout to merge into for: {sorted(unsupported)[:6]} (of {len(unsupported)})")
        self._alpha = torch.tensor(alpha, dtype=torch.float32)
        self._owner = torch.tensor(owner, dtype=torch.int64)
        self.coef = torch.zeros(len(alpha), dtype=torch.float32, device=w.device)
        self.touched = sorted({n for it in self.items for n in (it.out, it.lns, it.lnb) if n})

    # ---- module path -> every stored copy of its weight ------------------------------------------------------------------------
    def _matrix(self, name: str, n0: int, rows: int, base: Optional[str] = None) -> dict:
        w = self.w
        if name in w.gemm_shape:
            N, K = w.gemm_shape[name]
            packed = w.packed
        else:
            N, K = w.t[name].shape
            packed = False
        return dict(base=base or name, out=name, n0=n0, rows=rows, N=N, K=K, packed=packed)

    def _copies(self, path: str) -> Optional[List[dict]]:
        w = self.w
        head, _, leaf = path.rpartition(".")
        if leaf in ("to_q", "to_k", "to_v") and head.endswith(".attn1"):
            blk = head[:-len(".attn1")]
            C = w.gemm_shape[f"{head}.qkv.w"][0] // 3
            n0 = ("to_q", "to_k", "to_v").index(leaf) * C
            out = [self._matrix(f"{head}.qkv.w", n0, C)]
            if w.has(f"{head}.qkv.lnw"):
                out.append(dict(self._matrix(f"{head}.qkv.lnw", n0, C, base=f"{head}.qkv.w"), gamma=f"{blk}.norm1.g", beta=f"{blk}.norm1.b",
                                lns=f"{head}.qkv.lns", lnb=f"{head}.qkv.lnb"))
            return out
        if leaf == "to_q" and head.endswith(".attn2"):
            blk = head[:-len(".attn2")]
            C = w.gemm_shape[f"{head}.q.w"][0]
            out = [self._matrix(f"{head}.q.w", 0, C)]
            if w.has(f"{head}.q.lnw"):
                out.append(dict(self._matrix(f"{head}.q.lnw", 0, C, base=f"{head}.q.w"), gamma=f"{blk}.norm2.g", beta=f"{blk}.norm2.b",
                                lns=f"{head}.q.lns", lnb=f"{head}.q.lnb"))
            return out
        if leaf in ("to_k", "to_v") and head.endswith(".attn2"):
            C = w.gemm_shape[f"{head}.kv.w"][0] // 2
            v = leaf == "to_v"
            out = [self._matrix(f"{head}.kv.w", C if v else 0, C)]
            if head in getattr(w, "kv_all_offset", {}):
                out.append(self._matrix("attn2_kv_all.w", w.kv_all_offset[head][1 if v else 0], C))
            return out
        if path.endswith(".to_out.0"):
            name = path[:-len(".to_out.0")] + ".out.w"
        elif path.endswith(".ff.net.2"):
            name = path[:-len(".ff.net.2")] + ".ff2.w"
        elif leaf == "time_emb_proj":
            if head not in w.temb_offsets:
                return None
            rows = w.gemm_shape[f"{head}.conv1.w"][0]
            return [self._matrix("temb_proj.w", w.temb_offsets[head], rows)]
        elif leaf in ("proj_in", "proj_out", "conv1", "conv2", "conv_shortcut", "conv"):
            name = path + ".w"
        else:
            return None         # GEGLU.proj (row-permuted copies), conv_in / conv_out, the embedding MLPs
        if name not in w.gemm_shape:
            return None
        return [self._matrix(name, 0, w.gemm_shape[name][0])]

    # ---- device side -----------------------------------------------------------------------------------------------------------
    def coefficients(self, scales: Sequence[float]) -> torch.Tensor:
        """c[r] = scale_i * alpha_i / rank_i over the concatenated R of every module (host, fp32)"""
        if len(scales) != len(self.sliders):
            raise ValueError(f"{len(scales)} scales for {len(self.sliders)} sliders")
        return self._alpha * torch.tensor([float(s) for s in scales], dtype=torch.float32)[self._owner]

    def _build(self):
        w = self.w
        self._pristine = {n: w.t[n].clone() for n in self.touched}        # of the touched tensors only, on first use
        ptr = lambda n: w.t[n].data_ptr() if n else 0
        recs = []
        for it in self.items:
            recs.append(lib.LoraMergeItem(
                base=self._pristine[it.base].data_ptr(), out=ptr(it.out), u=it.u.data_ptr(), d=it.d.data_ptr(),
                c=self.coef.data_ptr() + 4 * it.c_off, gamma=ptr(it.gamma), beta=ptr(it.beta), bias=0, lns=ptr(it.lns), lnb=ptr(it.lnb),
                n0=it.n0, rows=it.rows, N=it.N, K=it.K, R=it.R, ldu=it.R, ldd=it.K, ld=0 if it.packed else it.K,
                w_layout=1 if it.packed else 0))
        self._desc, self._keep = lib.merge_table(recs, w.device)

    def merge(self, scales: Sequence[float]):
        """W' = W + sum_i scales[i] * (alpha_i / r_i) * B_i . A_i into every stored copy, one launch on the current stream, always
        from the pristine bits (merging twice does not accumulate)."""
        if self.w._dgrad_ready:
            raise RuntimeError("WeightMerger: this engine holds backward-data copies of its weights (a training pass was planned); "
                               "merged weights are for no-grad passes only")
        c = self.coefficients(scales)
        if self._desc is None:
            self._build()
        self._c_host = c.pin_memory() if self.coef.is_cuda else c      # (kept until the next merge: the upload is asynchronous)
        self.coef.copy_(self._c_host, non_blocking=True)
        lib.call(lib.OP_LORA_MERGE, self._desc, torch.cuda.current_stream().cuda_stream)
        self.merged = True

    def restore(self):
        """Put the original bits back."""
        if self._pristine is not None and self.merged:
            names = list(self._pristine)
            torch._foreach_copy_([self.w.t[n] for n in names], [self._pristine[n] for n in names])
        self.merged = False

    def nbytes_touched(self) -> int:
        return sum(self.w.t[n].numel() * self.w.t[n].element_size() for n in self.touched)
