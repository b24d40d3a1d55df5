"""Prompt-direction sampling: the signal a text slider is trained to imitate, used as guidance (docs/SAMPLING.md).

A slider's training target (trainscripts/textsliders/prompt_util.py:108-135, PromptEmbedsPair._enhance / _erase) is

    eps_target = eps(neutral) +- eta * (eps(positive) - eps(unconditional))

Here the same difference steers a sampling run without a trained slider.  One UNet pass carries, next to the rows plain sampling
runs, the `positive` and `unconditional` prompts of up to three prompts.yaml entries on the same latent, and the step sees

    m = u + g (t - u) + sum_k w_k * keep_k * (e+_k - e-_k),        w_k = scale * sign_k * eta_k

sign + for `enhance`, - for `erase`; eta the entry's guidance_scale; keep_k the sparsifier of slh_direction_threshold (the largest
entries of each latent channel).  slh_eps_direction writes the guided text row t' = rne_bf16(t + sum_k c_k keep_k d_k) that the step
kernels read through their eps_text input: c_k = w_k / g for the CFG pair, w_k for the single branch.

Momentum (SEGA's second half; momentum=(s_m, beta)): an fp32 state nu per latent element, zero when a call first acts, is added to the
guided row at strength s_m and then moved towards what the directions (and it) just gave: slh_eps_direction_momentum,
t' = rne_bf16(t + G), G = sum_k c_k keep_k d_k + s_m nu, nu <- beta nu + (1 - beta) G.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import lib
from .passes import Pass

MAX_DIRECTIONS = lib.MAX_DIRECTIONS


@dataclass
class Direction:
    """One prompt pair: the encoded `positive` and `unconditional` prompts ((1, 77, D), or one row per image; SDXL: the pooled rows too),
    eta (the entry's guidance_scale) and sign (+1 enhance, -1 erase)."""
    ctx_pos: torch.Tensor
    ctx_neg: torch.Tensor
    pooled_pos: Optional[torch.Tensor] = None
    pooled_neg: Optional[torch.Tensor] = None
    eta: float = 1.0
    sign: float = 1.0

    def swapped(self) -> "Direction":
        """the pair the other way round: at scale -s it samples what this one samples at s, bit for bit"""
        return Direction(self.ctx_neg, self.ctx_pos, self.pooled_neg, self.pooled_pos, self.eta, self.sign)


class DirectionSet:
    """Up to three directions, applied together."""

    def __init__(self, directions: Sequence[Direction]):
        self.directions: List[Direction] = list(directions)
        if not 1 <= len(self.directions) <= MAX_DIRECTIONS:
            raise ValueError(f"DirectionSet: {len(self.directions)} directions: 1 to {MAX_DIRECTIONS} (one UNet pass carries at most 8 row blocks)")
        for k, d in enumerate(self.directions):
            if d.sign not in (1.0, -1.0) or not math.isfinite(float(d.eta)):
                raise ValueError(f"DirectionSet: direction {k}: sign {d.sign!r} (+1 enhance, -1 erase), eta {d.eta!r} (finite)")
            if d.ctx_pos.shape != d.ctx_neg.shape or (d.pooled_pos is None) != (d.pooled_neg is None):
                raise ValueError(f"DirectionSet: direction {k}: the positive and the unconditional prompt are encoded alike")

    def __len__(self) -> int:
        return len(self.directions)

    @classmethod
    def from_settings(cls, entries, encode: Callable[[str], Tuple[torch.Tensor, Optional[torch.Tensor]]]) -> "DirectionSet":
        """entries: prompt_util.PromptSettings (load_prompts_from_yaml), of which `positive`, `unconditional`, `guidance_scale` and `action`
        are read; encode(text) -> (ctx (1, 77, D), pooled (1, P) or None)"""
        out = []
        for e in entries:
            (cp, pp), (cn, pn) = encode(e.positive), encode(e.unconditional)
            out.append(Direction(cp, cn, pp, pn, eta=float(e.guidance_scale), sign=1.0 if e.action == "enhance" else -1.0))
        return cls(out)

    def swapped(self) -> "DirectionSet":
        return DirectionSet([d.swapped() for d in self.directions])

    def coefficients(self, scale: float, guidance: float, single: bool) -> List[float]:
        """c_k of slh_eps_direction: w_k = scale * sign_k * eta_k for the single branch, w_k / guidance for the CFG pair - whose step
        multiplies the text row's offset from the unconditional row by the guidance"""
        w = [float(scale) * d.sign * float(d.eta) for d in self.directions]
        if single:
            return w
        if any(w) and (float(guidance) == 0.0 or not math.isfinite(float(guidance))):
            raise ValueError(f"DirectionSet: guidance_scale {guidance!r} with the CFG pair: the direction enters through the text row, which a "
                             "guidance of 0 does not read")
        return [v / float(guidance) if v != 0.0 else 0.0 for v in w]

    @staticmethod
    def n_keep(hw: int, quantile: float) -> int:
        """entries of a channel's hw pixels the sparsifier keeps (ties at the threshold come on top): hw - floor(q hw), at least 1;
        q = 0 keeps all"""
        q = float(quantile)
        if not 0.0 <= q < 1.0:
            raise ValueError(f"direction_quantile {quantile!r}: expected 0 <= q < 1")
        if hw < 1:
            raise ValueError(f"n_keep: hw = {hw}")
        return max(1, int(hw) - int(math.floor(q * int(hw))))

    def rows(self, bs: int, device) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """(ctx (2 J bs, 77, D), pooled (2 J bs, P) or None): the blocks e+_1, e-_1, ... e+_J, e-_J of bs rows each"""
        def fit(v):
            v = v.to(device)
            if v.shape[0] not in (1, bs):
                raise ValueError(f"DirectionSet: a prompt of {v.shape[0]} rows for {bs} images: expected 1 or {bs}")
            return v.expand(bs, *v.shape[1:])
        ctx = torch.cat([fit(v) for d in self.directions for v in (d.ctx_pos, d.ctx_neg)])
        if self.directions[0].pooled_pos is None:
            return ctx, None
        return ctx, torch.cat([fit(v) for d in self.directions for v in (d.pooled_pos, d.pooled_neg)])


def check_momentum(momentum) -> Optional[Tuple[float, float]]:
    """momentum=(s_m, beta) as DirectionGuide takes it -> (s_m, beta), or None where there is no momentum: None, or an s_m whose fp32
    value is 0 (the launches are then slh_eps_direction's, bit for bit).  s_m finite, 0 <= beta < 1, else a ValueError."""
    if momentum is None:
        return None
    try:
        s_m, beta = (float(v) for v in momentum)
    except (TypeError, ValueError):
        raise ValueError(f"direction_momentum {momentum!r}: expected (s_m, beta)")
    if not math.isfinite(s_m) or not 0.0 <= beta < 1.0:
        raise ValueError(f"direction_momentum {momentum!r}: expected a finite s_m and 0 <= beta < 1")
    if not math.isfinite(ctypes.c_float(s_m).value):
        raise ValueError(f"direction_momentum {momentum!r}: s_m is not finite in fp32")
    return None if ctypes.c_float(s_m).value == 0.0 else (s_m, beta)


class DirectionGuide:
    """The wide pass of one sampling call: the plan of R = (1 or 2) + 2 J row blocks, entered at the first step the directions act on,
    and the launches between its replay and the step.  Row blocks of bs rows: [u, t, e+_1, e-_1, ...] (single branch: [t, e+_1, ...]).
    momentum=(s_m, beta): the combine is slh_eps_direction_momentum on a state this guide owns, zero when the plan is entered; None or
    s_m == 0: slh_eps_direction."""

    def __init__(self, eng, dirs: DirectionSet, coef: Sequence[float], quantile: float, mode: str, bs: int, h: int, w: int, single: bool,
                 ctx: torch.Tensor, pooled: Optional[torch.Tensor], time_ids: Optional[torch.Tensor], start_noise: float,
                 momentum: Optional[Tuple[float, float]] = None):
        self.momentum = check_momentum(momentum)
        self.mom = None
        self.eng, self.dirs, self.coef, self.mode = eng, dirs, [float(c) for c in coef], mode
        self.bs, self.h, self.w, self.single, self.start_noise = bs, h, w, single, float(start_noise)
        self.base = 1 if single else 2                   # row blocks of plain sampling
        self.blocks = self.base + 2 * len(dirs)
        self.chw, self.hw = eng.cfg.out_channels * h * w, h * w
        self.keep = DirectionSet.n_keep(self.hw, quantile)
        self.cond = (ctx, pooled, time_ids)
        self.drv: Optional[Pass] = None
        self.guided = self.thr = None

    def live(self, t) -> bool:
        return not float(t) > self.start_noise

    @property
    def entered(self) -> bool:
        return self.drv is not None

    def enter(self) -> Pass:
        """Build the wide plan and write its conditioning.  Plans share the engine's arena - the plain plan's buffers are dead from
        here on, and so is the plan itself if the arena had to grow - so the caller takes what it needs out of them first."""
        eng, bs = self.eng, self.bs
        ctx, pooled, time_ids = self.cond
        d_ctx, d_pooled = self.dirs.rows(bs, eng.device)
        if (pooled is None) != (d_pooled is None):
            raise ValueError("directions: pooled embeddings on one side only (SDXL needs them for the prompt and for every direction)")
        if time_ids is not None:         # the text block's micro-conditioning for every direction row
            ti = time_ids.to(eng.device, torch.float32).reshape(-1, 6)
            time_ids = torch.cat([ti] + [ti[-bs:]] * (2 * len(self.dirs)))
        self.drv = Pass(eng, eng.plan(self.blocks * bs, self.h, self.w, self.mode))
        self.drv.load_cond(torch.cat([ctx.to(eng.device, torch.bfloat16), d_ctx.to(torch.bfloat16)]),
                           None if pooled is None else torch.cat([pooled.to(eng.device, torch.bfloat16), d_pooled.to(torch.bfloat16)]), time_ids)
        self.guided = torch.empty((bs,) + tuple(self.drv.io["eps"].tensor.shape[1:]), dtype=torch.bfloat16, device=eng.device)
        if self.keep < self.hw:
            self.thr = torch.empty((bs, len(self.dirs), self.chw // self.hw), dtype=torch.int32, device=eng.device)
        if self.momentum is not None:
            self.mom = torch.zeros((bs, self.chw), dtype=torch.float32, device=eng.device)
        return self.drv

    def block(self, name: str, j: int) -> int:
        """device address of row block j of io[name]"""
        b = self.drv.io[name]
        return b.ptr + j * (b.nbytes // self.blocks)

    def guide(self, stream: int) -> int:
        """after the wide replay: the threshold launch (a quantile > 0 only) and the combine (with momentum: which also moves the state)
        -> the address of the guided text row"""
        J = len(self.dirs)
        pos = [self.block("eps", self.base + 2 * k) for k in range(J)]
        neg = [self.block("eps", self.base + 2 * k + 1) for k in range(J)]
        shape = dict(nb=self.bs, chw=self.chw, hw=self.hw)
        if self.thr is not None:
            lib.direction_threshold(stream, pos=pos, neg=neg, thr=self.thr.data_ptr(), n_keep=[self.keep] * J, **shape)
        rows = dict(t=self.block("eps", self.base - 1), out=self.guided.data_ptr(), pos=pos, neg=neg, c=self.coef,
                    thr=0 if self.thr is None else self.thr.data_ptr(), **shape)
        if self.mom is None:
            lib.eps_direction(stream, **rows)
        else:                            # the state is updated in place
            lib.eps_direction_momentum(stream, mom_in=self.mom.data_ptr(), mom_out=self.mom.data_ptr(), s_m=self.momentum[0],
                                       beta=self.momentum[1], **rows)
        return self.guided.data_ptr()

    def spread(self):
        """one copy of the input the step just wrote (row block 0) into the direction rows' blocks"""
        smp, bs = self.drv.io["sample"].tensor, self.bs
        smp[self.base * bs:].view(self.blocks - self.base, bs, *smp.shape[1:]).copy_(smp[:bs])
