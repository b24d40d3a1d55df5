"""One UNet pass on a UNetPlan, driven from the host: write the conditioning, write the latents, choose the program, run it.

Every loop of the package (SliderSampler, SliderEditor, SliderTrainer, ImageSliderTrainer, UNetEngine.__call__) drives its passes
through a `Pass`; what a loop adds is what follows the pass - its combine / step launch - and, for the samplers, the slider gate in
front of it (SliderSampler.slider_session).  A new step form plugs in here once.
"""
from __future__ import annotations

from typing import Optional

import torch


def default_time_ids(h: int, w: int, rows: int) -> torch.Tensor:
    """SDXL micro-conditioning of an uncropped h x w latent: [orig_h, orig_w, crop_top, crop_left, target_h, target_w] in pixels
    (train_util.py:298-333), fp32 (rows, 6) on the host"""
    return torch.tensor([[h * 8.0, w * 8.0, 0.0, 0.0, h * 8.0, w * 8.0]] * rows)


class Pass:
    """The inputs and the two programs of one plan.  eng: what owns the plan (cfg.is_xl, cfg.pooled_dim, device)."""

    def __init__(self, eng, p):
        self.eng, self.p, self.io = eng, p, p.io

    def load_cond(self, ctx: torch.Tensor, pooled: Optional[torch.Tensor] = None, time_ids: Optional[torch.Tensor] = None):
        """ctx (rows, 77, D) -> io["ctx"] (bf16); SDXL: time_ids (anything of rows * 6 numbers; None: default_time_ids) -> io["time_ids"],
        pooled (rows, P) -> the first pooled_dim columns of io["add_in"].  Casts of tensors that already have the buffer's dtype on the
        device are no-ops, so a caller that keeps its conditioning there pays the copies alone."""
        p, io, cfg = self.p, self.io, self.eng.cfg
        io["ctx"].tensor.copy_(ctx.to(torch.bfloat16))
        if cfg.is_xl:
            if time_ids is None:
                time_ids = default_time_ids(p.H, p.W, p.B)
            io["time_ids"].tensor.copy_(time_ids.to(device=self.eng.device, dtype=torch.float32).reshape(p.B, 6))
            io["add_in"].tensor[:, : cfg.pooled_dim].copy_(pooled.to(torch.bfloat16))

    def load_latents(self, x: torch.Tensor):
        """x (bs, C, h, w) -> every block of bs rows of io["sample"], as its bf16 rounding: the single branch (one block), the CFG pair
        (two), the de-duplicated frozen pass (three)"""
        smp = self.io["sample"].tensor
        bs = x.shape[0]
        xb = x.to(device=smp.device, dtype=torch.bfloat16)
        for r in range(0, smp.shape[0], bs):
            smp[r:r + bs].copy_(xb)

    def program(self, first: bool):
        """The full pass, or - when the conditioning and the weights are those of the pass before (first = False) and the plan has one -
        the program that skips the text projections: the cross-attention K/V are already there"""
        p = self.p
        return p.prog if first or p.prog_text_cached is None else p.prog_text_cached

    def run(self, t, first: bool, stream: int):
        self.io["t"].tensor.fill_(float(t))
        self.program(first).run(stream)
