"""Slider inference on the MI355X engine: the sampling loop the reference's consumers run over a trained slider
(eval-scripts/generate_images_sd1.py:136-171, trainscripts/textsliders/generate_images_xl.py:39-394, the inference
notebooks):

    latents = randn(seed) * init_noise_sigma
    for t in scheduler.timesteps (DDIM, `ddim_steps`):
        network.set_lora_slider(scale = 0 if t > start_noise else scale)
        with network: eps = unet(cat([latents] * 2), t, cat([uncond, text]) [, added_cond_kwargs])
        eps = eps_uncond + guidance_scale * (eps_text - eps_uncond)
        latents = scheduler.step(eps, t, latents).prev_sample
    image = vae.decode(latents / scaling_factor); image = (image / 2 + 0.5).clamp(0, 1)

Every UNet evaluation is one replay of the engine's LoRA-on command buffer (the adapter scale is a device scalar, so
gating it per step costs nothing); CFG combine + DDIM step is the fused slh_cfg_ddim kernel; the VAE decoder is the fp32
command buffer of sliders_amd/vae.py.  This is what lets a slider trained here be evaluated here (CLIP-score direction,
eval-scripts/clip_score.py) without the diffusers pipelines.
"""
from __future__ import annotations

from contextlib import contextmanager
from itertools import count
from typing import Optional

import torch

from . import lib
from . import schedulers
from .ddim import DDIMSchedule
from .lora_store import LoraStore
from .merge import SliderSet, WeightMerger
from .passes import Pass
from .unet import UNetEngine
from .vae import VaeDecoder


class SliderSampler:
    def __init__(self, engine: UNetEngine, store: Optional[LoraStore] = None, decoder: Optional[VaeDecoder] = None,
                 prediction_type: str = "epsilon", scheduler: str = "ddim", scheduler_seed: int = 0,
                 sliders: Optional[SliderSet] = None, timestep_spacing: Optional[str] = None, latents: Optional[str] = None):
        """sliders: several sliders of any rank, folded into the frozen weights (sliders_amd/merge.py) instead of the fused rank-4
        adapter path of `store`: the loop samples on the base weights while t > start_noise, merges once when it crosses
        start_noise, runs the adapter-free program on the merged weights and restores the original bits when the image is done.
        scheduler: "ddim" (fused HIP step), "lms" (what eval-scripts/generate_images_sd1.py:51 and the SD-1 notebook
        construct), "euler" (the SDXL checkpoints' scheduler_config: what generate_images_xl.py's pipeline runs), "euler_a",
        "ddpm" - the non-DDIM ones from sliders_amd/schedulers.py - and "dpmpp_2m" (DPM-Solver++ 2M; not one of the reference's).
        timestep_spacing (euler, euler_a and dpmpp_2m only; None: each scheduler's default): "leading" / "linspace", and for euler_a
        and dpmpp_2m "trailing", the few-step grid of the distilled checkpoints (demo_SDXL_Turbo.ipynb: 1-4 steps of euler_a, no CFG;
        docs/SAMPLING.md).
        latents: "bf16" (the default): the latent between two passes is a bf16 tensor and the tensor-op scheduler steps it; "fp32"
        (euler, euler_a, lms, ddpm): an fp32 master latent stepped by one slh_sigma_step launch per pass (_sample_fp32).
        scheduler "dpmpp_2m" (DPM-Solver++ 2M) exists in the fp32 form only, so fp32 is its default."""
        self.eng, self.store, self.decoder = engine, store, decoder
        key = scheduler.lower().replace(" ", "_")
        spacing = {} if timestep_spacing is None else {"timestep_spacing": timestep_spacing}
        if spacing and key not in ("euler", "euler_a", "dpmpp_2m"):
            raise ValueError(f"SliderSampler: timestep_spacing applies to the schedulers euler, euler_a and dpmpp_2m, not {scheduler!r}")
        if latents is None:
            latents = "fp32" if key == "dpmpp_2m" else "bf16"
        if latents not in ("bf16", "fp32"):
            raise ValueError(f"SliderSampler: latents {latents!r}: bf16 and fp32 are implemented")
        if latents == "fp32" and key == "ddim":
            raise ValueError("SliderSampler: latents='fp32' does not apply to ddim: the fused DDIM step (slh_cfg_ddim) has its own rounding "
                             "contract, the reference's bf16 tensor ops")
        if latents == "bf16" and key == "dpmpp_2m":
            raise ValueError("SliderSampler: dpmpp_2m exists only with latents='fp32' (the fused fp32 step)")
        self.latents = latents
        if sliders is not None and store is not None:
            raise ValueError("SliderSampler: give either store= (one rank-4 slider, fused adapters) or sliders= (merged weights)")
        self.merger = WeightMerger(engine.weights, sliders) if sliders is not None else None
        if store is not None and engine.lora is not store:
            engine.attach_lora(store)
        if key == "ddim":
            self.sched = DDIMSchedule(prediction_type=prediction_type)
        elif key == "euler":     # the SDXL checkpoints' own scheduler (generate_images_xl.py pipelines)
            self.sched = schedulers.EulerDiscreteScheduler(prediction_type=prediction_type, **spacing)
            self.sched_generator = None
        elif key == "dpmpp_2m":
            self.sched = schedulers.DPMSolverPP2MScheduler(prediction_type=prediction_type, **spacing)
            self.sched_generator = None
        else:
            self.sched = (schedulers.EulerAncestralDiscreteScheduler(prediction_type=prediction_type, **spacing) if spacing
                          else schedulers.create(scheduler, prediction_type))
            self.sched_generator = torch.Generator(device=engine.device)
            self.sched_generator.manual_seed(int(scheduler_seed))

    @torch.no_grad()
    def sample_latents(self, ctx: torch.Tensor, noise: torch.Tensor, scale: float = 0.0, start_noise: int = 750,
                       ddim_steps: int = 50, guidance_scale: float = 7.5, pooled: Optional[torch.Tensor] = None,
                       time_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ctx: (2*bs, 77, D) = cat([unconditional, text]); noise: (bs, 4, h, w) UNIT noise (it is multiplied by the
        scheduler's init_noise_sigma here, generate_images_sd1.py:165); returns the final latents (bs, 4, h, w) bf16.
        LoRA multiplier per step: 0 while t > start_noise, `scale` after.
        Single branch: a ctx of bs rows (the text prompt alone; pooled and time_ids then have bs rows too) samples without
        classifier-free guidance - one UNet row per image, guidance_scale is not read - as the reference's pipelines do for
        guidance_scale <= 1 (the distilled few-step checkpoints)."""
        eng = self.eng
        bs, _, h, w = noise.shape
        if ctx.shape[0] not in (bs, 2 * bs):
            raise ValueError(f"sample_latents: ctx has {ctx.shape[0]} rows for {bs} noise rows: expected {2 * bs} (the CFG pair) or {bs}")
        single = ctx.shape[0] == bs
        p = eng.plan(ctx.shape[0], h, w, "on" if self.store is not None else "off")
        drv = Pass(eng, p)
        drv.load_cond(ctx, pooled, time_ids)
        with self.slider_session(scale, start_noise) as gate:
            if self.latents == "fp32":
                return self._sample_fp32(drv, gate, noise, ddim_steps, guidance_scale, single)
            if not self.sched.fused:
                return self._sample_unfused(drv, gate, noise, ddim_steps, guidance_scale, single)
            io, smp = p.io, p.io["sample"]
            drv.load_latents(noise)
            s = torch.cuda.current_stream().cuda_stream
            chw = eng.cfg.out_channels * h * w
            half = bs * chw * 2
            # single branch: the text half is read from the one epsilon there is and the guidance passed is 0 (guidance_scale is not
            # read), so the combine u + 0 * (u - u) hands the step u itself
            pair = ({"out2": 0, "eps_text": io["eps"].ptr, "guidance": 0.0} if single
                    else {"out2": smp.ptr + half, "guidance": float(guidance_scale)})
            for i, t in enumerate(self.sched.make_timesteps(ddim_steps)):
                drv.run(t, gate(t, i == 0), s)
                d = lib.CfgDdimDesc(eps=io["eps"].ptr, x=smp.ptr, out=smp.ptr, nb=bs, chw=chw, **pair,
                                    **self.sched.step_fields(t, ddim_steps))
                lib.call(lib.OP_CFG_DDIM, d, s)
            return smp.tensor[:bs].clone()

    @contextmanager
    def slider_session(self, scale: float = 0.0, start_noise: float = 750, zero_merges: bool = True):
        """The slider over the passes of one call.  Yields gate(t, first, multiplier = scale) -> first, to be called in front of every
        pass: the slider acts at `multiplier` once t <= start_noise.  store=: the adapter multiplier of this pass (0 above start_noise).
        sliders=: the merge when the loop crosses start_noise (all-zero scales: nothing to merge, the weights stay), which makes this
        pass a first one - the cross-attention K/V a text-cached program reuses were projected with the weights of the pass before.
        zero_merges = False (the editor): a multiplier of 0 is the inversion's pass and merges nothing, sliders held at a fixed scale
        included.  However the body ends, merged weights are restored and the adapter is switched off."""
        eng, m = self.eng, self.merger

        def gate(t, first: bool, multiplier: Optional[float] = None) -> bool:
            mult = float(scale if multiplier is None else multiplier)
            live = not float(t) > start_noise
            if self.store is not None:
                eng.set_lora(True, mult if live else 0.0)
            if m is not None and not m.merged and live and (zero_merges or mult != 0.0):
                scales = m.sliders.scales(mult)
                if any(v != 0.0 for v in scales):
                    m.merge(scales)
                    return True
            return first

        try:
            yield gate
        finally:
            if m is not None and m.merged:
                m.restore()
            if self.store is not None:
                eng.set_lora(False)

    def _sample_unfused(self, drv: Pass, gate, noise, steps, guidance_scale, single=False):
        """generate_images_sd1.py:160-185 with a tensor-op scheduler: schedulers.denoise over the whole grid (scale_model_input ->
        prediction -> scheduler.step on the device latents), the prediction being slider gate -> UNet replay -> guidance combine
        (slh_cfg_ddim, do_step = 0).  single: one epsilon row per sample and nothing to combine; the step reads the plan's epsilon as
        it is (it returns new tensors, so the next replay may overwrite it)"""
        eng, sch, io = self.eng, self.sched, drv.io
        bs = noise.shape[0]
        s = torch.cuda.current_stream().cuda_stream
        sch.set_timesteps(steps, device=eng.device)        # init_noise_sigma is the grid's
        lat = (noise.to(eng.device, torch.float32) * sch.init_noise_sigma).to(torch.bfloat16)
        eps = io["eps"].tensor.view_as(lat) if single else torch.empty_like(lat)
        combine = lib.CfgDdimDesc(eps=io["eps"].ptr, x=0, out=eps.data_ptr(), out2=0, nb=bs, chw=lat[0].numel(),
                                  guidance=float(guidance_scale), do_step=0)
        step = count()

        def predict(x, t):
            drv.load_latents(x)
            drv.run(t, gate(t, next(step) == 0), s)
            if not single:
                lib.call(lib.OP_CFG_DDIM, combine, s)
            return eps

        return schedulers.denoise(sch, predict, lat, steps, steps, generator=self.sched_generator, device=eng.device)

    def _sample_fp32(self, drv: Pass, gate, noise, steps, guidance_scale, single=False):
        """The same loop on an fp32 master latent: per step slider gate -> UNet replay -> ONE slh_sigma_step launch (the row of
        schedulers.step_row), which does the guidance combine and the scheduler's step in fp32, keeps the multistep history (a ring of
        min(order, steps) - 1 fp32 buffers owned by this call) and writes the next pass's scaled input into io["sample"], both halves
        for the pair.  The first scaled input is written ahead of the loop; inside it Pass.load_latents is not called.  euler_a / ddpm:
        the noise of all steps is one fp32 draw from sched_generator per call - seed-deterministic, and deliberately not the bf16
        path's draws (those are bf16 tensors drawn step by step).  Returns the bf16 rounding of the final latent."""
        eng, sch, io = self.eng, self.sched, drv.io
        bs = noise.shape[0]
        chw = noise[0].numel()
        s = torch.cuda.current_stream().cuda_stream
        sch.set_timesteps(steps, device=eng.device)        # init_noise_sigma is the grid's
        rows = [schedulers.step_row(sch, i, steps) for i in range(steps)]
        x = (noise.to(eng.device, torch.float32) * sch.init_noise_sigma).contiguous()
        ring = [torch.empty_like(x) for _ in range(schedulers.history_depth(sch, steps))]
        draws = (torch.randn((steps,) + tuple(x.shape), generator=self.sched_generator, device=eng.device, dtype=torch.float32)
                 if any(r.c_n != 0.0 for r in rows) else None)
        smp = io["sample"]
        drv.load_latents(sch.scale_model_input(x, sch.timesteps[0]))
        for i, (t, r) in enumerate(zip(sch.timesteps.tolist(), rows)):
            drv.run(t, gate(t, i == 0), s)
            lib.sigma_step(s, eps=io["eps"].ptr, x=x.data_ptr(), out=x.data_ptr(), nb=bs, chw=chw, kind=r.kind, p=r.p, q=r.q,
                           sigma=r.sigma, a=r.a, c=r.c, c_n=r.c_n, s_next=r.s_next, guidance=float(guidance_scale), single=single,
                           hist=[ring[(i - k) % len(ring)].data_ptr() for k in range(1, r.n_hist + 1)],
                           noise=draws[i].data_ptr() if draws is not None and r.c_n != 0.0 else 0,
                           hist_out=ring[i % len(ring)].data_ptr() if ring else 0,
                           in_bf16=smp.ptr, in2_bf16=0 if single else smp.ptr + bs * chw * 2)
        return x.to(torch.bfloat16)

    @torch.no_grad()
    def generate(self, ctx, noise, **kw) -> torch.Tensor:
        """-> uint8 images [bs][H][W][3] (needs a VaeDecoder)."""
        if self.decoder is None:
            raise RuntimeError("SliderSampler.generate needs a VaeDecoder")
        lat = self.sample_latents(ctx, noise, **kw)
        return VaeDecoder.to_uint8(self.decoder.decode(lat))
