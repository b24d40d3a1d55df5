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
from dataclasses import dataclass
from itertools import count
from typing import List, Optional, Sequence, Tuple

import torch

from . import lib
from . import schedulers
from .ddim import DDIMSchedule
from .directions import DirectionGuide, DirectionSet, check_momentum
from .lora_store import LoraStore
from .merge import SliderSet, WeightMerger
from .passes import Pass
from .unet import UNetEngine
from .vae import VaeDecoder


@dataclass
class SampleTrace:
    """What a scale-0 run of the sampling loop leaves (SliderSampler.base_trace): enough to run every other scale of the same seed
    localised to a mask - the chain's latent after every step is what a masked run keeps outside the mask - and to start those runs
    where the slider starts to act.  Tensors live on the engine's device, latents in the loop's dtype: bf16 for ddim, fp32 for
    latents="fp32"."""
    timesteps: List[float]                   # the grid
    x_start: torch.Tensor                    # [bs][4][h][w] the starting latent (noise * init_noise_sigma)
    visited: torch.Tensor                    # [steps][bs][4][h][w] the latent after every step; visited[-1] is the final latent
    final: torch.Tensor                      # what sample_latents(scale=0) returns: bf16
    draws: Optional[torch.Tensor]            # [steps][bs][4][h][w] fp32, the per-call noise of euler_a / ddpm (None elsewhere)
    input0: torch.Tensor                     # the first pass's UNet input (the sigma-space loops scale x_start)
    s_in: Optional[List[float]]              # fp32 loops: s_in[i], i >= 1, scales visited[i - 1] to pass i's input (row i - 1's s_next)
    ctx: torch.Tensor                        # the conditioning and guidance of the run
    pooled: Optional[torch.Tensor]
    time_ids: Optional[torch.Tensor]
    guidance: float
    single: bool                             # one UNet row per image, no guidance
    start_noise: float                       # (sliders= with sliders held at a fixed scale merges them there, at scale 0 too)

    @property
    def steps(self) -> int:
        return len(self.timesteps)

    def unet_input(self, i: int) -> torch.Tensor:
        """what the UNet read at step i of the chain, to the bit once rounded to bf16 (Pass.load_latents)"""
        if i == 0:
            return self.input0
        v = self.visited[i - 1]
        return v if self.s_in is None else (v * self.s_in[i]).to(torch.bfloat16)      # one fp32 product, then rne: slh_sigma_step's copy


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
                       time_ids: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                       trace: Optional[SampleTrace] = None, share_prefix: bool = True, directions: Optional[DirectionSet] = None,
                       direction_quantile: float = 0.0, direction_momentum: Optional[Tuple[float, float]] = None) -> torch.Tensor:
        """ctx: (2*bs, 77, D) = cat([unconditional, text]); noise: (bs, 4, h, w) UNIT noise (it is multiplied by the
        scheduler's init_noise_sigma here, generate_images_sd1.py:165); returns the final latents (bs, 4, h, w) bf16.
        LoRA multiplier per step: 0 while t > start_noise, `scale` after.
        Single branch: a ctx of bs rows (the text prompt alone; pooled and time_ids then have bs rows too) samples without
        classifier-free guidance - one UNet row per image, guidance_scale is not read - as the reference's pipelines do for
        guidance_scale <= 1 (the distilled few-step checkpoints).
        mask ([h][w], [bs][h][w] or [bs][1][h][w], values in [0, 1], 1 = the slider acts): localised sampling (docs/SAMPLING.md).
        After every step with t <= start_noise the latent is blended against the latent the scale-0 chain had after that step
        (trace.visited[i], one slh_latent_blend launch), so where the mask is 0 the result is trace.final bit for bit, at any scale.
        trace: the scale-0 run (base_trace) of this noise, conditioning, grid and guidance; built here if a mask comes without one.
        With a trace the chain starts on trace.x_start and uses its noise draws, not the scheduler generator's next ones.
        share_prefix: ddim, euler, euler_a, ddpm (no multistep history): start at the first step with t <= start_noise from the
        trace's latent instead of replaying the steps every scale shares - the same bits.  ddim and latents="fp32" only.
        directions (sliders_amd/directions.py, docs/SAMPLING.md "Prompt-direction sampling"): prompt pairs that steer the run at `scale`
        the way a slider trained on them would be taught to: on every step with t <= start_noise the pass also carries each pair's
        positive and unconditional prompt (the wide plan, 2 more row blocks per pair), slh_eps_direction adds the scaled differences to
        the text row and the step reads that row.  direction_quantile q in [0, 1): only the largest 1 - q of each latent channel's
        differences act (slh_direction_threshold).  Steps above start_noise, and a call whose coefficients are all zero, run plain
        sampling's launches on the plain plan.  store= / sliders= act on every row of the pass.
        direction_momentum = (s_m, beta): SEGA's momentum on the directions' guidance (slh_eps_direction_momentum; the state is zero at
        the first live step of this call); None or s_m = 0: none, the launches above."""
        eng = self.eng
        bs, _, h, w = noise.shape
        if ctx.shape[0] not in (bs, 2 * bs):
            raise ValueError(f"sample_latents: ctx has {ctx.shape[0]} rows for {bs} noise rows: expected {2 * bs} (the CFG pair) or {bs}")
        single = ctx.shape[0] == bs
        local = {}
        if mask is not None or trace is not None:
            self._check_localised("sample_latents with mask= or trace=")
            if mask is not None:
                from .edit import as_mask          # (edit imports this module)
                mask = as_mask(mask, bs, h, w).to(eng.device)
                if trace is None:
                    trace = self.base_trace(ctx, noise, ddim_steps, guidance_scale, pooled, time_ids, start_noise)
            if trace.steps != ddim_steps or tuple(trace.x_start.shape) != tuple(noise.shape) or trace.single != single:
                raise ValueError(f"sample_latents: the trace has {trace.steps} steps of {tuple(trace.x_start.shape)} latents, "
                                 f"{'single branch' if trace.single else 'CFG pair'}: this call has {ddim_steps} of {tuple(noise.shape)}, "
                                 f"{'single branch' if single else 'CFG pair'}")
            local = dict(mask=mask, trace=trace, start_noise=start_noise, share_prefix=share_prefix)
        mode = "on" if self.store is not None else "off"
        guide = None
        if directions is not None:
            DirectionSet.n_keep(h * w, direction_quantile)          # (an argument error, whether or not the directions act)
            check_momentum(direction_momentum)
            coef = directions.coefficients(scale, guidance_scale, single)
            if any(c != 0.0 for c in coef):
                guide = DirectionGuide(eng, directions, coef, direction_quantile, mode, bs, h, w, single, ctx, pooled, time_ids, start_noise,
                                       momentum=direction_momentum)
        elif direction_momentum is not None:
            raise ValueError("sample_latents: direction_momentum without directions")
        p = eng.plan(ctx.shape[0], h, w, mode)
        drv = Pass(eng, p)
        drv.load_cond(ctx, pooled, time_ids)
        with self.slider_session(scale, start_noise) as gate:
            if self.latents == "fp32":
                return self._sample_fp32(drv, gate, noise, ddim_steps, guidance_scale, single, guide=guide, **local)
            if not self.sched.fused:
                return self._sample_unfused(drv, gate, noise, ddim_steps, guidance_scale, single, guide=guide)
            return self._sample_ddim(drv, gate, noise, ddim_steps, guidance_scale, single, guide=guide, **local)

    @staticmethod
    def _widen(guide: DirectionGuide, latent: torch.Tensor) -> Pass:
        """Crossing start_noise with directions: the latent the next pass reads moves from the plain plan's input buffer into every row
        block of the wide plan's (a copy first: the two plans share the arena)"""
        x = latent.clone()
        drv = guide.enter()
        drv.load_latents(x)
        return drv

    def _check_localised(self, what: str):
        if self.latents != "fp32" and not self.sched.fused:
            raise ValueError(f"{what}: the bf16 tensor-op path of scheduler {type(self.sched).__name__} keeps no trace; use "
                             "latents='fp32' (--fp32_latents) or ddim")

    @torch.no_grad()
    def base_trace(self, ctx: torch.Tensor, noise: torch.Tensor, ddim_steps: int = 50, guidance_scale: float = 7.5,
                   pooled: Optional[torch.Tensor] = None, time_ids: Optional[torch.Tensor] = None, start_noise: int = 750) -> SampleTrace:
        """The loop sample_latents runs at scale 0 - the same launches on the same inputs, the scheduler generator advanced as one call
        advances it - with the latent after every step kept: trace.final is what sample_latents(scale=0) returns, bit for bit.
        start_noise matters only to sliders= with sliders held at a fixed scale (merged below it at scale 0 too)."""
        self._check_localised("base_trace")
        eng = self.eng
        bs, _, h, w = noise.shape
        if ctx.shape[0] not in (bs, 2 * bs):
            raise ValueError(f"base_trace: ctx has {ctx.shape[0]} rows for {bs} noise rows: expected {2 * bs} (the CFG pair) or {bs}")
        single = ctx.shape[0] == bs
        drv = Pass(eng, eng.plan(ctx.shape[0], h, w, "on" if self.store is not None else "off"))
        drv.load_cond(ctx, pooled, time_ids)
        rec = {}
        with self.slider_session(0.0, start_noise) as gate:
            loop = self._sample_fp32 if self.latents == "fp32" else self._sample_ddim
            final = loop(drv, gate, noise, ddim_steps, guidance_scale, single, record=rec)
        keep = lambda v: None if v is None else v.detach().clone()
        return SampleTrace(final=final, ctx=keep(ctx), pooled=keep(pooled), time_ids=keep(time_ids), guidance=float(guidance_scale),
                           single=single, start_noise=float(start_noise), **rec)

    @staticmethod
    def _first_live(ts: Sequence[float], start_noise: float) -> int:
        """index of the first step of the grid at which the slider acts (t <= start_noise); len(ts) if there is none"""
        return next((i for i, t in enumerate(ts) if not float(t) > start_noise), len(ts))

    def _sample_ddim(self, drv: Pass, gate, noise, steps, guidance_scale, single=False, mask=None, trace=None, start_noise=750,
                     share_prefix=True, record=None, guide=None):
        """The fused DDIM loop: per step slider gate -> UNet replay -> slh_cfg_ddim in place on io["sample"] (both halves for the pair).
        record (a dict): the scale-0 run's SampleTrace fields are left there.  trace: start on its latent - at the first live step if
        share_prefix - and, with a mask, blend io["sample"] in place against trace.visited[i] after every live step.
        guide (DirectionGuide): from the first step with t <= start_noise on, the wide plan; the step reads the guided text row and one
        copy spreads its result over the direction rows' blocks."""
        eng, io, smp = self.eng, drv.io, drv.io["sample"]
        bs, _, h, w = noise.shape
        s = torch.cuda.current_stream().cuda_stream
        chw = eng.cfg.out_channels * h * w
        half = bs * chw * 2
        # single branch: the text half is read from the one epsilon there is and the guidance passed is 0 (guidance_scale is not
        # read), so the combine u + 0 * (u - u) hands the step u itself
        # with directions both read the guided row `text` where the text row was read
        pair = lambda text: ({"eps": text or io["eps"].ptr, "out2": 0, "eps_text": text or io["eps"].ptr, "guidance": 0.0} if single
                             else {"eps": io["eps"].ptr, "out2": smp.ptr + half, "eps_text": text, "guidance": float(guidance_scale)})
        ts = self.sched.make_timesteps(steps)
        i0 = self._first_live(ts, start_noise) if trace is not None and share_prefix else 0
        if i0 == len(ts):            # the slider never acts: the base chain itself
            return trace.final.clone()
        start = noise if trace is None else trace.x_start if i0 == 0 else trace.visited[i0 - 1]
        drv.load_latents(start)
        if record is not None:
            record.update(timesteps=[float(t) for t in ts], x_start=smp.tensor[:bs].clone(), draws=None, s_in=None,
                          visited=torch.empty((steps,) + tuple(noise.shape), dtype=torch.bfloat16, device=eng.device))
            record["input0"] = record["x_start"]
        for i in range(i0, steps):
            t, first = ts[i], i == i0
            wide = guide is not None and guide.live(t)
            if wide and not guide.entered:
                drv, first = self._widen(guide, smp.tensor[:bs]), True
                io, smp = drv.io, drv.io["sample"]
            drv.run(t, gate(t, first), s)
            d = lib.CfgDdimDesc(x=smp.ptr, out=smp.ptr, nb=bs, chw=chw, **pair(guide.guide(s) if wide else 0),
                                **self.sched.step_fields(t, steps))
            lib.call(lib.OP_CFG_DDIM, d, s)
            if mask is not None and not float(t) > start_noise:
                lib.latent_blend(s, e=smp.ptr, keep=trace.visited[i].data_ptr(), mask=mask.data_ptr(), out=smp.ptr, nb=bs, chw=chw,
                                 hw=h * w, fp32=False, in_bf16=0 if single else smp.ptr + half)
            if wide:
                guide.spread()
            if record is not None:
                record["visited"][i].copy_(smp.tensor[:bs])
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

    def _sample_unfused(self, drv: Pass, gate, noise, steps, guidance_scale, single=False, guide=None):
        """generate_images_sd1.py:160-185 with a tensor-op scheduler: schedulers.denoise over the whole grid (scale_model_input ->
        prediction -> scheduler.step on the device latents), the prediction being slider gate -> UNet replay -> guidance combine
        (slh_cfg_ddim, do_step = 0).  single: one epsilon row per sample and nothing to combine; the step reads the plan's epsilon as
        it is (it returns new tensors, so the next replay may overwrite it).  guide (DirectionGuide): from the first step with
        t <= start_noise on the pass is the wide plan's and the prediction reads the guided text row - for the single branch it is that
        row"""
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
            nonlocal drv
            first = next(step) == 0
            wide = guide is not None and guide.live(t)
            if wide and not guide.entered:
                drv, first = guide.enter(), True
            drv.load_latents(x)
            drv.run(t, gate(t, first), s)
            if wide:
                combine.eps, combine.eps_text = drv.io["eps"].ptr, guide.guide(s)
                if single:
                    return guide.guided.view_as(lat)
            if not single:
                lib.call(lib.OP_CFG_DDIM, combine, s)
            return eps

        return schedulers.denoise(sch, predict, lat, steps, steps, generator=self.sched_generator, device=eng.device)

    def _sample_fp32(self, drv: Pass, gate, noise, steps, guidance_scale, single=False, mask=None, trace=None, start_noise=750,
                     share_prefix=True, record=None, guide=None):
        """The same loop on an fp32 master latent: per step slider gate -> UNet replay -> ONE slh_sigma_step launch (the row of
        schedulers.step_row), which does the guidance combine and the scheduler's step in fp32, keeps the multistep history (a ring of
        min(order, steps) - 1 fp32 buffers owned by this call) and writes the next pass's scaled input into io["sample"], both halves
        for the pair.  The first scaled input is written ahead of the loop; inside it Pass.load_latents is not called.  euler_a / ddpm:
        the noise of all steps is one fp32 draw from sched_generator per call - seed-deterministic, and deliberately not the bf16
        path's draws (those are bf16 tensors drawn step by step).  Returns the bf16 rounding of the final latent.
        record / trace / mask: as _sample_ddim; the draws are the trace's, the blend is on the master latent and rewrites the scaled
        input with the row's s_next.  A scheduler with a multistep history (lms, dpmpp_2m) runs the whole grid.
        guide (DirectionGuide): as _sample_ddim; the scaled input written for the first live step moves to the wide plan's buffer, and the
        step writes the following ones there."""
        eng, sch, io = self.eng, self.sched, drv.io
        bs = noise.shape[0]
        chw = noise[0].numel()
        hw = noise.shape[2] * noise.shape[3]
        s = torch.cuda.current_stream().cuda_stream
        sch.set_timesteps(steps, device=eng.device)        # init_noise_sigma is the grid's
        rows = [schedulers.step_row(sch, i, steps) for i in range(steps)]
        ts = sch.timesteps.tolist()
        depth = schedulers.history_depth(sch, steps)
        i0 = self._first_live(ts, start_noise) if trace is not None and share_prefix and depth == 0 else 0
        if i0 == steps:              # the slider never acts: the base chain itself
            return trace.final.clone()
        if trace is None:
            x = (noise.to(eng.device, torch.float32) * sch.init_noise_sigma).contiguous()
            draws = (torch.randn((steps,) + tuple(x.shape), generator=self.sched_generator, device=eng.device, dtype=torch.float32)
                     if any(r.c_n != 0.0 for r in rows) else None)
            first_input = sch.scale_model_input(x, sch.timesteps[0])
        else:
            x = (trace.x_start if i0 == 0 else trace.visited[i0 - 1]).clone()
            draws, first_input = trace.draws, trace.unet_input(i0)
        ring = [torch.empty_like(x) for _ in range(depth)]
        smp = io["sample"]
        drv.load_latents(first_input)
        if record is not None:
            record.update(timesteps=ts, x_start=x.clone(), draws=draws, input0=first_input.clone(), s_in=[1.0] + [r.s_next for r in rows[:-1]],
                          visited=torch.empty((steps,) + tuple(x.shape), dtype=torch.float32, device=eng.device))
        in2 = 0 if single else smp.ptr + bs * chw * 2
        for i in range(i0, steps):
            t, r, first = ts[i], rows[i], i == i0
            wide = guide is not None and guide.live(t)
            if wide and not guide.entered:
                drv, first = self._widen(guide, smp.tensor[:bs]), True
                io, smp = drv.io, drv.io["sample"]
                in2 = 0 if single else smp.ptr + bs * chw * 2
            drv.run(t, gate(t, first), s)
            text = guide.guide(s) if wide else 0          # the guided text row: the single branch's only row
            lib.sigma_step(s, eps=text if wide and single else io["eps"].ptr, eps_text=0 if single else text, x=x.data_ptr(),
                           out=x.data_ptr(), nb=bs, chw=chw, kind=r.kind, p=r.p, q=r.q,
                           sigma=r.sigma, a=r.a, c=r.c, c_n=r.c_n, s_next=r.s_next, guidance=float(guidance_scale), single=single,
                           hist=[ring[(i - k) % len(ring)].data_ptr() for k in range(1, r.n_hist + 1)],
                           noise=draws[i].data_ptr() if draws is not None and r.c_n != 0.0 else 0,
                           hist_out=ring[i % len(ring)].data_ptr() if ring else 0,
                           in_bf16=smp.ptr, in2_bf16=in2)
            if mask is not None and not float(t) > start_noise:
                lib.latent_blend(s, e=x.data_ptr(), keep=trace.visited[i].data_ptr(), mask=mask.data_ptr(), out=x.data_ptr(), nb=bs,
                                 chw=chw, hw=hw, fp32=True, s_next=r.s_next, in_bf16=smp.ptr, in2_bf16=in2)
            if wide:
                guide.spread()
            if record is not None:
                record["visited"][i].copy_(x)
        return x.to(torch.bfloat16)

    # -----------------------------------------------------------------------------------------------------------------------------
    # where the slider acts / where a word lives, over a source: anything with .timesteps, .unet_input(i), .ctx / .pooled / .time_ids and
    # .guidance - a SampleTrace here, an inversion's NoiseSpace in SliderEditor (sliders_amd/edit.py, which documents both maps)
    # -----------------------------------------------------------------------------------------------------------------------------
    def _source_pass(self, src, attn_maps=None) -> Pass:
        """the plan of the source's shape with its conditioning written; attn_maps: the plan of the shape that also records attention
        maps (UNetEngine.plan)"""
        _, _, h, w = src.unet_input(0).shape
        drv = Pass(self.eng, self.eng.plan(src.ctx.shape[0], h, w, "on" if self.store is not None else "off", attn_maps=attn_maps))
        drv.load_cond(src.ctx, src.pooled, src.time_ids)
        return drv

    def _footprint(self, src, scale: float, start_noise, draws: int, t_min: int, directions: Optional[DirectionSet] = None,
                   direction_quantile: float = 0.0, guidance: Optional[float] = None) -> torch.Tensor:
        from .edit import footprint_draws, footprint_mean          # (edit imports this module)
        ts = src.timesteps
        idx = footprint_draws(ts, start_noise, draws, t_min)
        dev = self.eng.device
        bs, ch, h, w = src.unet_input(0).shape
        if directions is not None:
            return footprint_mean(self._direction_footprint(src, idx, scale, start_noise, directions, direction_quantile,
                                                            src.guidance if guidance is None else guidance))
        drv = self._source_pass(src)
        io = drv.io
        single = src.ctx.shape[0] == bs          # one epsilon row per sample: both "halves" are it and the guidance is not read
        off = torch.empty((len(idx),) + tuple(io["eps"].tensor.shape), dtype=torch.bfloat16, device=dev)
        A = torch.empty((len(idx), bs, h, w), dtype=torch.float32, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        with self.slider_session(scale, start_noise, zero_merges=False) as gate:
            def unet(n, i, multiplier):
                """pass n of this call at step i of the grid; n and the multiplier choose the program as in the chain"""
                drv.load_latents(src.unet_input(i))
                drv.run(ts[i], gate(ts[i], n == 0, multiplier), s)

            for j, i in enumerate(idx):
                unet(j, i, 0.0)
                off[j].copy_(io["eps"].tensor)
            for j, i in enumerate(idx):
                unet(len(idx) + j, i, scale)
                halves = dict(eps_a_text=io["eps"].ptr, eps_b_text=off[j].data_ptr()) if single else {}
                d = lib.EpsAbsdiffDesc(eps_a=io["eps"].ptr, eps_b=off[j].data_ptr(), out=A[j].data_ptr(), nb=bs, chw=ch * h * w, hw=h * w,
                                       guidance=0.0 if single else float(src.guidance), **halves)
                lib.call(lib.OP_EPS_ABSDIFF, d, s)
        return footprint_mean(A)

    def _direction_footprint(self, src, idx, scale: float, start_noise, directions: DirectionSet, quantile: float, guidance: float) -> torch.Tensor:
        """A [len(idx)][bs][h][w]: per draw ONE wide pass (the rows of a direction step at this scale and guidance), the guided text row
        t' of DirectionGuide.guide, and slh_eps_absdiff of the pair (u, t') against the pair (u, t) - sum_c |g (t' - t)|, what the step
        would see differently.  No momentum: a draw is not a chain."""
        eng, ts = self.eng, src.timesteps
        bs, ch, h, w = src.unet_input(0).shape
        single = src.ctx.shape[0] == bs
        DirectionSet.n_keep(h * w, quantile)
        guide = DirectionGuide(eng, directions, directions.coefficients(scale, guidance, single), quantile,
                               "on" if self.store is not None else "off", bs, h, w, single, src.ctx, src.pooled, src.time_ids, start_noise)
        drv = guide.enter()
        A = torch.empty((len(idx), bs, h, w), dtype=torch.float32, device=eng.device)
        s = torch.cuda.current_stream().cuda_stream
        with self.slider_session(scale, start_noise, zero_merges=False) as gate:
            for n, i in enumerate(idx):
                drv.load_latents(src.unet_input(i))
                drv.run(ts[i], gate(ts[i], n == 0, scale), s)
                guided, text = guide.guide(s), guide.block("eps", guide.base - 1)
                u = text if single else drv.io["eps"].ptr          # single branch: both "halves" are the one row, the guidance is not read
                d = lib.EpsAbsdiffDesc(eps_a=guided if single else u, eps_a_text=guided, eps_b=u, eps_b_text=text, out=A[n].data_ptr(), nb=bs,
                                       chw=ch * h * w, hw=h * w, guidance=0.0 if single else float(guidance))
                lib.call(lib.OP_EPS_ABSDIFF, d, s)
        return A

    def _word_map(self, src, tokens, weights, draws: int, max_factor: int) -> torch.Tensor:
        from .edit import footprint_draws, key_weights, level_mean
        ts = src.timesteps
        idx = footprint_draws(ts, ts[0], draws, 0)
        eng, dev = self.eng, self.eng.device
        bs, _, h, w = src.unet_input(0).shape
        wt = key_weights(bs, eng.ctx_len, tokens, weights)
        drv = self._source_pass(src, attn_maps={"max_factor": int(max_factor)})
        io = drv.io
        io["xattn_wt"].tensor.copy_(wt)
        levels = {int(k.split(".")[1]): b for k, b in io.items() if k.startswith("xattn_map.")}
        s = torch.cuda.current_stream().cuda_stream
        total = torch.zeros((bs, h, w), dtype=torch.float32, device=dev)
        with self.slider_session(0.0, -1, zero_merges=False) as gate:
            for n, i in enumerate(idx):
                drv.load_latents(src.unet_input(i))
                drv.run(ts[i], gate(ts[i], n == 0), s)
                total += level_mean({f: b.tensor for f, b in levels.items()}, h, w)
        return total / float(len(idx))

    @torch.no_grad()
    def footprint(self, trace: SampleTrace, scale: float, start_noise: int = 750, draws: int = 8, t_min: int = 200,
                  directions: Optional[DirectionSet] = None, direction_quantile: float = 0.0, guidance_scale: Optional[float] = None) -> torch.Tensor:
        """Where the slider acts on the image of this trace: SliderEditor.footprint's map F [bs][h][w] (slh_eps_absdiff between the slider
        at `scale` and the slider off, over `draws` noise levels with t_min <= t <= start_noise), with the scale-0 chain's own UNet
        inputs, conditioning and guidance in place of an inversion's.  edit.footprint_mask turns it into a mask.
        directions: where the prompt directions act instead (SliderEditor.footprint), len(draws) wide passes."""
        self._check_localised("footprint")
        return self._footprint(trace, scale, start_noise, draws, t_min, directions, direction_quantile, guidance_scale)

    @torch.no_grad()
    def word_map(self, trace: SampleTrace, tokens: Optional[Sequence[int]] = None, weights: Optional[torch.Tensor] = None, draws: int = 8,
                 max_factor: int = 4) -> torch.Tensor:
        """Where words of the prompt live on the image of this trace: SliderEditor.word_map's map F [bs][h][w] (slh_xattn_map, the slider
        off) over `draws` steps of the scale-0 chain.  The maps are those of the text half of a CFG pair: a single-branch trace is
        refused by the plan.  edit.word_mask turns it into a mask."""
        self._check_localised("word_map")
        return self._word_map(trace, tokens, weights, draws, max_factor)

    @torch.no_grad()
    def generate(self, ctx, noise, **kw) -> torch.Tensor:
        """-> uint8 images [bs][H][W][3] (needs a VaeDecoder)."""
        if self.decoder is None:
            raise RuntimeError("SliderSampler.generate needs a VaeDecoder")
        lat = self.sample_latents(ctx, noise, **kw)
        return VaeDecoder.to_uint8(self.decoder.decode(lat))
