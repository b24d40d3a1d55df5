"""Edit a GIVEN image with a trained slider: the edit-friendly DDPM noise space (Huberman-Spiegelglas, Kulikov, Michaeli, CVPR 2024)
in residual form, on the MI355X engine.  docs/EDIT.md has the method, the reason for the residual form and the error bounds.

    python -m sliders_amd.edit --model sdxl --model_path DIR --image photo.png --prompt "photo of a person" \
        --lora_weight models/age_alpha1.0_rank4_noxattn_last.pt --scales=-2,-1,0,1,2 --out edited/ [--synthetic]

Grid: ts = DDIMSchedule.make_timesteps(steps)[skip:] - the sampler's DDIM grid without its `skip` noisiest steps.  Per step, with
the DDIM mean mu(x_t) of x_{t-1} (eta in [0, 1] sets how much of the step the residual carries instead of the predicted noise):

    invert (once per image, slider multiplier 0):  X_i = sqrt(a_i) x0 + sqrt(1 - a_i) e_i   independent e_i ~ N(0, I)
        x <- X_0;  per step  d_i = X_{i+1} - mu(x)  (x0 after the last step),  x <- mu(x) + d_i
    edit (slider scale s below start_noise):       x <- X_0;  per step  x <- mu'(x) + d_i

x <- mu + d_i (recomputed, never the target itself) makes the reconstruction an identity of the arithmetic, not of the network: an
edit at scale 0 runs the programs the inversion ran on the inputs the inversion had, so it reads the same epsilon, forms the same mu
and adds the same d_i - the same bits.  The latent master is fp32 (slh_ddpm_edit_step, csrc/edit.hip); only the UNet input is its
bf16 rounding.

`ddpm_step_coefficients`                               the per-step scalars, float64
`ddpm_mu_reference` / `invert_reference` / `edit_reference`  the recurrence in plain torch over a callable predict(x_bf16, t, multiplier):
                                                       float64 = the oracle, float32 = the kernel's operations in the kernel's order
`NoiseSpace`                                           what an inversion leaves: x0, X_0, the residuals, the reconstruction
`SliderEditor`                                         SliderSampler + invert / edit_latents / edit on the engine
"""
from __future__ import annotations

import argparse
import math
import os
from dataclasses import dataclass, fields
from typing import Callable, List, Optional, Tuple

import torch

from .ddim import DDIMSchedule
from .sampler import SliderSampler
from .vae import VaeDecoder

COEFFICIENTS = ("c_sqrt_beta_t", "c_inv_sqrt_alpha_t", "c_sqrt_alpha_t", "c_sqrt_alpha_prev", "c_dir")   # the descriptor's scalars


def default_skip(steps: int) -> int:
    """the paper's 36 of 100"""
    return int(0.36 * steps)


def edit_timesteps(schedule: DDIMSchedule, steps: int, skip: Optional[int] = None) -> List[int]:
    skip = default_skip(steps) if skip is None else int(skip)
    if not 0 <= skip < steps:
        raise ValueError(f"skip = {skip}: expected 0 <= skip < steps = {steps}")
    return schedule.make_timesteps(steps)[skip:]


def ddpm_step_coefficients(schedule: DDIMSchedule, t: int, steps: int, eta: float = 1.0) -> dict:
    """The scalars of the step t -> t - 1000 // steps, in float64 from schedule.alphas_cumprod (the kernel reads their fp32
    roundings: `fp32_coefficients`).  sigma is the DDPM noise level of the step; c_dir^2 + sigma^2 = 1 - alpha_prev.  On the last
    step alpha_prev = final_alpha_cumprod = 1: sigma = 0, c_dir = 0, c_sqrt_alpha_prev = 1."""
    if not 0.0 <= eta <= 1.0:
        raise ValueError(f"eta = {eta}: expected 0 <= eta <= 1")
    prev = t - schedule.num_train_timesteps // steps
    a_t = float(schedule.alphas_cumprod[t])
    a_p = float(schedule.alphas_cumprod[prev]) if prev >= 0 else float(schedule.final_alpha_cumprod)
    sigma = eta * math.sqrt((1.0 - a_p) / (1.0 - a_t)) * math.sqrt(max(0.0, 1.0 - a_t / a_p))
    return dict(sigma=sigma, c_dir=math.sqrt(max(0.0, 1.0 - a_p - sigma * sigma)), c_sqrt_alpha_prev=math.sqrt(a_p),
                c_sqrt_beta_t=math.sqrt(1.0 - a_t), c_inv_sqrt_alpha_t=1.0 / math.sqrt(a_t), c_sqrt_alpha_t=math.sqrt(a_t))


def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float64).to(torch.float32))


def fp32_coefficients(coef: dict) -> dict:
    """The descriptor's five scalars rounded to fp32 (as Python floats): what the kernel multiplies with"""
    return {k: _f32(coef[k]) for k in COEFFICIENTS}


def ddpm_mu_reference(eps_uncond: torch.Tensor, eps_text: torch.Tensor, x: torch.Tensor, coef: dict, guidance: float,
                      v_prediction: bool = False, dtype=torch.float64) -> torch.Tensor:
    """mu of one step from the bf16 epsilon halves and the master latent, on the fp32 values of the scalars.  float64: the oracle.
    float32: one tensor operation per operation of ddpm_edit_kernel, in its order - each rounds once, nothing is contracted."""
    c = {k: torch.tensor(v, dtype=dtype) for k, v in fp32_coefficients(coef).items()}
    g = torch.tensor(_f32(guidance), dtype=dtype)
    u, t, x = eps_uncond.to(dtype), eps_text.to(dtype), x.to(dtype)
    e = u + g * (t - u)
    if v_prediction:
        x0 = c["c_sqrt_alpha_t"] * x - c["c_sqrt_beta_t"] * e
        pe = c["c_sqrt_alpha_t"] * e + c["c_sqrt_beta_t"] * x
    else:
        x0 = (x - c["c_sqrt_beta_t"] * e) * c["c_inv_sqrt_alpha_t"]
        pe = e
    return c["c_sqrt_alpha_prev"] * x0 + c["c_dir"] * pe


def build_path(schedule: DDIMSchedule, x0: torch.Tensor, ts: List[int], seed: int) -> torch.Tensor:
    """X_i = sqrt(a_i) x0 + sqrt(1 - a_i) e_i for every t_i of the grid, [len(ts)][bs][4][h][w] in x0's dtype on x0's device; the e_i
    are ONE draw of a CPU generator seeded with `seed` (independent per step: what makes the space edit-friendly)."""
    g = torch.Generator().manual_seed(int(seed))
    noise = torch.randn((len(ts),) + tuple(x0.shape), generator=g, dtype=torch.float32).to(device=x0.device, dtype=x0.dtype)
    a = torch.tensor([float(schedule.alphas_cumprod[t]) for t in ts], dtype=torch.float64)
    shape = (len(ts),) + (1,) * x0.dim()
    sa = a.sqrt().to(device=x0.device, dtype=x0.dtype).reshape(shape)
    sb = (1.0 - a).sqrt().to(device=x0.device, dtype=x0.dtype).reshape(shape)
    return sa * x0[None] + sb * noise


@dataclass
class NoiseSpace:
    """What `invert` leaves: enough to edit the image any number of times.  Tensors are fp32 (float64 from the float64 reference)."""
    x0: torch.Tensor                 # [bs][4][h][w] the encoded image: scaling_factor * posterior mean
    x_start: torch.Tensor            # X_0, the latent at timesteps[0]
    resid: torch.Tensor              # [len(timesteps)][bs][4][h][w]  d_i = target_i - mu_i
    recon: torch.Tensor              # the final x of the inversion's own chain: x0 up to two roundings
    timesteps: List[int]
    steps: int
    skip: int
    eta: float
    guidance: float
    prediction_type: str
    seed: int
    ctx: Optional[torch.Tensor] = None          # the conditioning the inversion ran with (an edit without its own reuses it)
    pooled: Optional[torch.Tensor] = None
    time_ids: Optional[torch.Tensor] = None

    def _map(self, fn) -> dict:
        return {f.name: fn(getattr(self, f.name)) if torch.is_tensor(getattr(self, f.name)) else getattr(self, f.name) for f in fields(self)}

    def save(self, path: str):
        """torch.save of plain tensors (on the CPU) and numbers"""
        torch.save(self._map(lambda v: v.detach().cpu()), path)

    @classmethod
    def load(cls, path: str, device=None) -> "NoiseSpace":
        d = torch.load(path, map_location="cpu")
        missing = [f.name for f in fields(cls) if f.name not in d]
        if missing:
            raise KeyError(f"{path}: not a saved NoiseSpace (no {missing})")
        d = {f.name: d[f.name] for f in fields(cls)}
        d["timesteps"] = [int(t) for t in d["timesteps"]]
        sp = cls(**d)
        return sp.to(device) if device is not None else sp

    def to(self, device) -> "NoiseSpace":
        return NoiseSpace(**self._map(lambda v: v.to(device)))


Predict = Callable[[torch.Tensor, int, float], Tuple[torch.Tensor, torch.Tensor]]


def invert_reference(predict: Predict, x0: torch.Tensor, schedule: DDIMSchedule, steps: int = 50, skip: Optional[int] = None,
                     eta: float = 1.0, guidance: float = 7.5, seed: int = 0, dtype=torch.float32) -> NoiseSpace:
    """The inversion over predict(x_bf16, t, multiplier) -> (eps_uncond, eps_text), multiplier 0 throughout."""
    ts = edit_timesteps(schedule, steps, skip)
    x0 = x0.to(dtype)
    path = build_path(schedule, x0, ts, seed)
    v = schedule.prediction_type == "v_prediction"
    x = path[0].clone()
    resid = torch.empty_like(path)
    for i, t in enumerate(ts):
        eu, et = predict(x.to(torch.bfloat16), t, 0.0)
        mu = ddpm_mu_reference(eu, et, x, ddpm_step_coefficients(schedule, t, steps, eta), guidance, v, dtype)
        target = path[i + 1] if i + 1 < len(ts) else x0
        resid[i] = target - mu
        x = mu + resid[i]                     # NOT target: the edit can only recompute mu + d
    return NoiseSpace(x0=x0, x_start=path[0].clone(), resid=resid, recon=x, timesteps=list(ts), steps=int(steps),
                      skip=steps - len(ts), eta=float(eta), guidance=float(guidance), prediction_type=schedule.prediction_type,
                      seed=int(seed))


def edit_reference(predict: Predict, space: NoiseSpace, schedule: DDIMSchedule, scale: float = 0.0, start_noise: int = 750,
                   guidance: Optional[float] = None, dtype=torch.float32) -> torch.Tensor:
    """The edit at slider scale `scale` (multiplier 0 while t > start_noise, as SliderSampler.sample_latents)."""
    g = space.guidance if guidance is None else guidance
    v = schedule.prediction_type == "v_prediction"
    x = space.x_start.to(dtype).clone()
    for i, t in enumerate(space.timesteps):
        eu, et = predict(x.to(torch.bfloat16), t, 0.0 if t > start_noise else float(scale))
        mu = ddpm_mu_reference(eu, et, x, ddpm_step_coefficients(schedule, t, space.steps, space.eta), g, v, dtype)
        x = mu + space.resid[i].to(dtype)
    return x


# ---------------------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------------------
class SliderEditor(SliderSampler):
    """SliderSampler (same constructor; the scheduler must be DDIM) that also inverts a given image's latents into a NoiseSpace and
    edits them.  With store= the inversion and the edit replay the adapter program ("on", multiplier 0 resp. `scale`); with sliders=
    or no slider the adapter-free one, the edit on merged weights below start_noise."""

    def __init__(self, engine, store=None, decoder=None, prediction_type: str = "epsilon", scheduler: str = "ddim",
                 scheduler_seed: int = 0, sliders=None):
        if scheduler.lower().replace(" ", "_") != "ddim":
            raise ValueError(f"SliderEditor: scheduler {scheduler!r}: the DDPM noise space is defined on the DDIM grid")
        super().__init__(engine, store, decoder, prediction_type, "ddim", scheduler_seed, sliders)

    def _load_inputs(self, bs: int, h: int, w: int, ctx, pooled, time_ids):
        """the plan of this shape with its conditioning inputs written (the lines SliderSampler.sample_latents starts with)"""
        eng = self.eng
        p = eng.plan(2 * bs, h, w, "on" if self.store is not None else "off")
        io = p.io
        io["ctx"].tensor.copy_(ctx.to(torch.bfloat16))
        if eng.cfg.is_xl:
            if time_ids is None:
                time_ids = torch.tensor([[h * 8.0, w * 8.0, 0.0, 0.0, h * 8.0, w * 8.0]] * (2 * bs))
            io["time_ids"].tensor.copy_(time_ids.to(device=eng.device, dtype=torch.float32).reshape(2 * bs, 6))
            io["add_in"].tensor[:, : eng.cfg.pooled_dim].copy_(pooled.to(torch.bfloat16))
        return p

    def _edit_program(self, p, i: int, t: int, scale: float, start_noise: float):
        """SliderSampler._program, except that a multiplier of 0 means the inversion's program: at scale 0 nothing is merged, sliders
        held at a fixed scale included (they belong to the edit, and scale 0 is the reconstruction)."""
        if float(scale) == 0.0:
            return p.prog if i == 0 or p.prog_text_cached is None else p.prog_text_cached
        return self._program(p, i, t, scale, start_noise)

    def _chain(self, p, x, ts, steps, eta, guidance, scale, start_noise, resid, path=None, x0=None):
        """x (fp32, updated in place) through the grid: path given = invert (resid written), else edit (resid read)"""
        from . import lib
        eng, io = self.eng, p.io
        bs = x.shape[0]
        chw = x[0].numel()
        smp = io["sample"]
        xb = x.to(torch.bfloat16)
        smp.tensor[:bs].copy_(xb)
        smp.tensor[bs:].copy_(xb)
        s = torch.cuda.current_stream().cuda_stream
        v = 1 if self.sched.prediction_type == "v_prediction" else 0
        try:
            for i, t in enumerate(ts):
                if self.store is not None:
                    eng.set_lora(True, 0.0 if t > start_noise else float(scale))
                io["t"].tensor.fill_(float(t))
                self._edit_program(p, i, t, scale, start_noise).run(s)
                target = 0 if path is None else (path[i + 1] if i + 1 < len(ts) else x0).data_ptr()
                d = lib.DdpmEditDesc(eps=io["eps"].ptr, x=x.data_ptr(), target=target, resid=resid[i].data_ptr(), out=x.data_ptr(),
                                     out_bf16=smp.ptr, out2_bf16=smp.ptr + bs * chw * 2, nb=bs, chw=chw, guidance=float(guidance),
                                     mode=0 if path is not None else 1, v_prediction=v,
                                     **fp32_coefficients(ddpm_step_coefficients(self.sched, t, steps, eta)))
                lib.call(lib.OP_DDPM_EDIT, d, s)
        finally:
            self._restore()
            if self.store is not None:
                eng.set_lora(False)
        return x

    @torch.no_grad()
    def invert(self, ctx: torch.Tensor, x0_latents: torch.Tensor, steps: int = 50, skip: Optional[int] = None, eta: float = 1.0,
               guidance_scale: float = 7.5, seed: int = 0, pooled: Optional[torch.Tensor] = None,
               time_ids: Optional[torch.Tensor] = None) -> NoiseSpace:
        """ctx: (2*bs, 77, D) = cat([unconditional, text]); x0_latents: (bs, 4, h, w) = scaling_factor * posterior mean of the image
        (VaeEncoder.get_noisy_image's third output with zero noises).  2 * len(grid) launches besides the UNet replays."""
        ts = edit_timesteps(self.sched, steps, skip)
        ddpm_step_coefficients(self.sched, ts[0], steps, eta)          # validates eta before anything runs
        dev = self.eng.device
        x0 = x0_latents.detach().to(dev, torch.float32).contiguous()
        bs, _, h, w = x0.shape
        p = self._load_inputs(bs, h, w, ctx, pooled, time_ids)
        path = build_path(self.sched, x0, ts, seed)
        resid = torch.empty_like(path)
        x = self._chain(p, path[0].clone(), ts, steps, eta, guidance_scale, 0.0, -1, resid, path, x0)
        return NoiseSpace(x0=x0, x_start=path[0].clone(), resid=resid, recon=x, timesteps=list(ts), steps=int(steps),
                          skip=steps - len(ts), eta=float(eta), guidance=float(guidance_scale),
                          prediction_type=self.sched.prediction_type, seed=int(seed), ctx=ctx.detach().clone(),
                          pooled=None if pooled is None else pooled.detach().clone(),
                          time_ids=None if time_ids is None else time_ids.detach().clone())

    @torch.no_grad()
    def edit_latents(self, space: NoiseSpace, ctx: Optional[torch.Tensor] = None, scale: float = 0.0, start_noise: int = 750,
                     guidance_scale: Optional[float] = None, pooled: Optional[torch.Tensor] = None,
                     time_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> the edited latents (bs, 4, h, w) fp32.  ctx / guidance_scale None: the inversion's own - then scale 0 returns
        space.recon bit for bit.  Another prompt or guidance is an edit of its own; no reconstruction claim applies."""
        if space.prediction_type != self.sched.prediction_type:
            raise ValueError(f"the NoiseSpace was inverted with {space.prediction_type}, this editor predicts {self.sched.prediction_type}")
        if ctx is None:
            if space.ctx is None:
                raise ValueError("edit_latents: this NoiseSpace carries no conditioning; pass ctx")
            ctx = space.ctx
            pooled = space.pooled if pooled is None else pooled
            time_ids = space.time_ids if time_ids is None else time_ids
        dev = self.eng.device
        x = space.x_start.to(dev, torch.float32).clone().contiguous()
        resid = space.resid.to(dev, torch.float32).contiguous()
        bs, _, h, w = x.shape
        p = self._load_inputs(bs, h, w, ctx, pooled, time_ids)
        g = space.guidance if guidance_scale is None else guidance_scale
        return self._chain(p, x, space.timesteps, space.steps, space.eta, g, scale, start_noise, resid)

    @torch.no_grad()
    def edit(self, space: NoiseSpace, **kw) -> torch.Tensor:
        """-> uint8 images [bs][H][W][3] (needs a VaeDecoder)."""
        if self.decoder is None:
            raise RuntimeError("SliderEditor.edit needs a VaeDecoder")
        return VaeDecoder.to_uint8(self.decoder.decode(self.edit_latents(space, **kw)))


# ---------------------------------------------------------------------------------------------------------------------------------
# python -m sliders_amd.edit
# ---------------------------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="edit a given image with a trained slider (docs/EDIT.md)")
    p.add_argument("--model", default="sdxl", choices=["sdxl", "sd1"])
    p.add_argument("--model_path", default=None, help="diffusers-format model directory (unet/, vae/, text encoders)")
    p.add_argument("--synthetic", action="store_true", help="random-init weights and embeddings (no model files)")
    p.add_argument("--lora_weight", default=None, help="slider checkpoint (.pt) written by the trainers")
    p.add_argument("--compose", action="append", default=[], metavar="PATH:SCALE",
                   help="one more slider (.pt, any rank) held at a fixed scale in every edit of non-zero scale; repeatable (merged weights, "
                        "as sliders_amd.generate)")
    p.add_argument("--image", default=None, help="the image to edit (resized to res x res)")
    p.add_argument("--prompt", default="image of a person", help="describes the image: the inversion's conditioning")
    p.add_argument("--edit_prompt", default=None, help="another prompt for the edits (default: --prompt)")
    p.add_argument("--scales", default="-2,-1,0,1,2")
    p.add_argument("--start_noise", type=int, default=750)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--skip", type=int, default=None, help="noisiest steps of the grid left out (default int(0.36 * steps))")
    p.add_argument("--eta", type=float, default=1.0)
    p.add_argument("--guidance_scale", type=float, default=7.5)
    p.add_argument("--edit_guidance_scale", type=float, default=None, help="guidance of the edits (default: the inversion's)")
    p.add_argument("--save_inversion", default=None, help="write the NoiseSpace here")
    p.add_argument("--inversion", default=None, help="edit a saved NoiseSpace instead of inverting --image")
    p.add_argument("--res", type=int, default=None)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--out", default="edited")
    return p


def check_args(a):
    """every argument error, before any model is built"""
    if a.inversion and a.save_inversion:
        raise SystemExit("--inversion reads a saved inversion, --save_inversion writes one: give one of them")
    if not a.inversion and not a.image:
        raise SystemExit("--image (or --inversion) is required")
    if not 1 <= a.steps <= 1000:
        raise SystemExit(f"--steps {a.steps}: expected 1 <= steps <= 1000")
    skip = default_skip(a.steps) if a.skip is None else a.skip
    if not 0 <= skip < a.steps:
        raise SystemExit(f"--skip {skip}: expected 0 <= skip < steps = {a.steps}")
    if not 0.0 <= a.eta <= 1.0:
        raise SystemExit(f"--eta {a.eta}: expected 0 <= eta <= 1")
    if not a.synthetic and not a.model_path:
        raise SystemExit("--model_path (diffusers-format directory) or --synthetic is required")
    try:
        scales = [float(v) for v in a.scales.split(",")]
    except ValueError:
        raise SystemExit(f"--scales {a.scales!r}: expected comma-separated numbers")
    return scales


def main(argv=None):
    a = build_parser().parse_args(argv)
    scales = check_args(a)
    from .generate import parse_compose, parse_slider_name, slider_rank
    held = [parse_compose(c) for c in a.compose]
    from PIL import Image
    from .lora_store import LoraStore
    from .model_util import load_unet_engine, synthetic_engine
    from .vae import VAE_SCALING, VaeEncoder, random_vae_state_dict
    dev = torch.device("cuda", a.device)
    xl = a.model == "sdxl"
    res = a.res or (1024 if xl else 512)
    prompts = [a.prompt] + ([a.edit_prompt] if a.edit_prompt is not None else [])
    if a.synthetic:
        eng = synthetic_engine(a.model, dev, a.seed)
        vae_sd = random_vae_state_dict(device=dev, seed=a.seed, decoder=True)
        g = torch.Generator().manual_seed(a.seed)
        cond = []
        for _ in prompts:            # a prompt is a draw: the first is the image's, the second the edit's
            cond.append((torch.randn(2, 77, eng.cfg.cross_attention_dim, generator=g),
                         torch.randn(2, eng.cfg.pooled_dim, generator=g) if xl else None))
    else:
        from safetensors.torch import load_file
        from . import model_util
        eng = load_unet_engine(a.model_path, dev)
        vae_sd = load_file(os.path.join(a.model_path, "vae", "diffusion_pytorch_model.safetensors"))
        cond = []
        if xl:
            toks, encs = model_util.load_text_encoders_xl(a.model_path, dev, torch.bfloat16)
            for pr in prompts:
                (e_u, p_u), (e_t, p_t) = (model_util.encode_prompts_xl(toks, encs, [s]) for s in ("", pr))
                cond.append((torch.cat([e_u, e_t]), torch.cat([p_u, p_t])))
        else:
            tok, enc = model_util.load_text_encoder(a.model_path, dev, torch.bfloat16)
            for pr in prompts:
                cond.append((torch.cat([model_util.encode_prompts(tok, enc, [s]) for s in ("", pr)]), None))
    dec = VaeDecoder(vae_sd, dev, VAE_SCALING[a.model])
    store = sliders = None
    swept = torch.load(a.lora_weight, map_location="cpu") if a.lora_weight else None
    if held or (swept is not None and slider_rank(swept) != 4):
        from .merge import SliderSet
        sliders = SliderSet(eng.cfg, ([(swept, None)] if swept is not None else [])
                            + [(torch.load(path, map_location="cpu"), s) for path, s in held])
    elif swept is not None:
        rank, alpha, method = parse_slider_name(a.lora_weight)
        store = LoraStore(eng.cfg, rank=rank, alpha=alpha, train_method=method, device=dev, init="none")
        store.load_state_dict(swept, strict=True)
    ed = SliderEditor(eng, store, dec, sliders=sliders)
    ctx, pooled = (None if v is None else v.to(dev) for v in cond[0])
    if a.inversion:
        space = NoiseSpace.load(a.inversion, dev)
        if space.ctx is None:
            space.ctx, space.pooled = ctx, pooled
    else:
        img = Image.open(a.image).convert("RGB").resize((res, res), Image.LANCZOS)
        encoder = VaeEncoder(vae_sd, dev, VAE_SCALING[a.model])
        image = VaeEncoder.preprocess(img).to(dev)
        zero = torch.zeros(1, 4, res // 8, res // 8, device=dev)
        x0 = encoder.get_noisy_image(image, zero, zero, 1.0, 0.0)[2].clone()          # scaling_factor * posterior mean, fp32
        del encoder
        space = ed.invert(ctx, x0, steps=a.steps, skip=a.skip, eta=a.eta, guidance_scale=a.guidance_scale, seed=a.seed, pooled=pooled)
        if a.save_inversion:
            space.save(a.save_inversion)
            print(f"inversion saved to {a.save_inversion}")
    os.makedirs(a.out, exist_ok=True)
    Image.fromarray(VaeDecoder.to_uint8(dec.decode(space.recon))[0].cpu().numpy()).save(os.path.join(a.out, "recon.png"))
    kw = dict(start_noise=a.start_noise, guidance_scale=a.edit_guidance_scale)
    if a.edit_prompt is not None:
        kw.update(ctx=cond[1][0].to(dev), pooled=None if cond[1][1] is None else cond[1][1].to(dev))
    for s in scales:
        img = ed.edit(space, scale=s, **kw)
        Image.fromarray(img[0].cpu().numpy()).save(os.path.join(a.out, f"scale_{s:g}.png"))
        print(f"scale {s:g}: saved {os.path.join(a.out, f'scale_{s:g}.png')}")
    return a.out


if __name__ == "__main__":
    main()
