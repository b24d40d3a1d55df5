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
`NoiseSpace`                                           what an inversion leaves: x0, X_0, the residuals, the reconstruction, its latents
`SliderEditor`                                         SliderSampler + invert / edit_latents / edit / footprint on the engine

`ddpm_step2_coefficients` / `ddpm_mu2_reference`        the second-order space (invert(order=2), --order 2; docs/EDIT.md "Second-order noise
                                                       space"): mu gains c_corr (x0h - x0h of the chain's step before), one launch of
                                                       slh_edit_step2 per step; NoiseSpace.order says which, and every edit reads it

Localised edits (mask=, --mask / --auto_mask): every step of an edit is blended against the latent the inversion itself had after
that step (NoiseSpace.visited, slh_ddpm_edit_blend), so outside the mask the result is the reconstruction bit for bit.  The mask
comes from a file (`load_mask`, `feather_mask`) or from where the slider changes the predicted noise on this image
(`SliderEditor.footprint`, slh_eps_absdiff; `footprint_mask`), or from where a word of the prompt lives in the UNet's cross-attention
(`SliderEditor.word_map`, slh_xattn_map; `word_mask`, `word_token_indices`).  `blend_reference` restates the blend as the other
references do.

Prompt-direction edits (directions=, --direction; docs/EDIT.md "Prompt-direction edits"): below start_noise the pass also carries the
positive and unconditional prompt of up to three pairs (sliders_amd/directions.py), and the step reads the text row with their scaled
differences added (slh_eps_direction, or slh_eps_direction_momentum with direction_momentum=) through its eps_text input.
"""
from __future__ import annotations

import argparse
import math
import os
from dataclasses import dataclass, fields
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import lib
from .ddim import DDIMSchedule
from .directions import DirectionGuide, DirectionSet, check_momentum
from .passes import Pass
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
    """The descriptor's five scalars rounded to fp32 (as Python floats): what the kernel multiplies with; and c_corr where the step
    has one (`ddpm_step2_coefficients`)"""
    return {k: _f32(coef[k]) for k in COEFFICIENTS + (("c_corr",) if "c_corr" in coef else ())}


def check_order(order: int) -> int:
    if order not in (1, 2):
        raise ValueError(f"order = {order!r}: expected 1 or 2")
    return int(order)


def ddpm_step2_coefficients(schedule: DDIMSchedule, t: int, steps: int, eta: float = 1.0, t_older: Optional[int] = None) -> dict:
    """`ddpm_step_coefficients` of the step from t, and, where the step is second order, c_corr: the weight of x0h(t) - x0h(t_older)
    in the mean (docs/EDIT.md, "Second-order noise space").  With lambda = ln(sqrt(a) / sqrt(1 - a)),

        h = lambda(prev) - lambda(t)    h_old = lambda(t) - lambda(t_older)
        B = c_sqrt_alpha_prev - c_dir c_sqrt_alpha_t / c_sqrt_beta_t          d mu_1 / d x0h at fixed x, epsilon and v prediction alike
        c_corr = B h / (2 h_old)

    in float64.  t_older: the grid point before t; None on the grid's first step.  There, and on the last step (prev < 0: lambda(prev)
    is infinite with alpha_prev = 1, the `lower_order_final` of the multistep solvers), the step is first order and the dict has no c_corr."""
    coef = ddpm_step_coefficients(schedule, t, steps, eta)
    prev = t - schedule.num_train_timesteps // steps
    if t_older is None or prev < 0:
        return coef
    if not t_older > t:
        raise ValueError(f"t_older = {t_older}: expected the grid point before t = {t}")
    lam = lambda a: 0.5 * (math.log(a) - math.log1p(-a))
    a_t, a_p, a_o = (float(schedule.alphas_cumprod[k]) for k in (t, prev, t_older))
    h, h_old = lam(a_p) - lam(a_t), lam(a_t) - lam(a_o)
    B = coef["c_sqrt_alpha_prev"] - coef["c_dir"] * coef["c_sqrt_alpha_t"] / coef["c_sqrt_beta_t"]
    return dict(coef, c_corr=0.5 * B * h / h_old)


def chain_coefficients(schedule: DDIMSchedule, ts: List[int], i: int, steps: int, eta: float, order: int = 1) -> dict:
    """the scalars of step i of the grid ts for a chain of this order"""
    if order == 1:
        return ddpm_step_coefficients(schedule, ts[i], steps, eta)
    return ddpm_step2_coefficients(schedule, ts[i], steps, eta, ts[i - 1] if i > 0 else None)


def ddpm_mu_reference(eps_uncond: torch.Tensor, eps_text: torch.Tensor, x: torch.Tensor, coef: dict, guidance: float,
                      v_prediction: bool = False, dtype=torch.float64) -> torch.Tensor:
    """mu of one step from the bf16 epsilon halves and the master latent, on the fp32 values of the scalars.  float64: the oracle.
    float32: one tensor operation per operation of ddpm_edit_kernel, in its order - each rounds once, nothing is contracted."""
    return ddpm_mu2_reference(eps_uncond, eps_text, x, {k: coef[k] for k in COEFFICIENTS}, guidance, v_prediction, dtype)[0]


def ddpm_mu2_reference(eps_uncond: torch.Tensor, eps_text: torch.Tensor, x: torch.Tensor, coef: dict, guidance: float,
                       v_prediction: bool = False, dtype=torch.float64, x0_prev: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mu, x0h) of one step of the second-order chain: mu_1 and x0h as `ddpm_mu_reference` forms them, and where coef has a c_corr
    (`ddpm_step2_coefficients`) and x0_prev - the same chain's x0h one step earlier - is given, mu = mu_1 + c_corr (x0h - x0_prev).
    float64: the oracle.  float32: one tensor operation per operation of edit_step2_kernel, in its order."""
    if ("c_corr" in coef) != (x0_prev is not None):
        raise ValueError("ddpm_mu2_reference: c_corr and x0_prev go together (neither on a first-order step)")
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
    mu = c["c_sqrt_alpha_prev"] * x0 + c["c_dir"] * pe
    if x0_prev is not None:
        d = x0 - x0_prev.to(dtype)
        p = c["c_corr"] * d
        mu = mu + p
    return mu, x0


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
    visited: Optional[torch.Tensor] = None      # [len(timesteps)][bs][4][h][w] the latent after each step of the inversion's own chain
                                                # (visited[-1] == recon): what a masked edit keeps outside the mask
    order: int = 1                              # 1: the DDIM mean; 2: with the multistep correction (every edit of the space reads it)

    def _map(self, fn) -> dict:
        return {f.name: fn(getattr(self, f.name)) if torch.is_tensor(getattr(self, f.name)) else getattr(self, f.name) for f in fields(self)}

    def save(self, path: str):
        """torch.save of plain tensors (on the CPU) and numbers"""
        torch.save(self._map(lambda v: v.detach().cpu()), path)

    @classmethod
    def load(cls, path: str, device=None) -> "NoiseSpace":
        d = torch.load(path, map_location="cpu")
        # files from before masked edits have no visited, files from before the second-order space no order: they are first order
        missing = [f.name for f in fields(cls) if f.name not in d and f.name not in ("visited", "order")]
        if missing:
            raise KeyError(f"{path}: not a saved NoiseSpace (no {missing})")
        d = {f.name: d.get(f.name) for f in fields(cls)}
        d["timesteps"] = [int(t) for t in d["timesteps"]]
        d["order"] = check_order(1 if d["order"] is None else d["order"])
        sp = cls(**d)
        return sp.to(device) if device is not None else sp

    def to(self, device) -> "NoiseSpace":
        return NoiseSpace(**self._map(lambda v: v.to(device)))


Predict = Callable[[torch.Tensor, int, float], Tuple[torch.Tensor, torch.Tensor]]


def invert_reference(predict: Predict, x0: torch.Tensor, schedule: DDIMSchedule, steps: int = 50, skip: Optional[int] = None,
                     eta: float = 1.0, guidance: float = 7.5, seed: int = 0, dtype=torch.float32, order: int = 1) -> NoiseSpace:
    """The inversion over predict(x_bf16, t, multiplier) -> (eps_uncond, eps_text), multiplier 0 throughout.  order 2: every step but
    the first and the last adds the correction from the chain's own x0h of the step before (`ddpm_mu2_reference`)."""
    check_order(order)
    ts = edit_timesteps(schedule, steps, skip)
    x0 = x0.to(dtype)
    path = build_path(schedule, x0, ts, seed)
    v = schedule.prediction_type == "v_prediction"
    x = path[0].clone()
    resid, visited = torch.empty_like(path), torch.empty_like(path)
    hist = None
    for i, t in enumerate(ts):
        eu, et = predict(x.to(torch.bfloat16), t, 0.0)
        mu, hist = _mu_step(eu, et, x, schedule, ts, i, steps, eta, guidance, v, dtype, order, hist)
        target = path[i + 1] if i + 1 < len(ts) else x0
        resid[i] = target - mu
        x = mu + resid[i]                     # NOT target: the edit can only recompute mu + d
        visited[i] = x
    return NoiseSpace(x0=x0, x_start=path[0].clone(), resid=resid, recon=x, timesteps=list(ts), steps=int(steps),
                      skip=steps - len(ts), eta=float(eta), guidance=float(guidance), prediction_type=schedule.prediction_type,
                      seed=int(seed), visited=visited, order=order)


def _mu_step(eu, et, x, schedule, ts, i, steps, eta, guidance, v, dtype, order, hist):
    """(mu, x0h) of step i of a reference chain of this order; hist: the chain's x0h of step i - 1 (read only where the step has a c_corr)"""
    coef = chain_coefficients(schedule, ts, i, steps, eta, order)
    return ddpm_mu2_reference(eu, et, x, coef, guidance, v, dtype, hist if "c_corr" in coef else None)


def as_mask(mask: torch.Tensor, bs: int, h: int, w: int) -> torch.Tensor:
    """[h][w], [bs][h][w] or [bs][1][h][w] with values in [0, 1] -> fp32 [bs][1][h][w], contiguous (one value per latent pixel, shared
    by the channels); anything else is a ValueError"""
    if not torch.is_tensor(mask):
        raise ValueError(f"mask: expected a tensor, got {type(mask).__name__}")
    shape = tuple(mask.shape)
    if shape not in ((h, w), (bs, h, w), (bs, 1, h, w)):
        raise ValueError(f"mask of shape {shape}: expected ({h}, {w}), ({bs}, {h}, {w}) or ({bs}, 1, {h}, {w})")
    if not (mask.dtype.is_floating_point or mask.dtype == torch.bool):
        raise ValueError(f"mask of dtype {mask.dtype}: expected floating point values in [0, 1] (or bool)")
    m = mask.detach().to(torch.float32)
    if not bool(((m >= 0.0) & (m <= 1.0)).all()):            # NaN fails both comparisons
        raise ValueError("mask values must lie in [0, 1]")
    return (m[None].expand(bs, h, w) if m.dim() == 2 else m).reshape(bs, 1, h, w).contiguous()


def blend_reference(e: torch.Tensor, keep: torch.Tensor, mask: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """The masked step's blend of the edited latent e against the inversion's latent `keep`, mask broadcast over the channels:
    keep where the mask is 0, e where it is 1 (both exactly), keep + m (e - keep) between.  float64: the oracle.  float32: the
    operations of ddpm_edit_blend_kernel in its order, one rounding each."""
    e, k, m = e.to(dtype), keep.to(dtype), mask.to(dtype)
    out = k + m * (e - k)
    return torch.where(m == 0, k, torch.where(m == 1, e, out))


def edit_reference(predict: Predict, space: NoiseSpace, schedule: DDIMSchedule, scale: float = 0.0, start_noise: int = 750,
                   guidance: Optional[float] = None, dtype=torch.float32, mask: Optional[torch.Tensor] = None,
                   order: Optional[int] = None) -> torch.Tensor:
    """The edit at slider scale `scale` (multiplier 0 while t > start_noise, as SliderSampler.sample_latents).  mask: every step is
    blended against the inversion's latent after that step (space.visited), so the result is space.recon outside the mask.
    order None: the space's own (another order is another image; no reconstruction claim applies).  At order 2 the history is the
    edit chain's own x0h, formed on the blended and guided latent of the step before."""
    order = check_order(space.order if order is None else order)
    g = space.guidance if guidance is None else guidance
    v = schedule.prediction_type == "v_prediction"
    x = space.x_start.to(dtype).clone()
    if mask is not None:
        space = trajectory_reference(predict, space, schedule, dtype, order)
        mask = as_mask(mask, x.shape[0], x.shape[2], x.shape[3])
    hist = None
    for i, t in enumerate(space.timesteps):
        eu, et = predict(x.to(torch.bfloat16), t, 0.0 if t > start_noise else float(scale))
        mu, hist = _mu_step(eu, et, x, schedule, space.timesteps, i, space.steps, space.eta, g, v, dtype, order, hist)
        x = mu + space.resid[i].to(dtype)
        if mask is not None:
            x = blend_reference(x, space.visited[i], mask, dtype)
    return x


def trajectory_reference(predict: Predict, space: NoiseSpace, schedule: DDIMSchedule, dtype=torch.float32,
                         order: Optional[int] = None) -> NoiseSpace:
    """Fills a missing space.visited by the scale-0 replay (SliderEditor.trajectory over predict); raises if it does not end on recon.
    order None: the space's own."""
    if space.visited is not None:
        return space
    order = check_order(space.order if order is None else order)
    v = schedule.prediction_type == "v_prediction"
    x = space.x_start.to(dtype).clone()
    visited = torch.empty_like(space.resid, dtype=dtype)
    hist = None
    for i, t in enumerate(space.timesteps):
        eu, et = predict(x.to(torch.bfloat16), t, 0.0)
        mu, hist = _mu_step(eu, et, x, schedule, space.timesteps, i, space.steps, space.eta, space.guidance, v, dtype, order, hist)
        x = mu + space.resid[i].to(dtype)
        visited[i] = x
    if not torch.equal(x, space.recon.to(dtype)):
        raise RuntimeError("trajectory_reference: the scale-0 replay does not end on space.recon bit for bit")
    space.visited = visited
    return space


# ---------------------------------------------------------------------------------------------------------------------------------
# masks: from a file, or from the slider's footprint (host tensor ops on one small array per image)
# ---------------------------------------------------------------------------------------------------------------------------------
def load_mask(path: str, res: int, invert: bool = False) -> torch.Tensor:
    """An image file -> the latent-resolution mask [res/8][res/8] fp32 in [0, 1]: grey levels / 255 at res x res (BOX filter), then
    the mean over each 8 x 8 block of pixels (one latent pixel).  White means edit; invert swaps the sides."""
    from PIL import Image
    import numpy as np
    if res <= 0 or res % 8:
        raise ValueError(f"load_mask: res = {res}: expected a positive multiple of 8")
    img = Image.open(path).convert("L").resize((res, res), Image.BOX)
    m = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).to(torch.float32) / 255.0
    m = m.reshape(res // 8, 8, res // 8, 8).mean(dim=(1, 3))
    return 1.0 - m if invert else m


def feather_mask(mask: torch.Tensor, sigma: float) -> torch.Tensor:
    """Separable Gaussian blur in latent pixels over the last two dimensions: radius ceil(3 sigma), taps normalised to sum 1, replicate
    padding, fp32, clamped to [0, 1].  sigma = 0 returns the mask as it is."""
    sigma = float(sigma)
    if not sigma >= 0.0 or math.isinf(sigma):
        raise ValueError(f"feather_mask: sigma = {sigma}: expected a finite sigma >= 0")
    if mask.dim() < 2:
        raise ValueError(f"feather_mask: mask of shape {tuple(mask.shape)}: expected at least two dimensions")
    if sigma == 0.0:
        return mask
    import torch.nn.functional as F
    r = int(math.ceil(3.0 * sigma))
    taps = torch.exp(-0.5 * (torch.arange(-r, r + 1, dtype=torch.float32, device=mask.device) / sigma) ** 2)
    taps = taps / taps.sum()
    h, w = mask.shape[-2:]
    m = mask.to(torch.float32).reshape(-1, 1, h, w)
    m = F.conv2d(F.pad(m, (r, r, 0, 0), mode="replicate"), taps.reshape(1, 1, 1, -1))
    m = F.conv2d(F.pad(m, (0, 0, r, r), mode="replicate"), taps.reshape(1, 1, -1, 1))
    return m.clamp(0.0, 1.0).reshape(mask.shape)


def footprint_draws(timesteps: List[int], start_noise: int = 750, draws: int = 8, t_min: int = 200) -> List[int]:
    """The steps a footprint is measured at: `draws` of the indices i with t_min <= t_i <= start_noise, evenly spaced (all of them
    if there are fewer)"""
    if draws < 1:
        raise ValueError(f"draws = {draws}: expected draws >= 1")
    ok = [i for i, t in enumerate(timesteps) if t_min <= t <= start_noise]
    if not ok:
        raise ValueError(f"no step of the grid {list(timesteps)} has t_min = {t_min} <= t <= start_noise = {start_noise}")
    if len(ok) <= draws:
        return ok
    pick = torch.linspace(0, len(ok) - 1, draws, dtype=torch.float64).round().long().tolist()
    return [ok[j] for j in sorted(set(pick))]


def footprint_mean(A: torch.Tensor) -> torch.Tensor:
    """A [draws][bs][h][w] (slh_eps_absdiff per draw) -> F [bs][h][w]: every draw divided by its own mean over the pixels (a draw at a
    noisier level has a larger epsilon difference everywhere), then the mean over the draws; a draw whose mean is 0 contributes 0"""
    mean = A.mean(dim=(2, 3), keepdim=True)
    return torch.where(mean > 0, A / mean, torch.zeros_like(A)).mean(dim=0)


def footprint_mask(F: torch.Tensor, quantile: float = 0.98, threshold: float = 0.5, dilate: int = 1, feather: float = 1.0) -> torch.Tensor:
    """A footprint [bs][h][w] (or [h][w]) -> a mask of its shape, DiffEdit's procedure: scale by the `quantile` value of each sample
    and clamp to [0, 1], binarise at `threshold`, dilate by `dilate` pixels, feather with a Gaussian of sigma `feather`."""
    if F.dim() not in (2, 3):
        raise ValueError(f"footprint_mask: F of shape {tuple(F.shape)}: expected [bs][h][w] or [h][w]")
    if not 0.0 < quantile <= 1.0 or not 0.0 < threshold <= 1.0 or int(dilate) != dilate or dilate < 0:
        raise ValueError(f"footprint_mask: quantile = {quantile}, threshold = {threshold}, dilate = {dilate}: expected 0 < quantile <= 1, "
                         f"0 < threshold <= 1, an integer dilate >= 0")
    f = F.to(torch.float32).reshape((-1,) + tuple(F.shape[-2:]))
    hw = f.shape[1] * f.shape[2]
    q = torch.kthvalue(f.reshape(f.shape[0], hw), max(1, int(math.ceil(quantile * hw))), dim=1).values
    if not bool((q > 0).all()):
        raise ValueError("footprint_mask: the slider has no footprint at this scale")
    m = (f / q[:, None, None]).clamp(0.0, 1.0)
    return _binary_tail(m >= threshold, dilate, feather).reshape(F.shape)


def _binary_tail(inside: torch.Tensor, dilate: int, feather: float) -> torch.Tensor:
    """What footprint_mask and word_mask end with: a boolean [n][h][w] -> fp32, grown by `dilate` pixels, feathered with sigma `feather`"""
    import torch.nn.functional as nnf
    m = inside.to(torch.float32)
    if dilate > 0:
        m = nnf.max_pool2d(m[:, None], 2 * int(dilate) + 1, stride=1, padding=int(dilate))[:, 0]
    return feather_mask(m, feather)


def word_mask(F: torch.Tensor, threshold: float = 0.3, dilate: int = 1, feather: float = 1.0) -> torch.Tensor:
    """A word map [bs][h][w] (or [h][w]) -> a mask of its shape: F divided by its maximum over the pixels of each sample, binarised
    at `threshold` (a pixel exactly at it is in), then footprint_mask's dilation and feathering.  0.3 is the default of
    prompt-to-prompt's local blend; a default, not a tuned value.  A map whose maximum is not positive raises."""
    if F.dim() not in (2, 3):
        raise ValueError(f"word_mask: F of shape {tuple(F.shape)}: expected [bs][h][w] or [h][w]")
    if not 0.0 < threshold <= 1.0 or int(dilate) != dilate or dilate < 0:
        raise ValueError(f"word_mask: threshold = {threshold}, dilate = {dilate}: expected 0 < threshold <= 1, an integer dilate >= 0")
    f = F.to(torch.float32).reshape((-1,) + tuple(F.shape[-2:]))
    top = f.amax(dim=(1, 2))
    if not bool((top > 0).all()):
        raise ValueError("word_mask: the map is zero everywhere (no attention on the chosen tokens)")
    return _binary_tail(f / top[:, None, None] >= threshold, dilate, feather).reshape(F.shape)


def word_token_indices(prompt: str, word: str, tokenizer, ctx_len: int = 77) -> List[int]:
    """Key positions (BOS = 0) of the sub-word tokens that spell every whitespace-separated word of `prompt` equal to `word`
    (case-insensitive).  The prompt's tokens are decoded one by one and walked along its words: a word owns tokens until their pieces
    are as long as it is.  tokenizer: encode(prompt) -> ids with BOS first and EOS last, decode([id]) -> the piece.  Raises if the
    word is absent or one of its tokens falls past position ctx_len - 2 (the last key before the EOS of a truncated prompt)."""
    words = prompt.split()
    want = {n for n, w in enumerate(words) if w.lower() == word.lower()}
    if not want:
        raise ValueError(f"word_token_indices: {word!r} is not a word of {prompt!r}")
    ids = list(tokenizer.encode(prompt))[1:-1]
    out, at, have = [], 0, 0
    for pos, tid in enumerate(ids, start=1):
        if at >= len(words):
            break
        if at in want:
            out.append(pos)
        have += len(tokenizer.decode([tid]).strip().lstrip("#"))
        if have >= len(words[at]):
            at, have = at + 1, 0
    if not out or at <= max(want):
        raise ValueError(f"word_token_indices: the tokens of {prompt!r} end before {word!r} is spelled")
    if max(out) > ctx_len - 2:
        raise ValueError(f"word_token_indices: {word!r} reaches key position {max(out)}, past the last text key {ctx_len - 2} of a {ctx_len}-key context")
    return out


def key_weights(bs: int, ctx_len: int, tokens: Optional[Sequence[int]] = None, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The [bs][ctx_len] fp32 key weights of a word map: 1 at `tokens` (key positions, BOS = 0), or `weights` as given"""
    if (tokens is None) == (weights is None):
        raise ValueError("word_map: give either tokens= or weights=")
    if weights is not None:
        w = torch.as_tensor(weights, dtype=torch.float32)
        if tuple(w.shape) != (bs, ctx_len) or not bool(torch.isfinite(w).all()):
            raise ValueError(f"word_map: weights of shape {tuple(w.shape)}: expected finite values of shape ({bs}, {ctx_len})")
        return w.contiguous()
    tokens = [int(t) for t in tokens]
    if not tokens or min(tokens) < 0 or max(tokens) >= ctx_len:
        raise ValueError(f"word_map: tokens = {tokens}: expected key positions in 0 .. {ctx_len - 1}")
    w = torch.zeros(bs, ctx_len, dtype=torch.float32)
    w[:, tokens] = 1.0
    return w


def level_mean(maps: Dict[int, torch.Tensor], h: int, w: int) -> torch.Tensor:
    """{factor: [bs][(h / factor) (w / factor)]} -> [bs][h][w]: every level replicated factor x factor to the latent grid
    (repeat_interleave: exact), then the mean over the levels in ascending factor"""
    if not maps:
        raise ValueError("level_mean: no level")
    total = None
    for f in sorted(maps):
        if h % f or w % f:
            raise ValueError(f"level_mean: a {h} x {w} grid is not divisible by {f}")
        m = maps[f].to(torch.float32).reshape(-1, h // f, w // f).repeat_interleave(f, dim=1).repeat_interleave(f, dim=2)
        total = m if total is None else total + m
    return total / float(len(maps))


def word_map_reference(collect: Callable[[torch.Tensor, int], Dict[int, torch.Tensor]], space: NoiseSpace, draws: int = 8) -> torch.Tensor:
    """SliderEditor.word_map over a callable collect(x_bf16, t) -> {factor: [bs][T_level]}: the inversion's own latents at `draws` evenly
    spaced steps of the whole grid, level_mean per draw, then the mean over the draws in grid order"""
    if space.visited is None:
        raise ValueError("word_map_reference: the NoiseSpace carries no visited latents")
    idx = footprint_draws(space.timesteps, space.timesteps[0], draws, 0)
    h, w = space.x_start.shape[-2:]
    total = None
    for i in idx:
        x = space.x_start if i == 0 else space.visited[i - 1]
        m = level_mean(collect(x.to(torch.bfloat16), space.timesteps[i]), h, w)
        total = m if total is None else total + m
    return total / float(len(idx))


# ---------------------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------------------
class _SpaceSource:
    """A NoiseSpace as the source of SliderSampler._footprint / _word_map: the grid, the UNet input at step i (the inversion's own
    latents), the conditioning and the guidance"""

    def __init__(self, editor: "SliderEditor", space: NoiseSpace):
        dev = editor.eng.device
        self.visited = editor.trajectory(space).visited.to(dev, torch.float32)
        self.x_start = space.x_start.to(dev, torch.float32)
        self.timesteps, self.guidance = space.timesteps, space.guidance
        self.ctx, self.pooled, self.time_ids = space.ctx, space.pooled, space.time_ids

    def unet_input(self, i: int) -> torch.Tensor:
        return self.x_start if i == 0 else self.visited[i - 1]


class SliderEditor(SliderSampler):
    """SliderSampler (same constructor; the scheduler must be DDIM) that also inverts a given image's latents into a NoiseSpace and
    edits them.  With store= the inversion and the edit replay the adapter program ("on", multiplier 0 resp. `scale`); with sliders=
    or no slider the adapter-free one, the edit on merged weights below start_noise."""

    def __init__(self, engine, store=None, decoder=None, prediction_type: str = "epsilon", scheduler: str = "ddim",
                 scheduler_seed: int = 0, sliders=None):
        if scheduler.lower().replace(" ", "_") != "ddim":
            raise ValueError(f"SliderEditor: scheduler {scheduler!r}: the DDPM noise space is defined on the DDIM grid")
        super().__init__(engine, store, decoder, prediction_type, "ddim", scheduler_seed, sliders)

    def _pass(self, bs: int, h: int, w: int, ctx, pooled, time_ids, attn_maps=None) -> Pass:
        """the CFG-pair plan of this shape with its conditioning written; attn_maps: the plan of the shape that also records attention
        maps (UNetEngine.plan)"""
        drv = Pass(self.eng, self.eng.plan(2 * bs, h, w, "on" if self.store is not None else "off", attn_maps=attn_maps))
        drv.load_cond(ctx, pooled, time_ids)
        return drv

    def _launch_step(self, p, t, steps, eta, guidance, src, dst, resid_i, target=None, keep=None, mask=None, eps_text=0, hist=None,
                     t_older=None):
        """The step's one element-wise launch after the UNet pass, src -> dst (fp32, may be one tensor) and the bf16 halves of `sample`:
        slh_ddpm_edit_step - mode 0 with a target (resid_i written), else mode 1 (resid_i read) - or, with a mask, slh_ddpm_edit_blend
        against keep.  eps_text: the address of a text row to read in place of the one behind the unconditional half (a direction
        step's guided row; p is then the wide plan, whose first two row blocks are the pair's).
        hist (fp32, src's shape: a second-order chain): the launch is slh_edit_step2 in all these forms; it reads the chain's x0h of
        the step from t_older out of hist where the step is second order (`ddpm_step2_coefficients`) and leaves its own x0h there."""
        io, bs, chw = p.io, src.shape[0], src[0].numel()
        smp = io["sample"]
        common = dict(eps=io["eps"].ptr, eps_text=eps_text, x=src.data_ptr(), resid=resid_i.data_ptr(), out=dst.data_ptr(), out_bf16=smp.ptr,
                      out2_bf16=smp.ptr + bs * chw * 2, nb=bs, chw=chw, guidance=float(guidance),
                      v_prediction=1 if self.sched.prediction_type == "v_prediction" else 0)
        s = torch.cuda.current_stream().cuda_stream
        if hist is not None:
            coef = fp32_coefficients(ddpm_step2_coefficients(self.sched, t, steps, eta, t_older))
            lib.edit_step2(s, x0_prev=hist.data_ptr() if "c_corr" in coef else 0, x0_out=hist.data_ptr(), hw=chw // src.shape[1],
                           target=0 if target is None else target.data_ptr(), mode=0 if target is not None else 1,
                           keep=0 if mask is None else keep.data_ptr(), mask=0 if mask is None else mask.data_ptr(), **common, **coef)
            return
        common.update(fp32_coefficients(ddpm_step_coefficients(self.sched, t, steps, eta)))
        if mask is None:
            d = lib.DdpmEditDesc(target=0 if target is None else target.data_ptr(), mode=0 if target is not None else 1, **common)
            lib.call(lib.OP_DDPM_EDIT, d, s)
        else:
            d = lib.DdpmEditBlendDesc(keep=keep.data_ptr(), mask=mask.data_ptr(), hw=chw // src.shape[1], **common)
            lib.call(lib.OP_DDPM_EDIT_BLEND, d, s)

    def _chain(self, drv: Pass, x, ts, steps, eta, guidance, scale, start_noise, resid, path=None, x0=None, record=None, keep=None,
               mask=None, guide=None, order=1):
        """x (fp32) through the grid; returns the final latent.  path given = invert (resid written), else edit (resid read).
        record None: x is updated in place.  record [len(ts)][bs][4][h][w]: the same launches, but step i reads record[i - 1] (x for
        i = 0) and writes record[i], so the chain's latents are kept (the inversion, `trajectory`).
        mask [bs][1][h][w] with keep = the inversion's latents: every step is blended against keep[i] (in place).
        The slider is the sampler's (slider_session), except that a multiplier of 0 means the inversion's pass: at scale 0 nothing is
        merged, sliders held at a fixed scale included (they belong to the edit, and scale 0 is the reconstruction).
        guide (DirectionGuide, an edit only): the steps with t > start_noise are the launches above; at the first live step the pass
        moves to the wide plan - the bf16 rounding of the fp32 master, which is what the step before wrote as the plain plan's input,
        into every row block, and the full program, since the direction rows' cross-attention K/V were never projected - and from
        there on every step is wide replay -> guide.guide -> the same step launch reading the guided text row and writing the wide
        plan's first two row blocks -> guide.spread.
        order 2: the launches are slh_edit_step2 over one fp32 history buffer of this chain's own (x0h of the step before, updated in
        place; it belongs to no plan, so the move to the wide plan leaves it as it is)."""
        drv.load_latents(x)
        hist = torch.empty_like(x) if check_order(order) == 2 else None
        s = torch.cuda.current_stream().cuda_stream
        with self.slider_session(scale, start_noise, zero_merges=False) as gate:
            for i, t in enumerate(ts):
                src, dst = (x, x) if record is None else (x if i == 0 else record[i - 1], record[i])
                first, wide = i == 0, guide is not None and guide.live(t)
                if wide and not guide.entered:
                    drv, first = guide.enter(), True
                    drv.load_latents(src)
                drv.run(t, gate(t, first), s)
                target = None if path is None else (path[i + 1] if i + 1 < len(ts) else x0)
                self._launch_step(drv.p, t, steps, eta, guidance, src, dst, resid[i], target, None if mask is None else keep[i], mask,
                                  eps_text=guide.guide(s) if wide else 0, hist=hist, t_older=ts[i - 1] if i > 0 else None)
                if wide:
                    guide.spread()
        return x if record is None else record[-1].clone()

    @torch.no_grad()
    def invert(self, ctx: torch.Tensor, x0_latents: torch.Tensor, steps: int = 50, skip: Optional[int] = None, eta: float = 1.0,
               guidance_scale: float = 7.5, seed: int = 0, pooled: Optional[torch.Tensor] = None,
               time_ids: Optional[torch.Tensor] = None, order: int = 1) -> NoiseSpace:
        """ctx: (2*bs, 77, D) = cat([unconditional, text]); x0_latents: (bs, 4, h, w) = scaling_factor * posterior mean of the image
        (VaeEncoder.get_noisy_image's third output with zero noises).  2 * len(grid) launches besides the UNet replays.
        order 2: the second-order noise space (docs/EDIT.md; slh_edit_step2 in place of slh_ddpm_edit_step); every edit of the
        returned space reads its order."""
        check_order(order)
        ts = edit_timesteps(self.sched, steps, skip)
        ddpm_step_coefficients(self.sched, ts[0], steps, eta)          # validates eta before anything runs
        dev = self.eng.device
        x0 = x0_latents.detach().to(dev, torch.float32).contiguous()
        bs, _, h, w = x0.shape
        drv = self._pass(bs, h, w, ctx, pooled, time_ids)
        path = build_path(self.sched, x0, ts, seed)
        resid, visited = torch.empty_like(path), torch.empty_like(path)
        x = self._chain(drv, path[0].clone(), ts, steps, eta, guidance_scale, 0.0, -1, resid, path, x0, record=visited, order=order)
        return NoiseSpace(x0=x0, x_start=path[0].clone(), resid=resid, recon=x, timesteps=list(ts), steps=int(steps),
                          skip=steps - len(ts), eta=float(eta), guidance=float(guidance_scale),
                          prediction_type=self.sched.prediction_type, seed=int(seed), ctx=ctx.detach().clone(),
                          pooled=None if pooled is None else pooled.detach().clone(),
                          time_ids=None if time_ids is None else time_ids.detach().clone(), visited=visited, order=int(order))

    def _check_prediction(self, space: NoiseSpace):
        if space.prediction_type != self.sched.prediction_type:
            raise ValueError(f"the NoiseSpace was inverted with {space.prediction_type}, this editor predicts {self.sched.prediction_type}")

    @staticmethod
    def _check_conditioning(space: NoiseSpace, what: str):
        if space.ctx is None:
            raise ValueError(f"{what}: this NoiseSpace carries no conditioning (set space.ctx to the inversion's)")

    @torch.no_grad()
    def trajectory(self, space: NoiseSpace) -> NoiseSpace:
        """Fills space.visited where it is missing (a file saved before masked edits) by one scale-0 replay with the inversion's
        conditioning and guidance - the inversion's latents again, bit for bit, by the identity the whole method rests on; raises if
        the replay does not end on space.recon (other weights, another engine: its latents are then not this inversion's)."""
        if space.visited is not None:
            return space
        self._check_prediction(space)
        self._check_conditioning(space, "trajectory")
        dev = self.eng.device
        x = space.x_start.to(dev, torch.float32).clone().contiguous()
        resid = space.resid.to(dev, torch.float32).contiguous()
        bs, _, h, w = x.shape
        drv = self._pass(bs, h, w, space.ctx, space.pooled, space.time_ids)
        visited = torch.empty_like(resid)
        end = self._chain(drv, x, space.timesteps, space.steps, space.eta, space.guidance, 0.0, -1, resid, record=visited, order=space.order)
        if not torch.equal(end, space.recon.to(dev)):
            raise RuntimeError("trajectory: the scale-0 replay does not end on space.recon bit for bit: this NoiseSpace was not inverted "
                               "with these weights and this conditioning")
        space.visited = visited.to(space.recon.device)
        return space

    @torch.no_grad()
    def edit_latents(self, space: NoiseSpace, ctx: Optional[torch.Tensor] = None, scale: float = 0.0, start_noise: int = 750,
                     guidance_scale: Optional[float] = None, pooled: Optional[torch.Tensor] = None,
                     time_ids: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                     directions: Optional[DirectionSet] = None, direction_quantile: float = 0.0,
                     direction_momentum: Optional[Tuple[float, float]] = None) -> torch.Tensor:
        """-> the edited latents (bs, 4, h, w) fp32.  ctx / guidance_scale None: the inversion's own - then scale 0 returns
        space.recon bit for bit.  Another prompt or guidance is an edit of its own; no reconstruction claim applies.
        mask ([h][w], [bs][h][w] or [bs][1][h][w], values in [0, 1], 1 = edit): every step is blended against the inversion's latent
        after that step, so where the mask is 0 the result is space.recon bit for bit - at any scale, prompt or guidance.
        directions / direction_quantile / direction_momentum: as SliderSampler.sample_latents, with the coefficients of the CFG pair at
        this edit's guidance; `scale` drives them and store= / sliders= alike.  Where they do not act - scale 0, or no step of the grid
        with t <= start_noise - nothing of them is built or launched: the chain is the one without them."""
        self._check_prediction(space)
        if ctx is None:
            self._check_conditioning(space, "edit_latents without ctx")
            ctx = space.ctx
            pooled = space.pooled if pooled is None else pooled
            time_ids = space.time_ids if time_ids is None else time_ids
        dev = self.eng.device
        x = space.x_start.to(dev, torch.float32).clone().contiguous()
        resid = space.resid.to(dev, torch.float32).contiguous()
        bs, _, h, w = x.shape
        visited = None
        if mask is not None:
            mask = as_mask(mask, bs, h, w).to(dev)
            visited = self.trajectory(space).visited.to(dev, torch.float32).contiguous()
        g = space.guidance if guidance_scale is None else guidance_scale
        guide = None
        if directions is not None:
            DirectionSet.n_keep(h * w, direction_quantile)          # (argument errors, whether or not the directions act)
            check_momentum(direction_momentum)
            coef = directions.coefficients(scale, g, single=False)
            if any(c != 0.0 for c in coef) and any(not float(t) > start_noise for t in space.timesteps):
                guide = DirectionGuide(self.eng, directions, coef, direction_quantile, "on" if self.store is not None else "off", bs, h, w,
                                       False, ctx, pooled, time_ids, start_noise, momentum=direction_momentum)
        elif direction_momentum is not None:
            raise ValueError("edit_latents: direction_momentum without directions")
        drv = self._pass(bs, h, w, ctx, pooled, time_ids)
        return self._chain(drv, x, space.timesteps, space.steps, space.eta, g, scale, start_noise, resid, keep=visited, mask=mask, guide=guide,
                           order=space.order)

    @torch.no_grad()
    def footprint(self, space: NoiseSpace, scale: float, start_noise: int = 750, draws: int = 8, t_min: int = 200,
                  directions: Optional[DirectionSet] = None, direction_quantile: float = 0.0, guidance_scale: Optional[float] = None) -> torch.Tensor:
        """Where the slider acts on this image: F [bs][h][w] fp32 = the mean over `draws` noise levels of
        sum_c |eps(slider at `scale`) - eps(slider off)| (slh_eps_absdiff), each draw divided by its mean over the pixels - DiffEdit's
        contrast (Couairon et al. 2022) with the slider in place of the second prompt.  The UNet inputs are the inversion's own at
        those levels (x_start / visited[i - 1]: the image under independent noise draws), conditioning and guidance the inversion's.
        All slider-off passes run first, then the slider is switched on once (store=: the multiplier; sliders=: one merge, full
        program on the first pass after it) for the slider-on passes: 2 * len(draws) UNet passes.
        directions (with direction_quantile; guidance_scale None: the inversion's): where the prompt directions act instead.  One wide
        pass per draw gives u, t and the pairs' rows; with t' the guided text row of a direction step at `scale` (no momentum: a draw
        is not a chain) the map is slh_eps_absdiff of (u, t') against (u, t) = sum_c |g (t' - t)|, what the step would see differently:
        len(draws) UNet passes."""
        self._check_prediction(space)
        self._check_conditioning(space, "footprint")
        footprint_draws(space.timesteps, start_noise, draws, t_min)          # the grid's errors before the trajectory is replayed
        return self._footprint(_SpaceSource(self, space), scale, start_noise, draws, t_min, directions, direction_quantile, guidance_scale)

    @torch.no_grad()
    def word_map(self, space: NoiseSpace, tokens: Optional[Sequence[int]] = None, weights: Optional[torch.Tensor] = None, draws: int = 8,
                 max_factor: int = 4) -> torch.Tensor:
        """Where words of the inversion's prompt live on this image: F [bs][h][w] fp32 = the mean over `draws` evenly spaced steps of
        the whole grid of the mean over the collected levels of the UNet's cross-attention probabilities on the chosen keys
        (slh_xattn_map behind every attn2 whose tokens are the latent grid divided by <= max_factor; heads and layers of a level
        averaged, a level replicated to the latent grid).  tokens: key positions (BOS = 0, `word_token_indices`), or weights
        [bs][ctx_len].  Inputs, conditioning and guidance are the footprint's - the inversion's own - and the slider is off
        (multiplier 0, or the base weights with sliders=): len(draws) UNet passes of the maps plan, half of the footprint's, and
        none of them depends on a slider.  The edit's own plans are not touched; the next chain starts with its full program."""
        self._check_prediction(space)
        self._check_conditioning(space, "word_map")
        footprint_draws(space.timesteps, space.timesteps[0], draws, 0)
        return self._word_map(_SpaceSource(self, space), tokens, weights, draws, max_factor)

    @torch.no_grad()
    def edit(self, space: NoiseSpace, **kw) -> torch.Tensor:
        """-> uint8 images [bs][H][W][3] (needs a VaeDecoder); the arguments of edit_latents, mask= included."""
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
    p.add_argument("--inversion", "--load_inversion", default=None, help="edit a saved NoiseSpace instead of inverting --image")
    p.add_argument("--order", type=int, choices=[1, 2], default=None,
                   help="order of the inversion's solver (default 1; 2: the second-order noise space, for coarser grids); stored by "
                        "--save_inversion, and not given with --inversion: the file decides")
    p.add_argument("--res", type=int, default=None)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--out", default="edited")
    p.add_argument("--mask", default=None, help="localise the edits: an image file, white = edit, black = keep the reconstruction bit for bit")
    p.add_argument("--mask_invert", action="store_true", help="with --mask: black = edit")
    p.add_argument("--mask_feather", type=float, default=None, metavar="SIGMA",
                   help="Gaussian feathering of the mask in latent pixels (default 0 with --mask, 1 with --auto_mask)")
    p.add_argument("--auto_mask", action="store_true", help="localise the edits to the slider's own footprint on this image")
    p.add_argument("--auto_mask_scale", type=float, default=None, help="slider scale the footprint is measured at (default: the largest |scale| of --scales)")
    p.add_argument("--auto_mask_draws", type=int, default=None, help="noise levels the footprint averages over (default 8)")
    p.add_argument("--auto_mask_threshold", type=float, default=None, help="binarisation threshold of the footprint (default 0.5)")
    p.add_argument("--auto_mask_dilate", type=int, default=None, help="latent pixels the binary footprint is grown by (default 1)")
    p.add_argument("--mask_word", action="append", default=[], metavar="WORD",
                   help="localise the edits to where this word of --prompt lives in the cross-attention; repeatable (needs the model's tokenizer)")
    p.add_argument("--mask_tokens", default=None, metavar="I,J,...", help="the same from key positions of the prompt (BOS = 0)")
    p.add_argument("--mask_word_threshold", type=float, default=None, help="binarisation threshold of the word map / its maximum (default 0.3)")
    p.add_argument("--mask_word_draws", type=int, default=None, help="steps of the grid the word map averages over (default 8)")
    p.add_argument("--save_attention", default=None, help="write the word map / its maximum here (8-bit PNG at latent resolution)")
    p.add_argument("--save_mask", default=None, help="write the latent-resolution mask here (8-bit PNG)")
    # prompt-direction edits (docs/EDIT.md): the options of sliders_amd.generate, --scales sweeps the direction's strength
    p.add_argument("--direction", action="append", default=[], metavar="POSITIVE|NEGATIVE[:ETA]",
                   help="edit along eps(POSITIVE) - eps(NEGATIVE), times ETA (default 1) times the scale; repeatable, at most 3")
    p.add_argument("--direction_file", default=None, help="the same from a prompts.yaml of the trainers: positive, unconditional, guidance_scale "
                                                          "(ETA) and action (erase: the opposite sign) of its entries")
    p.add_argument("--direction_entries", default=None, metavar="I,J,...", help="entries of --direction_file to take (default: all, at most 3)")
    p.add_argument("--direction_quantile", type=float, default=None, metavar="Q",
                   help="keep only the largest 1 - Q of each latent channel's differences (default 0: all of them)")
    p.add_argument("--direction_momentum", default=None, metavar="S_M[:BETA]",
                   help="SEGA's momentum on the direction: strength S_M, decay BETA (default 0.4); 0: none")
    return p


def check_args(a):
    """every argument error, before any model is built"""
    if a.inversion and a.save_inversion:
        raise SystemExit("--inversion reads a saved inversion, --save_inversion writes one: give one of them")
    if a.inversion and a.order is not None:
        raise SystemExit("--order belongs to the inversion: a saved one (--inversion) carries its own")
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
    from .generate import check_direction_args
    g = a.guidance_scale if a.edit_guidance_scale is None else a.edit_guidance_scale
    check_direction_args(a, no_cfg=False, guidance_scale=g, guidance_option="--edit_guidance_scale" if a.edit_guidance_scale is not None
                         else "--guidance_scale")
    check_mask_args(a, scales, lambda: edit_timesteps(DDIMSchedule(), a.steps, skip))
    return scales


def check_mask_args(a, scales: List[float], grid: Callable[[], List]):
    """the argument errors of the mask options (shared with sliders_amd.generate); grid() -> the timesteps the run will visit"""
    word = bool(a.mask_word) or a.mask_tokens is not None
    if sum([bool(a.mask), bool(a.auto_mask), bool(a.mask_word), a.mask_tokens is not None]) > 1:
        raise SystemExit("--mask reads a mask, --auto_mask derives one from the slider, --mask_word / --mask_tokens from the prompt: give one of them")
    if a.mask_word and a.synthetic:
        raise SystemExit("--mask_word needs the model's tokenizer: with --synthetic give key positions (--mask_tokens)")
    if a.mask_tokens is not None:
        try:
            a.mask_token_list = [int(v) for v in a.mask_tokens.split(",")]
        except ValueError:
            raise SystemExit(f"--mask_tokens {a.mask_tokens!r}: expected comma-separated key positions")
        if not a.mask_token_list or min(a.mask_token_list) < 0 or max(a.mask_token_list) > 76:
            raise SystemExit(f"--mask_tokens {a.mask_tokens!r}: expected key positions in 0 .. 76")
    if not word and (a.mask_word_threshold is not None or a.mask_word_draws is not None or a.save_attention):
        raise SystemExit("--mask_word_threshold / --mask_word_draws / --save_attention need --mask_word or --mask_tokens")
    if a.mask_word_threshold is not None and not 0.0 < a.mask_word_threshold <= 1.0:
        raise SystemExit(f"--mask_word_threshold {a.mask_word_threshold}: expected 0 < threshold <= 1")
    if a.mask_word_draws is not None and a.mask_word_draws < 1:
        raise SystemExit(f"--mask_word_draws {a.mask_word_draws}: expected at least 1")
    if a.mask and not os.path.isfile(a.mask):
        raise SystemExit(f"--mask {a.mask}: no such file")
    if a.mask_invert and not (a.mask or a.mask_word or a.mask_tokens is not None):
        raise SystemExit("--mask_invert needs --mask (or --mask_word / --mask_tokens)")
    if not (a.mask or a.auto_mask or word) and (a.mask_feather is not None or a.save_mask):
        raise SystemExit("--mask_feather / --save_mask need --mask, --auto_mask, --mask_word or --mask_tokens")
    if a.mask_feather is not None and not 0.0 <= a.mask_feather < float("inf"):
        raise SystemExit(f"--mask_feather {a.mask_feather}: expected a finite sigma >= 0")
    given = [n for n in ("scale", "draws", "threshold", "dilate") if getattr(a, "auto_mask_" + n) is not None]
    if given and not a.auto_mask:
        raise SystemExit("--auto_mask_" + given[0] + " needs --auto_mask")
    if a.auto_mask:
        if not a.lora_weight and not a.compose and not (getattr(a, "direction", None) or getattr(a, "direction_file", None)):
            raise SystemExit("--auto_mask is the slider's footprint: it needs --lora_weight (or --compose)")
        if a.auto_mask_scale is None:
            a.auto_mask_scale = max(scales, key=abs)
        if a.auto_mask_scale == 0.0:
            raise SystemExit("--auto_mask: the footprint is measured at a non-zero scale (--auto_mask_scale, or a non-zero entry of --scales)")
        if a.auto_mask_draws is not None and a.auto_mask_draws < 1:
            raise SystemExit(f"--auto_mask_draws {a.auto_mask_draws}: expected at least 1")
        if a.auto_mask_threshold is not None and not 0.0 < a.auto_mask_threshold <= 1.0:
            raise SystemExit(f"--auto_mask_threshold {a.auto_mask_threshold}: expected 0 < threshold <= 1")
        if a.auto_mask_dilate is not None and a.auto_mask_dilate < 0:
            raise SystemExit(f"--auto_mask_dilate {a.auto_mask_dilate}: expected >= 0")
        try:
            footprint_draws(grid(), a.start_noise, a.auto_mask_draws or 8)
        except ValueError as e:
            raise SystemExit(f"--auto_mask: {e}")


def _suffixed(path: str, suffix: str) -> str:
    root, ext = os.path.splitext(path)
    return root + suffix + ext


def mask_from_args(a, ed, src, res: int, prompt: str, tokenizer, suffix: str = "", **steer):
    """The mask the command line asks for, or None: from the file (--mask), from the slider's footprint (--auto_mask: ed.footprint over
    src; steer: directions= / direction_quantile= / guidance_scale= - the footprint is then the directions') or from the prompt's words
    (--mask_word / --mask_tokens: ed.word_map over src); --save_attention and --save_mask are written here (suffix: put in front of
    their extensions).  ed / src: a SliderEditor and its NoiseSpace, or a SliderSampler and a SampleTrace.
    res: the image size the latents decode to."""
    from PIL import Image
    mask = None
    if a.mask:
        mask = feather_mask(load_mask(a.mask, res, a.mask_invert), a.mask_feather or 0.0)
    elif a.auto_mask:
        try:          # (check_args tried the grid of the command line; a saved inversion brings its own)
            F = ed.footprint(src, a.auto_mask_scale, start_noise=a.start_noise, draws=a.auto_mask_draws or 8, **steer)
            mask = footprint_mask(F.cpu(), threshold=0.5 if a.auto_mask_threshold is None else a.auto_mask_threshold,
                                  dilate=1 if a.auto_mask_dilate is None else a.auto_mask_dilate,
                                  feather=1.0 if a.mask_feather is None else a.mask_feather)
        except ValueError as e:
            raise SystemExit(f"--auto_mask: {e}")
    elif a.mask_word or a.mask_tokens is not None:
        try:
            tokens = sorted({i for wd in a.mask_word for i in word_token_indices(prompt, wd, tokenizer, ed.eng.ctx_len)}) if a.mask_word \
                else a.mask_token_list
            F = ed.word_map(src, tokens=tokens, draws=a.mask_word_draws or 8).cpu()
            mask = word_mask(F, threshold=0.3 if a.mask_word_threshold is None else a.mask_word_threshold,
                             feather=1.0 if a.mask_feather is None else a.mask_feather)
        except ValueError as e:
            raise SystemExit(f"--mask_word / --mask_tokens: {e}")
        if a.mask_invert:
            mask = 1.0 - mask
        print(f"word map over key positions {tokens}: maximum {float(F.max()):.4f}")
        if a.save_attention:
            a8 = (F[0] / F[0].max() * 255.0).round().to(torch.uint8)
            Image.fromarray(a8.numpy()).save(_suffixed(a.save_attention, suffix))
            print(f"attention saved to {_suffixed(a.save_attention, suffix)}")
    if a.save_mask:
        m8 = (mask.reshape(mask.shape[-2:]) * 255.0).round().to(torch.uint8)
        Image.fromarray(m8.cpu().numpy()).save(_suffixed(a.save_mask, suffix))
        print(f"mask saved to {_suffixed(a.save_mask, suffix)}: mean {float(mask.mean()):.3f}")
    return mask


def main(argv=None):
    a = build_parser().parse_args(argv)
    scales = check_args(a)
    tokenizer = None
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
    from .generate import direction_set, direction_specs
    specs = direction_specs(a)
    if a.synthetic:
        eng = synthetic_engine(a.model, dev, a.seed)
        vae_sd = random_vae_state_dict(device=dev, seed=a.seed, decoder=True)
        g = torch.Generator().manual_seed(a.seed)
        cond = []
        for _ in prompts:            # a prompt is a draw: the first is the image's, the second the edit's
            cond.append((torch.randn(2, 77, eng.cfg.cross_attention_dim, generator=g),
                         torch.randn(2, eng.cfg.pooled_dim, generator=g) if xl else None))
        encode = None
    else:
        from safetensors.torch import load_file
        from . import model_util
        eng = load_unet_engine(a.model_path, dev)
        vae_sd = load_file(os.path.join(a.model_path, "vae", "diffusion_pytorch_model.safetensors"))
        cond = []
        if xl:
            toks, encs = model_util.load_text_encoders_xl(a.model_path, dev, torch.bfloat16)
            tokenizer = toks[0]
            for pr in prompts:
                (e_u, p_u), (e_t, p_t) = (model_util.encode_prompts_xl(toks, encs, [s]) for s in ("", pr))
                cond.append((torch.cat([e_u, e_t]), torch.cat([p_u, p_t])))
            encode = lambda text: model_util.encode_prompts_xl(toks, encs, [text])
        else:
            tok, enc = model_util.load_text_encoder(a.model_path, dev, torch.bfloat16)
            tokenizer = tok
            for pr in prompts:
                cond.append((torch.cat([model_util.encode_prompts(tok, enc, [s]) for s in ("", pr)]), None))
            encode = lambda text: (model_util.encode_prompts(tok, enc, [text]), None)
    steer = direction_set(a, specs, encode, eng.cfg, xl)
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
        space = ed.invert(ctx, x0, steps=a.steps, skip=a.skip, eta=a.eta, guidance_scale=a.guidance_scale, seed=a.seed, pooled=pooled,
                          order=a.order or 1)
        if a.save_inversion:
            space.save(a.save_inversion)
            print(f"inversion saved to {a.save_inversion}")
    os.makedirs(a.out, exist_ok=True)
    Image.fromarray(VaeDecoder.to_uint8(dec.decode(space.recon))[0].cpu().numpy()).save(os.path.join(a.out, "recon.png"))
    kw = dict(start_noise=a.start_noise, guidance_scale=a.edit_guidance_scale, **steer)
    foot = {k: v for k, v in steer.items() if k != "direction_momentum"}
    if foot:
        foot["guidance_scale"] = a.edit_guidance_scale
    mask = mask_from_args(a, ed, space, 8 * space.x0.shape[-1], a.prompt, tokenizer, **foot)    # a saved inversion: its size
    if mask is not None:
        kw["mask"] = mask
    if a.edit_prompt is not None:
        kw.update(ctx=cond[1][0].to(dev), pooled=None if cond[1][1] is None else cond[1][1].to(dev))
    for s in scales:
        img = ed.edit(space, scale=s, **kw)
        Image.fromarray(img[0].cpu().numpy()).save(os.path.join(a.out, f"scale_{s:g}.png"))
        print(f"scale {s:g}: saved {os.path.join(a.out, f'scale_{s:g}.png')}")
    return a.out


if __name__ == "__main__":
    main()
