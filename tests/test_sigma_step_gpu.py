"""The fused fp32 sampler step on the MI355X (docs/SAMPLING.md, "Fused fp32 step"):

kernel   slh_sigma_step over the case matrix, every fp32 output within the derived bound of float64 (tests/sigma_step_ref.py), the
         exact identities with torch.equal, fenced NaN-prefilled buffers;
engine   SliderSampler(latents="fp32") for euler / euler_a / lms / ddpm against the fp32 reference loop, under the project's 3e-2
         ceiling and within 1.25 x of what today's bf16 path reaches on the same inputs; dpmpp_2m against the float64 lambda-form
         oracle; the launch shape; merged sliders; the bf16 path's bits;
cli      generate --scheduler dpmpp_2m and --fp32_latents.
"""
import itertools
import math
import os
import random

import pytest
import torch

from oracle.lora_oracle import LoRANetworkOracle
from oracle.unet_oracle import build_unet
from sliders_amd import lib, schedulers
from sliders_amd.config import CONFIGS
from sliders_amd.passes import Pass
from sliders_amd.sampler import SliderSampler
from sliders_amd.schedulers import StepRow
from sliders_amd.unet import UNetEngine
from tests.sigma_step_ref import bound, dpmpp_2m_oracle, worst_ratio
from tests.test_fewstep_sampler_gpu import HW, _bf16_valued, _inputs, _time_ids, tiny  # noqa: F401  (tiny: the module's fixture)
from tests.util import rel_err

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements of NaN in front of and behind every buffer
F32 = ("x", "h1", "h2", "h3", "noise", "out", "hist_out")
BF16 = ("eps", "eps_text", "in1", "in2")


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _row(kind, pred, n_hist, sigma, seed):
    """a row with the magnitudes of the schedulers' rows at this sigma, fp32-valued"""
    g = torch.Generator().manual_seed(seed)
    s1 = 0.6 * sigma
    p, q = (1 / (sigma ** 2 + 1), -sigma / math.sqrt(sigma ** 2 + 1)) if pred == "v" else (1.0, -sigma)
    c = (torch.randn(n_hist + 1, generator=g) * (sigma if kind == 0 else 1.0)).tolist()
    return StepRow(kind, _f32(p), _f32(q), _f32(sigma), 1.0 if kind == 0 else _f32(s1 / sigma), [_f32(v) for v in c], _f32(0.5 * sigma),
                   _f32(1 / math.sqrt(s1 ** 2 + 1)))


class Buffers:
    """Every buffer of one call inside two NaN-prefilled device tensors (one row per buffer, GUARD elements in front and behind; the
    rows are 16-byte aligned, so whether the kernel takes its four-element form depends on n alone), and their host images."""

    def __init__(self, dev, n, form, inputs, seed):
        g = torch.Generator().manual_seed(seed)
        self.n, self.form = n, form
        r = lambda m=n: torch.randn(m, generator=g)
        big = 1e3 if inputs == "large" else 1.0
        eps_rows = n if form == "single" else 2 * n
        eps = r(2 * n)[:eps_rows].to(torch.bfloat16)
        if inputs == "zero_eps":
            eps = torch.zeros_like(eps)
        vals32 = {"x": r() * big, "h1": r() * big, "h2": r() * big, "h3": r() * big, "noise": r()}
        vals16 = {"eps": eps[:n] if form == "eps_text" else eps, "eps_text": eps[n:] if form == "eps_text" else None}
        self.u, self.t = eps[:n], (None if form == "single" else eps[n:])
        self.L32, self.L16 = 2 * GUARD + (n + 3) // 4 * 4, 2 * GUARD + (2 * n + 7) // 8 * 8
        self.h32 = torch.full((len(F32), self.L32), float("nan"))
        self.h16 = torch.full((len(BF16), self.L16), float("nan"), dtype=torch.bfloat16)
        for k, name in enumerate(F32):
            if vals32.get(name) is not None:
                self.h32[k, GUARD:GUARD + n] = vals32[name]
        for k, name in enumerate(BF16):
            if vals16.get(name) is not None:
                self.h16[k, GUARD:GUARD + len(vals16[name])] = vals16[name]
        self.vals32 = vals32
        self.d32, self.d16 = self.h32.to(dev), self.h16.to(dev)

    def ptr(self, name):
        if name in F32:
            return self.d32[F32.index(name)].data_ptr() + GUARD * 4
        return self.d16[BF16.index(name)].data_ptr() + GUARD * 2

    def fetch(self):
        return self.d32.cpu(), self.d16.cpu()


def _launch(b, row, nb, chw, noise, guidance=7.5, out="out", hist_out="hist_out", in2=True):
    lib.sigma_step(torch.cuda.current_stream().cuda_stream, eps=b.ptr("eps"), x=b.ptr("x"), out=b.ptr(out), nb=nb, chw=chw, kind=row.kind,
                   p=row.p, q=row.q, sigma=row.sigma, a=row.a, c=row.c, c_n=row.c_n, s_next=row.s_next, guidance=guidance,
                   single=b.form == "single", eps_text=b.ptr("eps_text") if b.form == "eps_text" else 0,
                   hist=[b.ptr(f"h{k}") for k in range(1, row.n_hist + 1)], noise=b.ptr("noise") if noise else 0,
                   hist_out=b.ptr(hist_out) if hist_out else 0, in_bf16=b.ptr("in1"), in2_bf16=b.ptr("in2") if in2 else 0)
    torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _check_fences(b, got32, got16, written32, written16):
    """everything but the written windows has the bits it had: the inputs, the unused buffers, every guard"""
    n = b.n
    want32, want16 = b.h32.clone(), b.h16.clone()
    for name in written32:
        want32[F32.index(name), GUARD:GUARD + n] = got32[F32.index(name), GUARD:GUARD + n]
    for name in written16:
        want16[BF16.index(name), GUARD:GUARD + n] = got16[BF16.index(name), GUARD:GUARD + n]
    assert torch.equal(_bits(got32), _bits(want32)) and torch.equal(_bits(got16), _bits(want16)), "an input or a fence was written"


# chw: one pixel, a tail that is no multiple of 8, an exact multiple, the 33^2 tail - and two that are no multiple of 4: 5 (nothing but
# the one-element form) and 1023 (a tail behind the four-element form; as a pair without eps_text its text half is not 8-byte aligned
# and the whole range takes the one-element form)
MATRIX = list(itertools.product((1, 2), (4, 900, 1024, 4356, 5, 1023), (0, 1), (0, 1, 2, 3), (False, True), ("pair", "eps_text", "single"),
                                ("unit", "large", "zero_eps")))


def test_kernel_matrix(dev):
    worst = {"out": 0.0, "hist_out": 0.0, "in": 0.0}
    pick = random.Random(0)
    for idx, (nb, chw, kind, n_hist, noise, form, inputs) in enumerate(MATRIX):
        # epsilon / v prediction and the step's place on the grid are values of p, q, sigma to the kernel: drawn per case
        pred, sigma = pick.choice(("eps", "v")), pick.choice((14.6, 1.3, 0.03))
        n = nb * chw
        row = _row(kind, pred, n_hist, sigma, seed=idx)
        b = Buffers(dev, n, form, inputs, seed=1000 + idx)
        _launch(b, row, nb, chw, noise)
        got32, got16 = b.fetch()
        _check_fences(b, got32, got16, ("out", "hist_out"), ("in1", "in2"))
        win = lambda t, names, name: t[names.index(name), GUARD:GUARD + n]
        out, hist = win(got32, F32, "out"), win(got32, F32, "hist_out")
        H = [b.vals32[f"h{k}"] for k in (1, 2, 3)]
        ref, bnd = bound(b.u, b.t, b.vals32["x"], H, b.vals32["noise"] if noise else None, row, 7.5)
        tag = (nb, chw, kind, n_hist, noise, form, inputs, pred)
        for name, g_, r_, b_ in (("out", out, ref[0], bnd[0]), ("hist_out", hist, ref[1], bnd[1])):
            ratio = worst_ratio(g_, r_, b_)
            assert ratio <= 1.0, (name, ratio, tag)
            worst[name] = max(worst[name], ratio)
        # the bf16 copies are the rounding of the kernel's own fp32 out, scaled: exact
        want_in = (out * row.s_next).to(torch.bfloat16)
        assert torch.equal(_bits(win(got16, BF16, "in1")), _bits(want_in)) and torch.equal(_bits(win(got16, BF16, "in2")), _bits(want_in)), tag
        worst["in"] = max(worst["in"], worst_ratio(out * row.s_next, ref[2], bnd[2]))
    print(f"[sigma_step] {len(MATRIX)} cases, worst |got - float64| / bound: out {worst['out']:.3f}, hist_out {worst['hist_out']:.3f}, "
          f"scaled input before its bf16 rounding {worst['in']:.3f}")
    assert worst["in"] <= 1.0


@pytest.mark.parametrize("chw", [900, 1023])
def test_kernel_identities(dev, chw):
    nb, n = 2, 2 * chw
    out_of = lambda b: b.fetch()[0][F32.index("out"), GUARD:GUARD + n].clone()
    row = _row(0, "v", 3, 1.3, seed=7)
    # a second run is bit-equal
    b = Buffers(dev, n, "pair", "unit", seed=3)
    _launch(b, row, nb, chw, True)
    first = b.fetch()
    _launch(b, row, nb, chw, True)
    again = b.fetch()
    assert torch.equal(_bits(first[0]), _bits(again[0])) and torch.equal(_bits(first[1]), _bits(again[1]))
    # out aliasing x and hist_out aliasing the oldest history slot: the bits of the call that aliases nothing
    a = Buffers(dev, n, "pair", "unit", seed=3)
    _launch(a, row, nb, chw, True, out="x", hist_out="h3")
    got32, got16 = a.fetch()
    _check_fences(a, got32, got16, ("x", "h3"), ("in1", "in2"))
    w = lambda t, names, name: _bits(t[names.index(name), GUARD:GUARD + n])
    assert torch.equal(w(got32, F32, "x"), w(first[0], F32, "out")) and torch.equal(w(got32, F32, "h3"), w(first[0], F32, "hist_out"))
    assert torch.equal(w(got16, BF16, "in1"), w(first[1], BF16, "in1")) and torch.equal(w(got16, BF16, "in2"), w(first[1], BF16, "in2"))
    # without in2 and hist_out nothing is written there
    c = Buffers(dev, n, "pair", "unit", seed=3)
    _launch(c, row, nb, chw, True, hist_out=None, in2=False)
    got32, got16 = c.fetch()
    _check_fences(c, got32, got16, ("out",), ("in1",))
    assert torch.equal(w(got32, F32, "out"), w(first[0], F32, "out"))
    # a = 0, c0 = 1, kind 1 (the last dpmpp_2m step): out is hist_out
    last = StepRow(1, row.p, row.q, row.sigma, 0.0, (1.0,), 0.0, 1.0)
    d = Buffers(dev, n, "pair", "large", seed=4)
    _launch(d, last, nb, chw, False)
    got32, _ = d.fetch()
    assert torch.equal(got32[F32.index("out"), GUARD:GUARD + n], got32[F32.index("hist_out"), GUARD:GUARD + n])
    assert torch.isfinite(got32[F32.index("out"), GUARD:GUARD + n]).all()
    # a pair with equal halves: the single branch's bits
    e = Buffers(dev, n, "single", "unit", seed=5)
    _launch(e, row, nb, chw, True)
    f = Buffers(dev, n, "eps_text", "unit", seed=5)
    f.d16[BF16.index("eps_text")].copy_(f.d16[BF16.index("eps")])
    _launch(f, row, nb, chw, True)
    (e32, e16), (f32_, f16) = e.fetch(), f.fetch()
    for name in ("out", "hist_out"):
        assert torch.equal(e32[F32.index(name), GUARD:GUARD + n], f32_[F32.index(name), GUARD:GUARD + n]), name
    assert torch.equal(w(e16, BF16, "in1"), w(f16, BF16, "in1"))


# ---------------------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------------------
class _Model:
    """the fp32 oracle UNet with the slider's oracle LoRA network, gated at start_noise: eps(scaled input, t), guidance-combined for
    the pair"""

    def __init__(self, name, sd, ctx, kw, scale, start_noise, gs, rows):
        self.net = _bf16_valued(build_unet(name, seed=0))
        self.nw = None
        if sd is not None:
            self.nw = LoRANetworkOracle(self.net, rank=4, multiplier=1.0, alpha=1.0, train_method="noxattn")
            self.nw.load_state_dict(sd, strict=True)
        self.ctx, self.kw, self.scale, self.start_noise, self.gs, self.rows = ctx, kw, scale, start_noise, gs, rows

    @torch.no_grad()
    def __call__(self, x, t):
        args = (torch.cat([x] * self.rows), float(t), self.ctx) + ((self.kw,) if self.kw is not None else ())
        if self.nw is None:
            e = self.net(*args).sample
        else:
            self.nw.set_lora_slider(0 if float(t) > self.start_noise else self.scale)
            with self.nw:
                e = self.net(*args).sample
        if self.rows == 2:
            u, c = e.chunk(2)
            e = u + self.gs * (c - u)
        return e


def _reference_loop(model, sch, steps, noise, draws):
    """the reference's loop with the tensor-op scheduler on fp32 tensors"""
    sch.set_timesteps(steps)
    x = noise * sch.init_noise_sigma
    for i, t in enumerate(sch.timesteps):
        x = sch.step(model(sch.scale_model_input(x, t), t), t, x, noise=None if draws is None else draws[i]).prev_sample
    return x


def _fp32_draws(dev, seed, steps, shape):
    """what _sample_fp32 draws: one fp32 tensor for all steps from the scheduler's generator"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return list(torch.randn((steps,) + tuple(shape), generator=g, device=dev, dtype=torch.float32).cpu())


def _bf16_draws(dev, seed, steps, shape):
    """what the bf16 path draws: one bf16 tensor per step"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return [torch.randn(shape, generator=g, device=dev, dtype=torch.bfloat16).float().cpu() for _ in range(steps)]


def _sched(name, spacing, pred="epsilon"):
    k = {} if spacing is None else {"timestep_spacing": spacing}
    cls = {"euler": schedulers.EulerDiscreteScheduler, "euler_a": schedulers.EulerAncestralDiscreteScheduler,
           "dpmpp_2m": schedulers.DPMSolverPP2MScheduler}.get(name)
    return cls(prediction_type=pred, **k) if cls else schedulers.create(name, pred)


@pytest.mark.parametrize("scheduler", ["euler", "euler_a", "lms", "ddpm"])
@pytest.mark.parametrize("steps", [4, 10])
def test_fp32_latents_against_the_reference_loop(dev, tiny, scheduler, steps):
    """4 steps (euler_a: the trailing grid 999, 749, 499, 249; the others' own grids also cross start_noise) as the single branch, 10
    steps as the CFG pair; a slider gated at start_noise 600 in both"""
    cfg, net, eng, store, sd = tiny
    scale, start_noise, seed, gs = 2.0, 600, 3, 3.0
    spacing = "trailing" if scheduler == "euler_a" and steps == 4 else None
    single = steps == 4
    unc, txt, pu, pt, noise = _inputs(cfg, 1, seed=60 + steps)
    ctx, pooled = (txt, pt) if single else (torch.cat([unc, txt]), torch.cat([pu, pt]))
    rows = 1 if single else 2
    run = dict(scale=scale, start_noise=start_noise, ddim_steps=steps, guidance_scale=gs, pooled=pooled.to(dev))
    mk = lambda latents: SliderSampler(eng, store, scheduler=scheduler, timestep_spacing=spacing, scheduler_seed=seed, latents=latents)
    got = mk("fp32").sample_latents(ctx.to(dev), noise.to(dev), **run)
    old = mk("bf16").sample_latents(ctx.to(dev), noise.to(dev), **run)
    torch.cuda.synchronize()
    assert got.dtype == torch.bfloat16 and got.shape == noise.shape and torch.isfinite(got.float()).all()
    model = _Model("tiny_sdxl", sd, ctx, {"text_embeds": pooled, "time_ids": _time_ids(rows)}, scale, start_noise, gs, rows)
    noisy = scheduler in ("euler_a", "ddpm")
    want = _reference_loop(model, _sched(scheduler, spacing), steps, noise, _fp32_draws(dev, seed, steps, noise.shape) if noisy else None)
    want_old = (_reference_loop(model, _sched(scheduler, spacing), steps, noise, _bf16_draws(dev, seed, steps, noise.shape)) if noisy else want)
    r, r_old = rel_err(got.float().cpu(), want), rel_err(old.float().cpu(), want_old)
    print(f"[parity] {scheduler}, {steps} steps, {'single branch' if single else 'pair'}: final latents rel_l2 fp32 latents {r:.3e}, "
          f"bf16 path {r_old:.3e} (ratio {r / r_old:.2f})")
    assert r < 3e-2
    assert r <= 1.25 * r_old, f"fp32 latents {r:.3e} > 1.25 x the bf16 path's {r_old:.3e}"


@pytest.fixture(scope="module")
def tiny_v(dev):
    """tiny_sd2 (v prediction, no added conditions): config and engine"""
    cfg = CONFIGS["tiny_sd2"]()
    return cfg, UNetEngine(cfg, _bf16_valued(build_unet("tiny_sd2", seed=0)).state_dict(), dev)


@pytest.mark.parametrize("scheduler", ["euler", "euler_a", "lms", "ddpm"])
def test_fp32_latents_v_prediction_against_the_reference_loop(dev, tiny_v, scheduler):
    """the same comparison with the v rows of p and q: tiny_sd2, the CFG pair, 4 steps, no slider"""
    cfg, eng = tiny_v
    steps, seed, gs, pred = 4, 6, 3.0, "v_prediction"
    unc, txt, _, _, noise = _inputs(cfg, 1, seed=9, xl=False)
    ctx = torch.cat([unc, txt])
    mk = lambda latents: SliderSampler(eng, prediction_type=pred, scheduler=scheduler, scheduler_seed=seed, latents=latents)
    run = dict(ddim_steps=steps, guidance_scale=gs)
    got = mk("fp32").sample_latents(ctx.to(dev), noise.to(dev), **run)
    old = mk("bf16").sample_latents(ctx.to(dev), noise.to(dev), **run)
    torch.cuda.synchronize()
    model = _Model("tiny_sd2", None, ctx, None, 0.0, 0, gs, 2)
    noisy = scheduler in ("euler_a", "ddpm")
    want = _reference_loop(model, _sched(scheduler, None, pred), steps, noise, _fp32_draws(dev, seed, steps, noise.shape) if noisy else None)
    want_old = (_reference_loop(model, _sched(scheduler, None, pred), steps, noise, _bf16_draws(dev, seed, steps, noise.shape)) if noisy else want)
    r, r_old = rel_err(got.float().cpu(), want), rel_err(old.float().cpu(), want_old)
    print(f"[parity] {scheduler}, v prediction, {steps} steps, pair: final latents rel_l2 fp32 latents {r:.3e}, bf16 path {r_old:.3e} "
          f"(ratio {r / r_old:.2f})")
    assert torch.isfinite(got.float()).all() and r < 3e-2
    assert r <= 1.25 * r_old, f"fp32 latents {r:.3e} > 1.25 x the bf16 path's {r_old:.3e}"


@pytest.mark.parametrize("spacing,steps,pred", [("trailing", 4, "epsilon"), (None, 10, "epsilon"), ("trailing", 4, "v_prediction")])
def test_dpmpp_2m_against_the_lambda_form_oracle(dev, tiny, spacing, steps, pred):
    """the engine's dpmpp_2m latents against the same oracle UNet stepped by the float64 lambda-form oracle of the host tests; v
    prediction on tiny_sd2 (no slider, no added conditions)"""
    v = pred == "v_prediction"
    scale, start_noise, gs = 2.0, 600, 3.0
    if v:
        cfg = CONFIGS["tiny_sd2"]()
        eng = UNetEngine(cfg, _bf16_valued(build_unet("tiny_sd2", seed=0)).state_dict(), dev)
        _, txt, _, _, noise = _inputs(cfg, 1, seed=9, xl=False)
        smp = SliderSampler(eng, prediction_type=pred, scheduler="dpmpp_2m", timestep_spacing=spacing)
        got = smp.sample_latents(txt.to(dev), noise.to(dev), ddim_steps=steps)
        model = _Model("tiny_sd2", None, txt, None, 0.0, start_noise, gs, 1)
    else:
        cfg, _, eng, store, sd = tiny
        unc, txt, pu, pt, noise = _inputs(cfg, 1, seed=70 + steps)
        ctx, pooled = torch.cat([unc, txt]), torch.cat([pu, pt])
        smp = SliderSampler(eng, store, scheduler="dpmpp_2m", timestep_spacing=spacing)
        got = smp.sample_latents(ctx.to(dev), noise.to(dev), scale=scale, start_noise=start_noise, ddim_steps=steps, guidance_scale=gs,
                                 pooled=pooled.to(dev))
        model = _Model("tiny_sdxl", sd, ctx, {"text_embeds": pooled, "time_ids": _time_ids(2)}, scale, start_noise, gs, 2)
    torch.cuda.synchronize()
    assert smp.latents == "fp32" and got.dtype == torch.bfloat16
    sch = smp.sched
    sig, ts = sch.sigmas.double().tolist(), sch.timesteps.tolist()

    def denoise(x, i):
        s = sig[i]
        al = 1 / math.sqrt(s * s + 1)
        m = model((x * al).float(), ts[i]).double()
        return al * (x * al) - s * al * m if v else x - s * m

    want = dpmpp_2m_oracle(sig, noise.double() * float(sch.init_noise_sigma), denoise)[-1]
    r = rel_err(got.float().cpu(), want.float())
    print(f"[parity] dpmpp_2m {spacing} {steps} steps {pred}: final latents rel_l2 {r:.3e} against the lambda-form oracle")
    assert torch.isfinite(got.float()).all() and r < 3e-2


def test_fp32_loop_launch_shape(dev, tiny, monkeypatch):
    """per step: one replay, one slh_sigma_step; Pass.load_latents once, ahead of the loop"""
    cfg, _, eng, store, _ = tiny
    unc, txt, pu, pt, noise = _inputs(cfg, 1, seed=81)
    events = []
    real_load, real_run, real_step = Pass.load_latents, Pass.run, lib.sigma_step
    monkeypatch.setattr(Pass, "load_latents", lambda self, x: (events.append("load"), real_load(self, x))[1])
    monkeypatch.setattr(Pass, "run", lambda self, *a: (events.append("run"), real_run(self, *a))[1])
    monkeypatch.setattr(lib, "sigma_step", lambda *a, **k: (events.append("step"), real_step(*a, **k))[1])
    for scheduler, steps in (("lms", 6), ("euler_a", 3), ("dpmpp_2m", 5)):
        events.clear()
        smp = SliderSampler(eng, store, scheduler=scheduler, latents="fp32")
        smp.sample_latents(torch.cat([unc, txt]).to(dev), noise.to(dev), scale=1.0, ddim_steps=steps, pooled=torch.cat([pu, pt]).to(dev))
        assert events == ["load"] + ["run", "step"] * steps, (scheduler, events)
    with pytest.raises(ValueError, match="does not apply to ddim"):
        SliderSampler(eng, store, scheduler="ddim", latents="fp32")
    with pytest.raises(ValueError, match="only with latents='fp32'"):
        SliderSampler(eng, store, scheduler="dpmpp_2m", latents="bf16")


def test_fp32_latents_with_merged_sliders(dev, tiny):
    """sliders= (merged weights): one merge when the loop crosses start_noise, the weight bits restored, two calls bit-equal, the
    reference loop met"""
    from sliders_amd.merge import SliderSet
    cfg, net, _, _, sd = tiny
    eng = UNetEngine(cfg, net.state_dict(), dev)
    steps, scale, start_noise, seed = 4, 2.0, 600, 3
    _, txt, _, pt, noise = _inputs(cfg, 1, seed=44)
    snap = {k: v.clone() for k, v in eng.w.t.items()}
    kw = dict(scheduler="euler_a", timestep_spacing="trailing", scheduler_seed=seed, latents="fp32")
    smp = SliderSampler(eng, sliders=SliderSet(cfg, [(sd, None)]), **kw)
    merges, real = [], smp.merger.merge
    smp.merger.merge = lambda scales: (merges.append(list(scales)), real(scales))[1]
    run = dict(start_noise=start_noise, ddim_steps=steps, pooled=pt.to(dev))
    got = smp.sample_latents(txt.to(dev), noise.to(dev), scale=scale, **run)
    torch.cuda.synchronize()
    assert merges == [[scale]] and not smp.merger.merged
    assert all(torch.equal(v, snap[k]) for k, v in eng.w.t.items()), "the original weight bits are back"
    again = SliderSampler(eng, sliders=SliderSet(cfg, [(sd, None)]), **kw).sample_latents(txt.to(dev), noise.to(dev), scale=scale, **run)
    assert torch.equal(again, got), "two calls, the same bits"
    model = _Model("tiny_sdxl", sd, txt, {"text_embeds": pt, "time_ids": _time_ids(1)}, scale, start_noise, 0.0, 1)
    want = _reference_loop(model, _sched("euler_a", "trailing"), steps, noise, _fp32_draws(dev, seed, steps, noise.shape))
    r = rel_err(got.float().cpu(), want)
    print(f"[parity] euler_a trailing, fp32 latents, merged sliders: final latents rel_l2 {r:.3e}")
    assert r < 3e-2


@pytest.mark.parametrize("scheduler", ["euler", "euler_a"])
def test_bf16_latents_are_the_unfused_path(dev, tiny, scheduler):
    """without the option a call returns the bits of _sample_unfused, run here directly on the same object"""
    cfg, _, eng, store, _ = tiny
    unc, txt, pu, pt, noise = _inputs(cfg, 1, seed=90)
    ctx, pooled = torch.cat([unc, txt]).to(dev), torch.cat([pu, pt]).to(dev)
    smp = SliderSampler(eng, store, scheduler=scheduler, scheduler_seed=5)
    assert smp.latents == "bf16"
    state = None if smp.sched_generator is None else smp.sched_generator.get_state()
    got = smp.sample_latents(ctx, noise.to(dev), scale=1.5, start_noise=600, ddim_steps=4, guidance_scale=3.0, pooled=pooled)
    if state is not None:
        smp.sched_generator.set_state(state)
    drv = Pass(eng, eng.plan(2, HW, HW, "on"))
    drv.load_cond(ctx, pooled, None)
    with smp.slider_session(1.5, 600) as gate:
        want = smp._sample_unfused(drv, gate, noise.to(dev), 4, 3.0, False)
    assert want.dtype == torch.bfloat16 and torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,sched,latents", [(["--scheduler", "dpmpp_2m", "--ddim_steps", "6"], "DPMSolverPP2MScheduler", "fp32"),
                                                 (["--scheduler", "dpmpp_2m", "--ddim_steps", "6", "--timestep_spacing", "trailing"],
                                                  "DPMSolverPP2MScheduler", "fp32"),
                                                 (["--scheduler", "euler", "--fp32_latents", "--ddim_steps", "6"], "EulerDiscreteScheduler", "fp32")])
def test_cli(dev, tmp_path, monkeypatch, flags, sched, latents):
    import sliders_amd.model_util as mu
    from sliders_amd import generate

    def tiny_engine(model, device, seed):     # --synthetic on the tiny SDXL topology, as tests/test_fewstep_sampler_gpu.py
        cfg = CONFIGS["tiny_sdxl"]()
        return UNetEngine(cfg, mu.random_state_dict(cfg, device, seed), device)
    monkeypatch.setattr(mu, "synthetic_engine", tiny_engine)
    made = []
    real = SliderSampler.sample_latents

    def spy(self, ctx, noise, **kw):
        made.append((type(self.sched).__name__, self.sched.timestep_spacing, self.latents, ctx.shape[0], kw["ddim_steps"]))
        return real(self, ctx, noise, **kw)
    monkeypatch.setattr(SliderSampler, "sample_latents", spy)
    outs = []
    for run in ("a", "b"):
        out = os.path.join(tmp_path, run)
        generate.main(["--synthetic", "--scales=-1,1", "--res", "128", "--out", out] + flags)
        assert sorted(os.listdir(out)) == ["scale_-1.png", "scale_1.png"]
        outs.append([open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))])
    assert outs[0] == outs[1], "a second run writes the same bytes"
    spacing = "trailing" if "trailing" in flags else "leading"
    assert made == [(sched, spacing, latents, 2, 6)] * 4
