"""Prompt-direction sampling on the engine (docs/SAMPLING.md, "Prompt-direction sampling"): SliderSampler.sample_latents(directions=,
direction_quantile=) in all three loops and both branches, and python -m sliders_amd.generate --direction.

Everything here is an identity of bits: the tiny SDXL at 16^2 latents, 6 steps, start_noise on the grid's third point (two plain steps,
four live ones)."""
import os

import pytest
import torch

from sliders_amd import generate, lib, schedulers
from sliders_amd.config import CONFIGS
from sliders_amd.directions import Direction, DirectionSet
from sliders_amd.passes import Pass
from sliders_amd.sampler import SliderSampler
from sliders_amd.unet import UNetEngine
from tests.test_fewstep_sampler_gpu import HW, _inputs, tiny  # noqa: F401  (tiny: the module's fixture)

pytestmark = pytest.mark.gpu

STEPS, LIVE, SCALE, GS, SEED = 6, 4, 2.0, 3.0, 7
CHW, PIX = 4 * HW * HW, HW * HW
# (scheduler, latents): the fused DDIM loop, the fp32 loop without and with a multistep history, the bf16 tensor-op loop
LOOPS = {"ddim": ("ddim", None), "euler": ("euler", "fp32"), "dpmpp_2m": ("dpmpp_2m", None), "lms": ("lms", None)}


@pytest.fixture(scope="module")
def engine(dev, tiny):
    """an engine of this module's own: its plan cache shows what the calls below planned"""
    cfg, net, _, _, _ = tiny
    return cfg, UNetEngine(cfg, net.state_dict(), dev)


def _sampler(eng, loop):
    scheduler, latents = LOOPS[loop]
    return SliderSampler(eng, scheduler=scheduler, scheduler_seed=SEED, latents=latents)


def _grid(smp):
    if smp.sched.fused:
        return [float(t) for t in smp.sched.make_timesteps(STEPS)]
    smp.sched.set_timesteps(STEPS)
    return smp.sched.timesteps.tolist()


def _cond(cfg, dev, single=False, seed=21):
    unc, txt, pu, pt, noise = _inputs(cfg, 1, seed=seed)
    ctx, pooled = (txt, pt) if single else (torch.cat([unc, txt]), torch.cat([pu, pt]))
    return ctx.to(dev), pooled.to(dev), noise.to(dev)


def _directions(cfg, dev, J, seed=31):
    g = torch.Generator().manual_seed(seed)
    draw = lambda *shape: torch.randn(*shape, generator=g).to(dev)
    return DirectionSet([Direction(draw(1, 77, cfg.cross_attention_dim), draw(1, 77, cfg.cross_attention_dim), draw(1, cfg.pooled_dim),
                                   draw(1, cfg.pooled_dim), eta=1.0 + k, sign=1.0 if k == 0 else -1.0) for k in range(J)])


def _plans(eng):
    return sorted(k[0] for k in eng._plans)


# ---------------------------------------------------------------------------------------------------------------------------
# null cases
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("loop", ["ddim", "dpmpp_2m", "lms"])
def test_directions_that_do_not_act_are_plain_sampling(dev, engine, loop, single, monkeypatch):
    cfg, eng = engine
    ctx, pooled, noise = _cond(cfg, dev, single)
    dirs = _directions(cfg, dev, 2)
    run = dict(ddim_steps=STEPS, guidance_scale=GS, pooled=pooled)
    plain = _sampler(eng, loop).sample_latents(ctx, noise, scale=SCALE, **run)
    eng.flush_plans()
    launches = []
    monkeypatch.setattr(lib, "eps_direction", lambda *a, **k: launches.append("combine"))
    monkeypatch.setattr(lib, "direction_threshold", lambda *a, **k: launches.append("threshold"))
    smp = _sampler(eng, loop)
    start_noise = _grid(smp)[STEPS - LIVE]
    for kw in (dict(scale=0.0, start_noise=start_noise), dict(scale=SCALE, start_noise=-1)):
        got = _sampler(eng, loop).sample_latents(ctx, noise, directions=dirs, direction_quantile=0.9, **kw, **run)
        assert torch.equal(got, plain), kw
    assert _plans(eng) == [ctx.shape[0]] and not launches, "no wide plan, no direction launch"
    with pytest.raises(ValueError, match="expected 0 <= q < 1"):
        smp.sample_latents(ctx, noise, scale=0.0, directions=dirs, direction_quantile=1.0, **run)


# ---------------------------------------------------------------------------------------------------------------------------
# the chain against a loop driven here from the public pieces: which plan, which rows, which launches, which copy
# ---------------------------------------------------------------------------------------------------------------------------
class _Hand:
    def __init__(self, eng, ctx, pooled, dirs, q, single, scale):
        self.eng, self.single, self.base, self.J = eng, single, 1 if single else 2, len(dirs)
        self.R = self.base + 2 * self.J
        self.coef = dirs.coefficients(scale, GS, single)
        self.keep = DirectionSet.n_keep(PIX, q)
        d_ctx, d_pooled = dirs.rows(1, eng.device)
        self.wide_cond = (torch.cat([ctx, d_ctx]), torch.cat([pooled, d_pooled]))
        self.drv = Pass(eng, eng.plan(self.base, HW, HW, "off"))
        self.drv.load_cond(ctx, pooled, None)
        self.wide = False
        self.guided = torch.empty(1, 4, HW, HW, dtype=torch.bfloat16, device=eng.device)
        self.thr = torch.empty(1, self.J, 4, dtype=torch.int32, device=eng.device)
        self.s = torch.cuda.current_stream().cuda_stream

    def widen(self, latent=None):
        """-> the pass on the wide plan; latent: what the plain plan's input buffer holds for the next pass"""
        x = None if latent is None else latent.clone()
        self.drv = Pass(self.eng, self.eng.plan(self.R, HW, HW, "off"))
        self.drv.load_cond(*self.wide_cond, None)
        if x is not None:
            self.drv.load_latents(x)
        self.wide = True

    def guide(self):
        """threshold (q > 0) and combine behind a wide replay -> the guided row's address"""
        eps = self.drv.io["eps"].ptr
        pos = [eps + (self.base + 2 * k) * CHW * 2 for k in range(self.J)]
        neg = [eps + (self.base + 2 * k + 1) * CHW * 2 for k in range(self.J)]
        if self.keep < PIX:
            lib.direction_threshold(self.s, pos=pos, neg=neg, thr=self.thr.data_ptr(), n_keep=[self.keep] * self.J, nb=1, chw=CHW, hw=PIX)
        lib.eps_direction(self.s, t=eps + (self.base - 1) * CHW * 2, out=self.guided.data_ptr(), pos=pos, neg=neg, c=self.coef, nb=1, chw=CHW,
                          hw=PIX, thr=self.thr.data_ptr() if self.keep < PIX else 0)
        return self.guided.data_ptr()

    def spread(self):
        smp = self.drv.io["sample"].tensor
        smp[self.base:].copy_(smp[:1].expand(self.R - self.base, -1, -1, -1))


def _hand_loop(smp, h: _Hand, noise, start_noise):
    sch, s, single = smp.sched, h.s, h.single
    ts = _grid(smp)
    if smp.sched.fused:                                  # ddim: in place on the plan's input buffer
        h.drv.load_latents(noise)
        for i, t in enumerate(ts):
            first, live = i == 0, t <= start_noise
            if live and not h.wide:
                h.widen(h.drv.io["sample"].tensor[:1])
                first = True
            h.drv.run(t, first, s)
            buf, eps = h.drv.io["sample"], h.drv.io["eps"]
            text = h.guide() if live else 0
            rows = (dict(eps=text or eps.ptr, eps_text=text or eps.ptr, out2=0, guidance=0.0) if single
                    else dict(eps=eps.ptr, eps_text=text, out2=buf.ptr + CHW * 2, guidance=GS))
            lib.call(lib.OP_CFG_DDIM, lib.CfgDdimDesc(x=buf.ptr, out=buf.ptr, nb=1, chw=CHW, **rows, **sch.step_fields(int(t), STEPS)), s)
            if live:
                h.spread()
        return h.drv.io["sample"].tensor[:1].clone()
    if smp.latents == "fp32":                            # one slh_sigma_step per pass on an fp32 master latent
        rows = [schedulers.step_row(sch, i, STEPS) for i in range(STEPS)]
        x = (noise.float() * sch.init_noise_sigma).contiguous()
        ring = [torch.empty_like(x) for _ in range(schedulers.history_depth(sch, STEPS))]
        h.drv.load_latents(sch.scale_model_input(x, sch.timesteps[0]))
        for i, t in enumerate(ts):
            first, live, r = i == 0, t <= start_noise, rows[i]
            if live and not h.wide:
                h.widen(h.drv.io["sample"].tensor[:1])
                first = True
            h.drv.run(t, first, s)
            buf, eps = h.drv.io["sample"], h.drv.io["eps"]
            text = h.guide() if live else 0
            lib.sigma_step(s, eps=text if live and single else eps.ptr, eps_text=0 if single else text, x=x.data_ptr(), out=x.data_ptr(), nb=1,
                           chw=CHW, kind=r.kind, p=r.p, q=r.q, sigma=r.sigma, a=r.a, c=r.c, c_n=r.c_n, s_next=r.s_next, guidance=GS, single=single,
                           hist=[ring[(i - k) % len(ring)].data_ptr() for k in range(1, r.n_hist + 1)],
                           hist_out=ring[i % len(ring)].data_ptr() if ring else 0, in_bf16=buf.ptr, in2_bf16=0 if single else buf.ptr + CHW * 2)
            if live:
                h.spread()
        return x.to(torch.bfloat16)
    # the bf16 tensor-op path: the scheduler's own step around the prediction
    sch.set_timesteps(STEPS, device=h.eng.device)
    lat = (noise.float() * sch.init_noise_sigma).to(torch.bfloat16)
    out = torch.empty_like(lat)
    n = [0]

    def predict(x, t):
        first, live = n[0] == 0, float(t) <= start_noise
        n[0] += 1
        if live and not h.wide:
            h.widen()
            first = True
        h.drv.load_latents(x)
        h.drv.run(t, first, s)
        eps = h.drv.io["eps"]
        text = h.guide() if live else 0
        if single:
            return h.guided.view_as(lat) if live else eps.tensor.view_as(lat)
        lib.call(lib.OP_CFG_DDIM, lib.CfgDdimDesc(eps=eps.ptr, eps_text=text, x=0, out=out.data_ptr(), out2=0, nb=1, chw=CHW, guidance=GS, do_step=0), s)
        return out

    return schedulers.denoise(sch, predict, lat, STEPS, STEPS, generator=None, device=h.eng.device)


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("loop", list(LOOPS))
def test_sampler_against_a_loop_of_the_public_pieces(dev, engine, loop, single):
    cfg, eng = engine
    ctx, pooled, noise = _cond(cfg, dev, single, seed=22)
    start_noise = _grid(_sampler(eng, loop))[STEPS - LIVE]
    run = dict(start_noise=start_noise, ddim_steps=STEPS, guidance_scale=GS, pooled=pooled)
    base = _sampler(eng, loop).sample_latents(ctx, noise, scale=SCALE, **run)
    seen = []
    for J, q in ((1, 0.0), (2, 0.9), (1, 0.9), (2, 0.0)):
        dirs = _directions(cfg, dev, J)
        eng.flush_plans()
        got = _sampler(eng, loop).sample_latents(ctx, noise, scale=SCALE, directions=dirs, direction_quantile=q, **run)
        # (the plain plan ran above start_noise; where the wide plan made the arena grow, the engine has dropped it from its cache)
        assert ctx.shape[0] + 2 * J in _plans(eng) and set(_plans(eng)) <= {ctx.shape[0], ctx.shape[0] + 2 * J}, "one wide plan, of 2 J more blocks"
        want = _hand_loop(_sampler(eng, loop), _Hand(eng, ctx, pooled, dirs, q, single, SCALE), noise, start_noise)
        assert got.dtype == torch.bfloat16 and got.shape == noise.shape and bool(torch.isfinite(got.float()).all())
        assert torch.equal(got, want), (J, q)
        assert not torch.equal(got, base), "the directions act"
        assert all(not torch.equal(got, o) for o in seen), "J and the quantile matter"
        seen.append(got)
        # the pairs the other way round at the opposite scale: d and c change sign, the keys read |d|
        assert torch.equal(_sampler(eng, loop).sample_latents(ctx, noise, scale=-SCALE, directions=dirs.swapped(), direction_quantile=q, **run), got)
    # a second call of one sampler over a warm plan cache: the same bits (dpmpp_2m / ddim / euler draw nothing)
    smp = _sampler(eng, loop)
    a = smp.sample_latents(ctx, noise, scale=SCALE, directions=dirs, **run)
    assert torch.equal(smp.sample_latents(ctx, noise, scale=SCALE, directions=dirs, **run), a) and torch.equal(a, seen[-1])


# ---------------------------------------------------------------------------------------------------------------------------
# trace and mask; a slider next to the directions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", ["ddim", "euler", "dpmpp_2m"])
def test_trace_and_mask(dev, engine, loop, monkeypatch):
    cfg, eng = engine
    ctx, pooled, noise = _cond(cfg, dev, seed=23)
    dirs = _directions(cfg, dev, 2)
    smp = _sampler(eng, loop)
    start_noise = _grid(smp)[STEPS - LIVE]
    run = dict(start_noise=start_noise, ddim_steps=STEPS, guidance_scale=GS, pooled=pooled, directions=dirs, direction_quantile=0.5)
    trace = smp.base_trace(ctx, noise, STEPS, GS, pooled, None, start_noise)
    plain = _sampler(eng, loop).sample_latents(ctx, noise, scale=SCALE, **run)
    assert not torch.equal(plain, trace.final)
    runs = []
    real_run = Pass.run
    monkeypatch.setattr(Pass, "run", lambda self, *a: (runs.append(self.p.B), real_run(self, *a))[1])
    # a trace alone: the same bits; without a multistep history the chain starts at the first live step, on the wide plan
    assert torch.equal(smp.sample_latents(ctx, noise, scale=SCALE, trace=trace, **run), plain)
    assert runs == ([2] * (STEPS - LIVE) + [6] * LIVE if loop == "dpmpp_2m" else [6] * LIVE)
    half = torch.zeros(HW, HW)
    half[:, HW // 2:] = 1.0
    out = smp.sample_latents(ctx, noise, scale=SCALE, mask=half, trace=trace, **run)
    assert torch.equal(out[..., :HW // 2], trace.final[..., :HW // 2]), "outside the mask: the scale-0 image, bit for bit"
    assert not torch.equal(out[..., HW // 2:], trace.final[..., HW // 2:])
    assert torch.equal(smp.sample_latents(ctx, noise, scale=SCALE, mask=torch.ones(HW, HW), trace=trace, **run), plain)
    assert torch.equal(smp.sample_latents(ctx, noise, scale=SCALE, mask=torch.zeros(HW, HW), trace=trace, **run), trace.final)


def test_a_slider_next_to_the_directions(dev, tiny):
    """store= stays legal: the adapter acts on every row of the wide pass, and is off again afterwards"""
    cfg, _, eng, store, _ = tiny
    ctx, pooled, noise = _cond(cfg, dev, seed=24)
    dirs = _directions(cfg, dev, 1)
    smp = SliderSampler(eng, store, scheduler="ddim")
    start_noise = _grid(smp)[STEPS - LIVE]
    run = dict(scale=SCALE, start_noise=start_noise, ddim_steps=STEPS, guidance_scale=GS, pooled=pooled)
    slider = smp.sample_latents(ctx, noise, **run)
    both = smp.sample_latents(ctx, noise, directions=dirs, **run)
    assert bool(torch.isfinite(both.float()).all()) and not torch.equal(both, slider)
    assert torch.equal(smp.sample_latents(ctx, noise, directions=dirs, **run), both)
    assert (4, HW, HW, "on") in eng._plans and not eng.lora_active and float(eng.lora_scale) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------
def test_cli(dev, tmp_path, monkeypatch):
    import sliders_amd.model_util as mu
    cfg = CONFIGS["tiny_sdxl"]()
    engines = {}

    def tiny_engine(model, device, seed):     # --synthetic on the tiny SDXL topology, built once for the runs below
        if seed not in engines:
            engines[seed] = UNetEngine(cfg, mu.random_state_dict(cfg, device, seed), device)
        return engines[seed]
    monkeypatch.setattr(mu, "synthetic_engine", tiny_engine)
    common = ["--synthetic", "--res", "128", "--ddim_steps", "6", "--start_noise", "498", "--guidance_scale", "3"]
    read = lambda out, names: [open(os.path.join(out, n), "rb").read() for n in names]
    plain = generate.main(common + ["--scales=0", "--out", str(tmp_path / "plain")])
    steer = ["--direction", "smiling person|frowning person:2", "--direction", "old|young", "--direction_quantile", "0.8"]
    out = generate.main(common + steer + ["--scales=-1,0,1", "--out", str(tmp_path / "steer")])
    names = ["scale_-1.png", "scale_0.png", "scale_1.png"]
    assert sorted(os.listdir(out)) == sorted(names)
    got = read(out, names)
    assert got[1] == read(plain, ["scale_0.png"])[0], "scale 0 is the image without --direction"
    assert got[0] != got[1] != got[2] != got[0]
    assert 6 in _plans(engines[0]), "two directions next to the CFG pair: six row blocks"
    # a sweep without scale 0 takes the loop that keeps no trace: the same bytes
    out = generate.main(common + steer + ["--scales=1", "--out", str(tmp_path / "one")])
    assert read(out, ["scale_1.png"])[0] == got[2]
    # a prompts file, the single branch, an fp32 loop
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prompts_sample.yaml")
    out = generate.main(common + ["--direction_file", path, "--no_cfg", "--scheduler", "euler", "--fp32_latents", "--scales=0,2",
                                  "--out", str(tmp_path / "file")])
    two = read(out, ["scale_0.png", "scale_2.png"])
    assert two[0] != two[1] and 5 in _plans(engines[0])
    assert len(engines) == 1
