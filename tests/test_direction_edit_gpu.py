"""Prompt-direction edits on the engine (docs/EDIT.md, "Prompt-direction edits"): SliderEditor.edit_latents(directions=,
direction_quantile=, direction_momentum=), the directions' footprint, SliderSampler.sample_latents(direction_momentum=) and
python -m sliders_amd.edit --direction.

Everything here is an identity of bits: the tiny SDXL at 16^2 latents, 6 steps, skip 0, start_noise on the grid's third point (two
plain steps, four live ones)."""
import os

import numpy as np
import pytest
import torch

from sliders_amd import edit, lib
from sliders_amd.config import CONFIGS
from sliders_amd.ddim import DDIMSchedule
from sliders_amd.directions import DirectionSet
from sliders_amd.edit import NoiseSpace, SliderEditor, ddpm_step_coefficients, footprint_draws, footprint_mean, fp32_coefficients
from sliders_amd.passes import Pass
from sliders_amd.sampler import SliderSampler
from sliders_amd.unet import UNetEngine
from tests.test_direction_sampling_gpu import _cond, _directions, _plans
from tests.test_fewstep_sampler_gpu import HW, tiny  # noqa: F401  (tiny: the module's fixture)

pytestmark = pytest.mark.gpu

STEPS, LIVE, SCALE, GS = 6, 4, 2.0, 3.0
CHW, PIX = 4 * HW * HW, HW * HW
TS = DDIMSchedule().make_timesteps(STEPS)
START = TS[STEPS - LIVE]
MOMENTUM = (0.5, 0.4)


@pytest.fixture(scope="module")
def engine(dev, tiny):
    """an engine of this module's own (its plan cache shows what the calls below planned), its editor, and an inversion"""
    cfg, net, _, _, _ = tiny
    eng = UNetEngine(cfg, net.state_dict(), dev)
    ed = SliderEditor(eng)
    ctx, pooled, x0 = _cond(cfg, dev, seed=41)
    sp = ed.invert(ctx, x0, steps=STEPS, skip=0, guidance_scale=GS, seed=3, pooled=pooled)
    assert sp.timesteps == TS and sum(t <= START for t in TS) == LIVE
    return cfg, eng, ed, sp


class _Hand:
    """the launches of a direction step, driven from the public pieces"""

    def __init__(self, eng, ctx, pooled, dirs, q, momentum, scale, mode="off"):
        self.eng, self.J, self.mode, self.momentum = eng, len(dirs), mode, momentum
        self.R = 2 + 2 * self.J
        self.coef = dirs.coefficients(scale, GS, False)
        self.keep = DirectionSet.n_keep(PIX, q)
        d_ctx, d_pooled = dirs.rows(1, eng.device)
        self.cond, self.wide_cond = (ctx, pooled), (torch.cat([ctx, d_ctx]), torch.cat([pooled, d_pooled]))
        self.drv = Pass(eng, eng.plan(2, HW, HW, mode))
        self.drv.load_cond(ctx, pooled, None)
        self.wide = False
        self.guided = torch.empty(1, 4, HW, HW, dtype=torch.bfloat16, device=eng.device)
        self.thr = torch.empty(1, self.J, 4, dtype=torch.int32, device=eng.device)
        self.mom = None
        self.s = torch.cuda.current_stream().cuda_stream

    def widen(self, x):
        """-> the pass on the wide plan, the latent's bf16 rounding in every row block; the state starts at zero"""
        x = x.clone()
        self.drv = Pass(self.eng, self.eng.plan(self.R, HW, HW, self.mode))
        self.drv.load_cond(*self.wide_cond, None)
        self.drv.load_latents(x)
        self.wide = True
        if self.momentum is not None:
            self.mom = torch.zeros(1, CHW, dtype=torch.float32, device=self.eng.device)

    def guide(self):
        eps = self.drv.io["eps"].ptr
        pos = [eps + (2 + 2 * k) * CHW * 2 for k in range(self.J)]
        neg = [eps + (3 + 2 * k) * CHW * 2 for k in range(self.J)]
        if self.keep < PIX:
            lib.direction_threshold(self.s, pos=pos, neg=neg, thr=self.thr.data_ptr(), n_keep=[self.keep] * self.J, nb=1, chw=CHW, hw=PIX)
        rows = dict(t=eps + CHW * 2, out=self.guided.data_ptr(), pos=pos, neg=neg, c=self.coef, nb=1, chw=CHW, hw=PIX,
                    thr=self.thr.data_ptr() if self.keep < PIX else 0)
        if self.momentum is None:
            lib.eps_direction(self.s, **rows)
        else:
            lib.eps_direction_momentum(self.s, mom_in=self.mom.data_ptr(), mom_out=self.mom.data_ptr(), s_m=self.momentum[0],
                                       beta=self.momentum[1], **rows)
        return self.guided.data_ptr()

    def spread(self):
        smp = self.drv.io["sample"].tensor
        smp[2:].copy_(smp[:1].expand(self.R - 2, -1, -1, -1))


def _hand_edit(h: _Hand, sp, scale, start_noise, mask=None, store=False):
    sch = DDIMSchedule()
    x = sp.x_start.clone()
    h.drv.load_latents(x)
    for i, t in enumerate(sp.timesteps):
        first, live = i == 0, t <= start_noise
        if store:
            h.eng.set_lora(True, scale if live else 0.0)
        if live and not h.wide:
            h.widen(x)
            first = True
        h.drv.run(t, first, h.s)
        buf, eps = h.drv.io["sample"], h.drv.io["eps"]
        common = dict(eps=eps.ptr, eps_text=h.guide() if live else 0, x=x.data_ptr(), resid=sp.resid[i].data_ptr(), out=x.data_ptr(),
                      out_bf16=buf.ptr, out2_bf16=buf.ptr + CHW * 2, nb=1, chw=CHW, guidance=GS, v_prediction=0,
                      **fp32_coefficients(ddpm_step_coefficients(sch, t, STEPS, 1.0)))
        if mask is None:
            lib.call(lib.OP_DDPM_EDIT, lib.DdpmEditDesc(target=0, mode=1, **common), h.s)
        else:
            lib.call(lib.OP_DDPM_EDIT_BLEND, lib.DdpmEditBlendDesc(keep=sp.visited[i].data_ptr(), mask=mask.data_ptr(), hw=PIX, **common), h.s)
        if live:
            h.spread()
    if store:
        h.eng.set_lora(False)
    return x


# ---------------------------------------------------------------------------------------------------------------------------
# null cases
# ---------------------------------------------------------------------------------------------------------------------------
def test_directions_that_do_not_act_are_the_reconstruction(dev, engine, monkeypatch):
    cfg, eng, ed, sp = engine
    dirs = _directions(cfg, dev, 2)
    eng.flush_plans()
    launches = []
    for name in ("eps_direction", "eps_direction_momentum", "direction_threshold"):
        monkeypatch.setattr(lib, name, lambda *a, _n=name, **k: launches.append(_n))
    steer = dict(directions=dirs, direction_quantile=0.9, direction_momentum=MOMENTUM)
    for kw in (dict(scale=0.0, start_noise=START), dict(scale=SCALE, start_noise=-1)):
        assert torch.equal(ed.edit_latents(sp, **kw, **steer), sp.recon), kw
    assert _plans(eng) == [2] and not launches, "no wide plan, no direction launch"
    with pytest.raises(ValueError, match="expected 0 <= q < 1"):
        ed.edit_latents(sp, scale=0.0, directions=dirs, direction_quantile=1.0)
    with pytest.raises(ValueError, match="0 <= beta < 1"):
        ed.edit_latents(sp, scale=0.0, directions=dirs, direction_momentum=(0.5, 1.0))
    with pytest.raises(ValueError, match="without directions"):
        ed.edit_latents(sp, scale=0.0, direction_momentum=MOMENTUM)


# ---------------------------------------------------------------------------------------------------------------------------
# the chain against a loop driven here from the public pieces
# ---------------------------------------------------------------------------------------------------------------------------
def test_editor_against_a_loop_of_the_public_pieces(dev, engine):
    cfg, eng, ed, sp = engine
    run = dict(scale=SCALE, start_noise=START)
    base = ed.edit_latents(sp, **run)
    assert torch.equal(base, sp.recon), "no slider: the edit without directions is the reconstruction"
    seen = []
    for J, q, momentum in ((1, 0.0, None), (2, 0.9, None), (1, 0.9, MOMENTUM), (2, 0.0, MOMENTUM), (1, 0.0, MOMENTUM), (2, 0.9, MOMENTUM),
                           (1, 0.9, None), (2, 0.0, None)):
        dirs = _directions(cfg, dev, J)
        steer = dict(directions=dirs, direction_quantile=q, direction_momentum=momentum)
        eng.flush_plans()
        got = ed.edit_latents(sp, **run, **steer)
        assert 2 + 2 * J in _plans(eng) and set(_plans(eng)) <= {2, 2 + 2 * J}, "one wide plan, of 2 J more blocks"
        want = _hand_edit(_Hand(eng, sp.ctx, sp.pooled, dirs, q, momentum, SCALE), sp, SCALE, START)
        assert got.dtype == torch.float32 and got.shape == sp.recon.shape and bool(torch.isfinite(got).all())
        assert torch.equal(got, want), (J, q, momentum)
        assert not torch.equal(got, base), "the directions act"
        assert all(not torch.equal(got, o) for o in seen), "J, the quantile and the momentum matter"
        seen.append(got)
        # the pairs the other way round at the opposite scale: d and c change sign, the keys read |d|, the state is the same
        assert torch.equal(ed.edit_latents(sp, scale=-SCALE, start_noise=START, **{**steer, "directions": dirs.swapped()}), got)
    # a second call over a warm plan cache: the same bits, and the state started at zero again
    assert torch.equal(ed.edit_latents(sp, **run, **steer), seen[-1])
    assert torch.equal(ed.edit_latents(sp, scale=0.0), sp.recon), "the editor is as it was"


def test_a_slider_next_to_the_directions(dev, tiny):
    """store= stays legal: the adapter acts on every row of the wide pass at the edit's scale, and is off again afterwards"""
    cfg, _, eng, store, _ = tiny
    ed = SliderEditor(eng, store)
    ctx, pooled, x0 = _cond(cfg, dev, seed=42)
    sp = ed.invert(ctx, x0, steps=STEPS, skip=0, guidance_scale=GS, seed=5, pooled=pooled)
    dirs = _directions(cfg, dev, 1)
    steer = dict(directions=dirs, direction_quantile=0.9, direction_momentum=MOMENTUM)
    slider = ed.edit_latents(sp, scale=SCALE, start_noise=START)
    both = ed.edit_latents(sp, scale=SCALE, start_noise=START, **steer)
    assert bool(torch.isfinite(both).all()) and not torch.equal(both, slider) and not torch.equal(slider, sp.recon)
    want = _hand_edit(_Hand(eng, ctx, pooled, dirs, 0.9, MOMENTUM, SCALE, mode="on"), sp, SCALE, START, store=True)
    assert torch.equal(both, want)
    assert (4, HW, HW, "on") in eng._plans and not eng.lora_active and float(eng.lora_scale) == 0.0
    assert torch.equal(ed.edit_latents(sp, scale=0.0, **steer), sp.recon)


# ---------------------------------------------------------------------------------------------------------------------------
# mask; momentum off
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum", [None, MOMENTUM])
def test_mask(dev, engine, momentum):
    cfg, eng, ed, sp = engine
    dirs = _directions(cfg, dev, 2)
    run = dict(scale=SCALE, start_noise=START, directions=dirs, direction_quantile=0.5, direction_momentum=momentum)
    plain = ed.edit_latents(sp, **run)
    half = torch.zeros(HW, HW)
    half[:, HW // 2:] = 1.0
    out = ed.edit_latents(sp, mask=half, **run)
    assert torch.equal(out[..., :HW // 2], sp.recon[..., :HW // 2]), "outside the mask: the reconstruction, bit for bit"
    assert not torch.equal(out[..., HW // 2:], sp.recon[..., HW // 2:])
    assert torch.equal(out, _hand_edit(_Hand(eng, sp.ctx, sp.pooled, dirs, 0.5, momentum, SCALE), sp, SCALE, START, mask=half.to(dev).contiguous()))
    assert torch.equal(ed.edit_latents(sp, mask=torch.ones(HW, HW), **run), plain), "an all-one mask is the unmasked edit"
    assert torch.equal(ed.edit_latents(sp, mask=torch.zeros(HW, HW), **run), sp.recon)
    bare = NoiseSpace(**{**sp._map(lambda t: t), "visited": None})          # a file saved before masked edits
    assert torch.equal(ed.edit_latents(bare, mask=half, **run), out) and torch.equal(bare.visited, sp.visited), "trajectory refills visited"


def test_a_momentum_of_zero_is_no_momentum(dev, engine, monkeypatch):
    cfg, eng, ed, sp = engine
    dirs = _directions(cfg, dev, 2)
    run = dict(scale=SCALE, start_noise=START, directions=dirs, direction_quantile=0.9)
    none = ed.edit_latents(sp, **run)
    launches = []
    real = {n: getattr(lib, n) for n in ("eps_direction", "eps_direction_momentum")}
    for n, fn in real.items():
        monkeypatch.setattr(lib, n, lambda *a, _n=n, _fn=fn, **k: (launches.append(_n), _fn(*a, **k))[1])
    assert torch.equal(ed.edit_latents(sp, direction_momentum=(0.0, 0.4), **run), none)
    assert launches == ["eps_direction"] * LIVE
    del launches[:]
    assert not torch.equal(ed.edit_latents(sp, direction_momentum=MOMENTUM, **run), none)
    assert launches == ["eps_direction_momentum"] * LIVE


# ---------------------------------------------------------------------------------------------------------------------------
# the sampler's momentum
# ---------------------------------------------------------------------------------------------------------------------------
def test_sampler_momentum(dev, engine):
    cfg, eng, _, _ = engine
    ctx, pooled, noise = _cond(cfg, dev, seed=43)
    dirs = _directions(cfg, dev, 2)
    smp = SliderSampler(eng, scheduler="ddim")
    run = dict(scale=SCALE, start_noise=START, ddim_steps=STEPS, guidance_scale=GS, pooled=pooled, directions=dirs, direction_quantile=0.9)
    none = smp.sample_latents(ctx, noise, **run)
    assert torch.equal(smp.sample_latents(ctx, noise, direction_momentum=(0.0, 0.4), **run), none)
    got = smp.sample_latents(ctx, noise, direction_momentum=MOMENTUM, **run)
    assert not torch.equal(got, none)
    # by hand: the fused DDIM loop in place on the plan's input buffer
    h = _Hand(eng, ctx, pooled, dirs, 0.9, MOMENTUM, SCALE)
    h.drv.load_latents(noise)
    for i, t in enumerate(TS):
        first, live = i == 0, t <= START
        if live and not h.wide:
            h.widen(h.drv.io["sample"].tensor[:1])
            first = True
        h.drv.run(t, first, h.s)
        buf, eps = h.drv.io["sample"], h.drv.io["eps"]
        lib.call(lib.OP_CFG_DDIM, lib.CfgDdimDesc(x=buf.ptr, out=buf.ptr, nb=1, chw=CHW, eps=eps.ptr, eps_text=h.guide() if live else 0,
                                                  out2=buf.ptr + CHW * 2, guidance=GS, **smp.sched.step_fields(int(t), STEPS)), h.s)
        if live:
            h.spread()
    assert torch.equal(got, h.drv.io["sample"].tensor[:1])
    with pytest.raises(ValueError, match="without directions"):
        smp.sample_latents(ctx, noise, scale=SCALE, ddim_steps=STEPS, guidance_scale=GS, pooled=pooled, direction_momentum=MOMENTUM)


# ---------------------------------------------------------------------------------------------------------------------------
# the footprint
# ---------------------------------------------------------------------------------------------------------------------------
def test_footprint_of_a_direction(dev, engine, monkeypatch):
    cfg, eng, ed, sp = engine
    dirs = _directions(cfg, dev, 2)
    idx = footprint_draws(sp.timesteps, START, 2, 100)
    assert len(idx) == 2
    runs = []
    real_run = Pass.run
    monkeypatch.setattr(Pass, "run", lambda self, *a: (runs.append(self.p.B), real_run(self, *a))[1])
    F = ed.footprint(sp, SCALE, start_noise=START, draws=2, t_min=100, directions=dirs, direction_quantile=0.9)
    assert runs == [6] * len(idx), "one wide pass per draw"
    monkeypatch.setattr(Pass, "run", real_run)
    assert F.shape == (1, HW, HW) and bool(torch.isfinite(F).all()) and float(F.min()) >= 0.0 and float(F.max()) > float(F.min())
    # by hand: u, t and the guided row t' of each draw's wide pass; the pair (u, t') against the pair (u, t)
    h = _Hand(eng, sp.ctx, sp.pooled, dirs, 0.9, None, SCALE)
    A = torch.full((len(idx), 1, HW, HW), float("nan"), device=dev)
    for n, i in enumerate(idx):
        x = sp.x_start if i == 0 else sp.visited[i - 1]
        if n == 0:
            h.widen(x)
        h.drv.load_latents(x)
        h.drv.run(sp.timesteps[i], n == 0, h.s)
        eps = h.drv.io["eps"].ptr
        lib.call(lib.OP_EPS_ABSDIFF, lib.EpsAbsdiffDesc(eps_a=eps, eps_a_text=h.guide(), eps_b=eps, eps_b_text=eps + CHW * 2, out=A[n].data_ptr(),
                                                        nb=1, chw=CHW, hw=PIX, guidance=GS), h.s)
    assert torch.equal(F, footprint_mean(A))
    # the sampler's entry point over a trace, and the editor as it was
    smp = SliderSampler(eng, scheduler="ddim")
    ctx, pooled, noise = _cond(cfg, dev, seed=44)
    trace = smp.base_trace(ctx, noise, STEPS, GS, pooled, None, START)
    T = smp.footprint(trace, SCALE, start_noise=START, draws=2, t_min=100, directions=dirs)
    assert T.shape == (1, HW, HW) and float(T.max()) > float(T.min())
    Z = ed.footprint(sp, 0.0, start_noise=START, draws=2, t_min=100, directions=dirs)
    assert torch.equal(Z, torch.zeros_like(Z)), "scale 0: t' has t's bits"
    assert torch.equal(ed.edit_latents(sp, scale=0.0), sp.recon)


# ---------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------
def test_cli(dev, tmp_path, monkeypatch):
    from PIL import Image
    import sliders_amd.model_util as mu
    cfg = CONFIGS["tiny_sd1"]()
    engines = {}

    def tiny_engine(model, device, seed):     # --synthetic on the tiny SD-1 topology, built once for the runs below
        if seed not in engines:
            engines[seed] = UNetEngine(cfg, mu.random_state_dict(cfg, device, seed), device)
        return engines[seed]
    monkeypatch.setattr(mu, "synthetic_engine", tiny_engine)
    img = str(tmp_path / "photo.png")
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (128, 128, 3), dtype=np.uint8)).save(img)
    inv = str(tmp_path / "inversion.pt")
    common = ["--model", "sd1", "--synthetic", "--steps", "6", "--skip", "0", "--start_noise", str(START), "--guidance_scale", "3", "--res", "128"]
    read = lambda out, names: [open(os.path.join(out, n), "rb").read() for n in names]
    plain = edit.main(common + ["--image", img, "--scales=0", "--save_inversion", inv, "--out", str(tmp_path / "plain")])
    steer = ["--direction", "a|b:2"]
    out = edit.main(common + steer + ["--inversion", inv, "--scales=-1,0,1", "--out", str(tmp_path / "steer")])
    names = ["scale_-1.png", "scale_0.png", "scale_1.png"]
    assert sorted(os.listdir(out)) == sorted(names + ["recon.png"])
    got = read(out, names)
    assert got[1] == read(plain, ["scale_0.png"])[0], "scale 0 is the image without --direction"
    assert got[0] != got[1] != got[2] != got[0]
    assert 4 in _plans(engines[0]), "one direction next to the CFG pair: four row blocks"
    # a momentum of 0 changes no file
    zero = edit.main(common + steer + ["--inversion", inv, "--scales=-1,0,1", "--direction_momentum", "0", "--out", str(tmp_path / "zero")])
    assert read(zero, names + ["recon.png"]) == read(out, names + ["recon.png"])
    mom = edit.main(common + steer + ["--inversion", inv, "--scales=1", "--direction_momentum", "0.5", "--direction_quantile", "0.8",
                                      "--out", str(tmp_path / "mom")])
    assert read(mom, ["scale_1.png"])[0] != got[2]
    # the direction's footprint as the mask
    saved = str(tmp_path / "auto.png")
    auto = edit.main(common + steer + ["--inversion", inv, "--scales=0,1", "--auto_mask", "--auto_mask_draws", "2", "--save_mask", saved,
                                       "--out", str(tmp_path / "auto")])
    m = np.asarray(Image.open(saved))
    assert m.shape == (16, 16) and m.dtype == np.uint8 and m.max() > 0
    two = read(auto, ["scale_0.png", "scale_1.png"])
    assert two[0] == got[1] and two[1] != two[0]
    assert len(engines) == 1
