"""Localised sampling on the engine (docs/SAMPLING.md, "Localised sampling"): SliderSampler.base_trace, sample_latents(mask=, trace=,
share_prefix=) in both slider forms, the maps from a trace, and python -m sliders_amd.generate with the mask options.

Everything here is an identity of bits: the tiny SDXL at 16^2 latents, 6 steps, start_noise on the grid's third point (two shared steps,
four live ones), a rank-4 slider with non-zero up weights."""
import io
import os

import numpy as np
import pytest
import torch

from sliders_amd import edit, generate, lib, schedulers
from sliders_amd.config import CONFIGS
from sliders_amd.edit import NoiseSpace, SliderEditor
from sliders_amd.merge import SliderSet
from sliders_amd.passes import Pass
from sliders_amd.sampler import SampleTrace, SliderSampler
from sliders_amd.unet import UNetEngine
from tests.test_fewstep_sampler_gpu import HW, _inputs, tiny  # noqa: F401  (tiny: the module's fixture)
from tests.test_merge_gpu import drawn_slider

pytestmark = pytest.mark.gpu

STEPS, LIVE, SCALE, GS, SEED = 6, 4, 2.0, 3.0, 7
FP32 = {"ddim": None, "euler": "fp32", "euler_a": "fp32", "ddpm": "fp32", "lms": "fp32", "dpmpp_2m": "fp32"}
HISTORY = ("lms", "dpmpp_2m")


@pytest.fixture(scope="module")
def forms(dev, tiny):
    """(cfg, {form: (engine, sampler keywords)}): the fused rank-4 adapters (store=) and the same slider merged into the weights
    (sliders=, an engine of its own)"""
    cfg, net, eng, store, sd = tiny
    eng2 = UNetEngine(cfg, net.state_dict(), dev)
    return cfg, {"store": (eng, lambda: {"store": store}), "sliders": (eng2, lambda: {"sliders": SliderSet(cfg, [(sd, None)])})}


def _sampler(forms, form, scheduler):
    eng, kw = forms[1][form]
    return SliderSampler(eng, scheduler=scheduler, scheduler_seed=SEED, latents=FP32[scheduler], **kw())


def _grid(smp):
    if smp.sched.fused:
        return [float(t) for t in smp.sched.make_timesteps(STEPS)]
    smp.sched.set_timesteps(STEPS)
    return smp.sched.timesteps.tolist()


def _cond(cfg, dev, single=False, seed=21):
    unc, txt, pu, pt, noise = _inputs(cfg, 1, seed=seed)
    ctx, pooled = (txt, pt) if single else (torch.cat([unc, txt]), torch.cat([pu, pt]))
    return ctx.to(dev), pooled.to(dev), noise.to(dev)


def _idle(smp, snap=None):
    """the adapter is off, nothing is merged, the weight bits are the original ones"""
    eng = smp.eng
    assert not eng.lora_active and eng.lora_scale_host == 0.0 and float(eng.lora_scale) == 0.0
    if smp.merger is not None:
        assert not smp.merger.merged
        assert all(torch.equal(v, snap[k]) for k, v in eng.w.t.items()), "the original weight bits are back"


@pytest.mark.parametrize("scheduler", ["ddim", "euler", "euler_a", "dpmpp_2m"])
def test_base_trace_ends_on_the_scale_0_bits(dev, forms, scheduler):
    cfg = forms[0]
    ctx, pooled, noise = _cond(cfg, dev)
    run = dict(ddim_steps=STEPS, guidance_scale=GS, pooled=pooled)
    trace = _sampler(forms, "store", scheduler).base_trace(ctx, noise, **run)
    want = _sampler(forms, "store", scheduler).sample_latents(ctx, noise, scale=0.0, **run)       # a fresh sampler: the same draws
    assert isinstance(trace, SampleTrace) and trace.final.dtype == torch.bfloat16 and torch.equal(trace.final, want)
    loop = torch.float32 if FP32[scheduler] else torch.bfloat16
    assert trace.visited.shape == (STEPS,) + tuple(noise.shape) and trace.visited.dtype == loop and trace.x_start.dtype == loop
    assert torch.equal(trace.visited[-1].to(torch.bfloat16), trace.final) and trace.steps == STEPS and not trace.single
    assert (trace.draws is not None) == (scheduler == "euler_a") and trace.guidance == GS
    assert torch.isfinite(trace.visited.float()).all()
    _idle(_sampler(forms, "store", scheduler))


@pytest.mark.parametrize("form", ["store", "sliders"])
@pytest.mark.parametrize("scheduler", ["ddim", "euler", "euler_a", "ddpm", "lms", "dpmpp_2m"])
def test_masked_sampling_identities(dev, forms, scheduler, form, monkeypatch):
    cfg = forms[0]
    ctx, pooled, noise = _cond(cfg, dev)
    smp = _sampler(forms, form, scheduler)
    snap = {k: v.clone() for k, v in smp.eng.w.t.items()} if form == "sliders" else None
    start_noise = _grid(smp)[STEPS - LIVE]
    run = dict(start_noise=start_noise, ddim_steps=STEPS, guidance_scale=GS, pooled=pooled)
    runs = []
    real_run = Pass.run
    monkeypatch.setattr(Pass, "run", lambda self, *a: (runs.append(a[0]), real_run(self, *a))[1])
    blends = []
    real_blend = lib.latent_blend
    monkeypatch.setattr(lib, "latent_blend", lambda *a, **k: (blends.append(k["keep"]), real_blend(*a, **k))[1])

    trace = smp.base_trace(ctx, noise, STEPS, GS, pooled, None, start_noise)
    _idle(smp, snap)
    assert len(runs) == STEPS and not blends
    base = trace.final
    plain = _sampler(forms, form, scheduler).sample_latents(ctx, noise, scale=SCALE, **run)       # a fresh sampler: the trace's draws
    _idle(smp, snap)
    assert not torch.equal(plain, base), "the slider acts"
    shared = STEPS if scheduler in HISTORY else LIVE

    def masked(mask, **kw):
        runs.clear(), blends.clear()
        out = smp.sample_latents(ctx, noise, scale=SCALE, mask=mask, trace=trace, **run, **kw)
        _idle(smp, snap)
        assert out.dtype == torch.bfloat16 and out.shape == noise.shape
        return out

    # an all-zero mask: the base chain's bits; one blend per live step, against that step's visited latent
    out = masked(torch.zeros(HW, HW))
    assert torch.equal(out, base)
    assert len(runs) == shared and blends == [trace.visited[i].data_ptr() for i in range(STEPS - LIVE, STEPS)]
    assert [float(t) for t in runs] == [float(t) for t in _grid(smp)[STEPS - shared:]]
    # an all-one mask: the unmasked run at that scale
    assert torch.equal(masked(torch.ones(1, HW, HW)), plain)
    # a half-plane: the kept half is the base, the other half is not
    half = torch.zeros(1, 1, HW, HW)
    half[..., HW // 2:] = 1.0
    out = masked(half)
    assert torch.equal(out[..., :HW // 2], base[..., :HW // 2]) and not torch.equal(out[..., HW // 2:], base[..., HW // 2:])
    # a fractional mask: the shared prefix changes no bit, and is not replayed
    frac = torch.rand(HW, HW, generator=torch.Generator().manual_seed(3)).clamp(0.05, 0.95)
    a = masked(frac)
    assert len(runs) == shared
    b = masked(frac, share_prefix=False)
    assert len(runs) == STEPS and len(blends) == LIVE
    assert torch.equal(a, b) and not torch.equal(a, base) and not torch.equal(a, plain)
    # a trace without a mask: the unmasked run from the shared prefix, the same bits
    runs.clear()
    assert torch.equal(smp.sample_latents(ctx, noise, scale=SCALE, trace=trace, **run), plain) and len(runs) == shared
    # a mask without a trace builds one (the scheduler's next draws: deterministic schedulers give the same bits)
    if scheduler not in ("euler_a", "ddpm"):
        runs.clear()
        assert torch.equal(smp.sample_latents(ctx, noise, scale=SCALE, mask=frac, **run), a) and len(runs) == STEPS + shared
    _idle(smp, snap)


def test_single_branch_and_start_noise_below_the_grid(dev, forms):
    cfg = forms[0]
    ctx, pooled, noise = _cond(cfg, dev, single=True)
    smp = _sampler(forms, "store", "euler_a")
    start_noise = _grid(smp)[STEPS - LIVE]
    run = dict(start_noise=start_noise, ddim_steps=STEPS, pooled=pooled)
    trace = smp.base_trace(ctx, noise, STEPS, GS, pooled)
    assert trace.single
    plain = _sampler(forms, "store", "euler_a").sample_latents(ctx, noise, scale=SCALE, **run)
    half = torch.zeros(HW, HW)
    half[HW // 2:] = 1.0
    out = smp.sample_latents(ctx, noise, scale=SCALE, mask=half, trace=trace, **run)
    assert torch.equal(out[:, :, :HW // 2], trace.final[:, :, :HW // 2]) and not torch.equal(out[:, :, HW // 2:], trace.final[:, :, HW // 2:])
    assert torch.equal(smp.sample_latents(ctx, noise, scale=SCALE, mask=torch.ones(HW, HW), trace=trace, **run), plain)
    # the slider never acts: the base image
    assert torch.equal(smp.sample_latents(ctx, noise, scale=SCALE, mask=half, trace=trace, **dict(run, start_noise=-1)), trace.final)
    # a trace of another run is refused
    pair_ctx, pair_pooled, _ = _cond(cfg, dev)
    with pytest.raises(ValueError, match="the trace has 6 steps"):
        smp.sample_latents(pair_ctx, noise, scale=SCALE, mask=half, trace=trace, ddim_steps=STEPS, pooled=pair_pooled)
    with pytest.raises(ValueError, match="the trace has 6 steps"):
        smp.sample_latents(ctx, noise, scale=SCALE, mask=half, trace=trace, ddim_steps=4, pooled=pooled)
    with pytest.raises(ValueError, match="mask of shape"):
        smp.sample_latents(ctx, noise, scale=SCALE, mask=torch.ones(3, 3), trace=trace, **run)
    _idle(smp)


def test_the_bf16_tensor_op_path_refuses_a_mask(dev, forms):
    cfg = forms[0]
    ctx, pooled, noise = _cond(cfg, dev)
    for scheduler in ("euler", "lms"):
        eng, kw = forms[1]["store"]
        smp = SliderSampler(eng, scheduler=scheduler, **kw())
        assert smp.latents == "bf16"
        with pytest.raises(ValueError, match="--fp32_latents"):
            smp.sample_latents(ctx, noise, scale=SCALE, mask=torch.ones(HW, HW), ddim_steps=STEPS, pooled=pooled)
        with pytest.raises(ValueError, match="--fp32_latents"):
            smp.base_trace(ctx, noise, STEPS, GS, pooled)
        _idle(smp)


# ---------------------------------------------------------------------------------------------------------------------------
# the masked chain against a loop driven here from the public pieces: which buffer, which step, which visited[i]
# ---------------------------------------------------------------------------------------------------------------------------
def _hand_loop(smp, ctx, pooled, trace, mask, start_noise):
    eng = smp.eng
    p = eng.plan(2, HW, HW, "on")
    drv = Pass(eng, p)
    drv.load_cond(ctx, pooled, None)
    buf, eps = p.io["sample"], p.io["eps"]
    s = torch.cuda.current_stream().cuda_stream
    chw, hw = 4 * HW * HW, HW * HW
    m = edit.as_mask(mask, 1, HW, HW).to(eng.device)
    ts = _grid(smp)
    fp32 = smp.latents == "fp32"
    if fp32:
        rows = [schedulers.step_row(smp.sched, i, STEPS) for i in range(STEPS)]
        x = trace.x_start.clone()
        drv.load_latents(smp.sched.scale_model_input(x, smp.sched.timesteps[0]))
    else:
        drv.load_latents(trace.x_start)
    for i, t in enumerate(ts):
        live = t <= start_noise
        eng.set_lora(True, SCALE if live else 0.0)
        drv.run(t, i == 0, s)
        if fp32:
            r = rows[i]
            lib.sigma_step(s, eps=eps.ptr, x=x.data_ptr(), out=x.data_ptr(), nb=1, chw=chw, kind=r.kind, p=r.p, q=r.q, sigma=r.sigma, a=r.a, c=r.c,
                           c_n=r.c_n, s_next=r.s_next, guidance=GS, noise=trace.draws[i].data_ptr() if r.c_n != 0.0 else 0, in_bf16=buf.ptr,
                           in2_bf16=buf.ptr + chw * 2)
            if live:
                lib.latent_blend(s, e=x.data_ptr(), keep=trace.visited[i].data_ptr(), mask=m.data_ptr(), out=x.data_ptr(), nb=1, chw=chw, hw=hw,
                                 fp32=True, s_next=r.s_next, in_bf16=buf.ptr, in2_bf16=buf.ptr + chw * 2)
        else:
            d = lib.CfgDdimDesc(eps=eps.ptr, x=buf.ptr, out=buf.ptr, out2=buf.ptr + chw * 2, nb=1, chw=chw, guidance=GS,
                                **smp.sched.step_fields(int(t), STEPS))
            lib.call(lib.OP_CFG_DDIM, d, s)
            if live:
                lib.latent_blend(s, e=buf.ptr, keep=trace.visited[i].data_ptr(), mask=m.data_ptr(), out=buf.ptr, nb=1, chw=chw, hw=hw, fp32=False,
                                 in_bf16=buf.ptr + chw * 2)
    eng.set_lora(False)
    return x.to(torch.bfloat16) if fp32 else buf.tensor[:1].clone()


@pytest.mark.parametrize("scheduler", ["ddim", "euler_a"])
def test_fractional_mask_against_a_loop_of_the_public_pieces(dev, forms, scheduler):
    cfg = forms[0]
    ctx, pooled, noise = _cond(cfg, dev, seed=22)
    smp = _sampler(forms, "store", scheduler)
    start_noise = _grid(smp)[STEPS - LIVE]
    trace = smp.base_trace(ctx, noise, STEPS, GS, pooled)
    frac = torch.rand(1, HW, HW, generator=torch.Generator().manual_seed(5))
    frac[0, 0, :4] = torch.tensor([0.0, 1.0, 0.0, 1.0])
    got = smp.sample_latents(ctx, noise, scale=SCALE, start_noise=start_noise, ddim_steps=STEPS, guidance_scale=GS, pooled=pooled, mask=frac,
                             trace=trace)
    want = _hand_loop(smp, ctx, pooled, trace, frac, start_noise)
    assert torch.equal(got, want) and not torch.equal(got, trace.final)
    _idle(smp)


# ---------------------------------------------------------------------------------------------------------------------------
# masks from the slider or a word, without an inversion
# ---------------------------------------------------------------------------------------------------------------------------
def test_maps_from_a_trace_are_the_editors_maps(dev, forms):
    """a ddim trace dressed as a NoiseSpace: the editor's footprint and word map over it are the sampler's over the trace, bit for bit"""
    cfg = forms[0]
    eng, kw = forms[1]["store"]
    ctx, pooled, noise = _cond(cfg, dev, seed=23)
    smp = _sampler(forms, "store", "ddim")
    trace = smp.base_trace(ctx, noise, STEPS, GS, pooled)
    start_noise = _grid(smp)[STEPS - LIVE]
    F = smp.footprint(trace, SCALE, start_noise=start_noise, draws=2, t_min=100)
    W = smp.word_map(trace, tokens=[2, 3], draws=3)
    _idle(smp)
    assert F.shape == W.shape == (1, HW, HW) and F.dtype == W.dtype == torch.float32
    assert torch.isfinite(F).all() and bool((F >= 0).all()) and abs(float(F.mean()) - 1.0) < 1e-4, "every draw is divided by its mean"
    assert bool((W >= 0).all()) and bool((W <= 1).all()) and float(W.max()) > 0
    assert torch.equal(smp.footprint(trace, SCALE, start_noise=start_noise, draws=2, t_min=100), F)
    zero = torch.zeros_like(trace.visited, dtype=torch.float32)
    space = NoiseSpace(x0=zero[0], x_start=trace.x_start.float(), resid=zero, recon=trace.visited[-1].float(), timesteps=[int(t) for t in trace.timesteps],
                       steps=STEPS, skip=0, eta=1.0, guidance=GS, prediction_type="epsilon", seed=0, ctx=ctx, pooled=pooled, time_ids=None,
                       visited=trace.visited.float())
    ed = SliderEditor(eng, **kw())
    assert torch.equal(ed.footprint(space, SCALE, start_noise=int(start_noise), draws=2, t_min=100), F)
    assert torch.equal(ed.word_map(space, tokens=[2, 3], draws=3), W)
    m = edit.footprint_mask(F.cpu())
    assert m.shape == (1, HW, HW) and 0.0 < float(m.mean()) < 1.0
    # the sigma-space loops supply the scaled input: the same call on an fp32 trace
    smp = _sampler(forms, "store", "euler")
    trace = smp.base_trace(ctx, noise, STEPS, GS, pooled)
    F = smp.footprint(trace, SCALE, start_noise=_grid(smp)[STEPS - LIVE], draws=2, t_min=100)
    assert torch.isfinite(F).all() and abs(float(F.mean()) - 1.0) < 1e-4
    assert torch.equal(trace.unet_input(0).to(torch.bfloat16), smp.sched.scale_model_input(trace.x_start, smp.sched.timesteps[0]).to(torch.bfloat16))
    _idle(smp)


# ---------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------
def _pixels(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_cli(dev, tmp_path, monkeypatch):
    from PIL import Image
    import sliders_amd.model_util as mu
    from sliders_amd.lora_store import LoraStore
    from sliders_amd.vae import VAE_SCALING, VaeDecoder, random_vae_state_dict
    cfg = CONFIGS["tiny_sdxl"]()
    engines = {}

    def tiny_engine(model, device, seed):     # --synthetic on the tiny SDXL topology, built once for the runs below
        if seed not in engines:
            engines[seed] = UNetEngine(cfg, mu.random_state_dict(cfg, device, seed), device)
        return engines[seed]
    monkeypatch.setattr(mu, "synthetic_engine", tiny_engine)
    slider = str(tmp_path / "age_alpha1.0_rank4_noxattn.pt")
    torch.save(drawn_slider(cfg, "noxattn", 4, 1.0, 41), slider)
    half = np.zeros((128, 128), dtype=np.uint8)
    half[:, 64:] = 255
    files = {}
    for name, arr in (("half", half), ("black", np.zeros((16, 16), dtype=np.uint8))):
        files[name] = str(tmp_path / f"{name}.png")
        Image.fromarray(arr).save(files[name])
    scales = [-2.0, 0.0, 2.0]
    common = ["--synthetic", "--lora_weight", slider, "--scales=-2,0,2", "--res", "128", "--ddim_steps", "6", "--start_noise", "498",
              "--guidance_scale", "3"]
    names = [f"scale_{s:g}.png" for s in scales]
    read = lambda out: [open(os.path.join(out, n), "rb").read() for n in names]

    # without mask flags: the bytes of the call sequence this command line has always run - although a sweep that holds scale 0 keeps
    # it as a trace and does not replay the two steps above start_noise for the other scales
    runs = []
    real_run = Pass.run
    monkeypatch.setattr(Pass, "run", lambda self, *a: (runs.append(a[0]), real_run(self, *a))[1])
    plain = generate.main(common + ["--out", str(tmp_path / "plain")])
    assert sorted(os.listdir(plain)) == sorted(names)
    assert generate.shares_prefix(generate.build_parser().parse_args(common), scales) and len(runs) == STEPS + 2 * LIVE
    monkeypatch.setattr(Pass, "run", real_run)
    eng = tiny_engine("sdxl", dev, 0)
    dec = VaeDecoder(random_vae_state_dict(device=dev, seed=0, decoder=True), dev, VAE_SCALING["sdxl"])
    g = torch.Generator().manual_seed(0)
    ctx = torch.randn(2, 77, cfg.cross_attention_dim, generator=g)
    pooled = torch.randn(2, cfg.pooled_dim, generator=g)
    store = LoraStore(cfg, rank=4, alpha=1.0, train_method="noxattn", device=dev, init="none")
    store.load_state_dict(torch.load(slider, map_location="cpu"), strict=True)
    old = SliderSampler(eng, store, dec, scheduler="ddim", scheduler_seed=0)
    want = []
    for s in scales:
        noise = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(0))
        img = old.generate(ctx.to(dev), noise.to(dev), scale=s, start_noise=498, ddim_steps=6, guidance_scale=3.0, pooled=pooled.to(dev))
        buf = io.BytesIO()
        Image.fromarray(img[0].cpu().numpy()).save(buf, format="PNG")
        want.append(buf.getvalue())
    assert read(plain) == want
    assert want[0] != want[1] != want[2]

    # --mask: every scale, the saved mask, scale 0 the unmasked scale 0; an all-black mask keeps every scale on it
    saved = str(tmp_path / "half_latent.png")
    out = generate.main(common + ["--mask", files["half"], "--save_mask", saved, "--out", str(tmp_path / "half")])
    got = read(out)
    assert got[1] == want[1] and got[0] != want[0] and got[0] != got[1] and got[2] != got[1]
    m = np.zeros((16, 16), dtype=np.uint8)
    m[:, 8:] = 255
    assert np.array_equal(_pixels(saved), m)
    out = generate.main(common + ["--mask", files["black"], "--out", str(tmp_path / "black")])
    assert read(out) == [want[1]] * 3
    out = generate.main(common + ["--mask", files["black"], "--mask_invert", "--out", str(tmp_path / "white")])
    assert read(out) == want, "an all-white mask is the unmasked sweep"

    # --mask_tokens and --auto_mask: every scale and the saved mask
    for name, flags in (("tokens", ["--mask_tokens", "2,3", "--mask_word_draws", "2", "--save_attention", str(tmp_path / "attn.png")]),
                        ("auto", ["--auto_mask", "--auto_mask_draws", "2"])):
        saved = str(tmp_path / f"{name}_mask.png")
        out = generate.main(common + flags + ["--save_mask", saved, "--out", str(tmp_path / name)])
        got = read(out)
        m = _pixels(saved)
        assert m.shape == (16, 16) and m.dtype == np.uint8 and m.max() > 0, name
        assert got[1] == want[1] and all(len(b) > 0 for b in got), name
    assert _pixels(str(tmp_path / "attn.png")).shape == (16, 16)

    # the fp32 loops take the same flags
    out = generate.main(common + ["--scheduler", "euler_a", "--fp32_latents", "--mask", files["half"], "--out", str(tmp_path / "euler_a")])
    got = read(out)
    assert got[0] != got[1] != got[2]
    assert len(engines) == 1
