"""GPU: editing a given image with a slider (sliders_amd/edit.py) - slh_ddpm_edit_step element by element against the float64
reference, the bit-exact reconstruction on the engine in every slider form, the editor against loops written out here, the saved
inversion, the CLI.

Kernel bounds (docs/EDIT.md derives them): u = 2^-24, E = |eps_u| + g (|eps_t| + |eps_u|), S = the mu expression on absolute values,
n = 8 fp32 roundings on the longest path from the inputs to mu (the kernel contracts nothing):
    mode 0   |resid - (target - mu)| <= n u S + u (|target| + |mu|)        |out - target| <= 3 u (|target| + |mu|)
    mode 1   |out - (mu + resid)|    <= (n + 1) u (S + |resid|)
    both     the bf16 copies are out.to(bfloat16), bit for bit
"""
import itertools
import os

import numpy as np
import pytest
import torch

from oracle.unet_oracle import build_unet
from sliders_amd import edit, lib
from sliders_amd.config import CONFIGS
from sliders_amd.ddim import DDIMSchedule
from sliders_amd.edit import NoiseSpace, SliderEditor, ddpm_mu_reference, ddpm_step_coefficients, fp32_coefficients
from sliders_amd.lora_store import LoraStore
from sliders_amd.merge import SliderSet
from sliders_amd.unet import UNetEngine
from tests.test_bench_config_gpu import _nonzero_up
from tests.test_merge_gpu import drawn_slider
from tests.util import check_elementwise, stream

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N_OPS = 8
FENCE = 4096
GUIDANCE = 7.5
BF, F32 = torch.bfloat16, torch.float32


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel, element by element
# ---------------------------------------------------------------------------------------------------------------------------------
class Arena:
    """One allocation of 0xFF bytes (NaN in bf16 and in fp32), every buffer a view with >= 4 KiB of fence on each side"""

    def __init__(self, dev, sizes):
        self.off, pos = {}, FENCE
        for name, nbytes in sizes.items():
            self.off[name] = pos
            pos = (pos + nbytes + FENCE + 255) // 256 * 256
        self.sizes = sizes
        self.mem = torch.full((pos,), 0xFF, dtype=torch.uint8, device=dev)

    def view(self, name, dtype):
        return self.mem[self.off[name]:self.off[name] + self.sizes[name]].view(dtype)

    def ptr(self, name):
        return self.mem.data_ptr() + self.off[name]


def s_mu(f, ax, E, v):
    if v:
        return f["c_sqrt_alpha_prev"] * (f["c_sqrt_alpha_t"] * ax + f["c_sqrt_beta_t"] * E) + f["c_dir"] * (f["c_sqrt_alpha_t"] * E + f["c_sqrt_beta_t"] * ax)
    return f["c_sqrt_alpha_prev"] * f["c_inv_sqrt_alpha_t"] * (ax + f["c_sqrt_beta_t"] * E) + f["c_dir"] * E


def run_kernel_case(dev, nb, chw, mode, v, last, cls, sep_text=False, alias=False, seed=0):
    n = nb * chw
    g = torch.Generator().manual_seed(seed)
    big = 1e3 if cls == "large" else 1.0
    eps = torch.randn(2 * n, generator=g).to(BF)
    if cls == "zero_eps":
        eps.zero_()
    x = torch.randn(n, generator=g) * big
    target = torch.randn(n, generator=g) * big
    resid_in = torch.randn(n, generator=g) * big
    coef = ddpm_step_coefficients(DDIMSchedule(), 0 if last else 500, 50, 1.0)
    f = fp32_coefficients(coef)
    if last:
        assert f["c_dir"] == 0.0 and f["c_sqrt_alpha_prev"] == 1.0
    sizes = {"eps": 4 * n, "eps_text": 2 * n, "x": 4 * n, "target": 4 * n, "resid": 4 * n, "out": 4 * n, "out_bf16": 2 * n, "out2_bf16": 2 * n}
    ar = Arena(dev, sizes)
    ar.view("x", F32).copy_(x)
    ar.view("target", F32).copy_(target)
    if sep_text:
        # the text half lives elsewhere; what follows the uncond half is a decoy that must not be read
        ar.view("eps", BF)[:n].copy_(eps[:n])
        ar.view("eps", BF)[n:].fill_(1e4)
        ar.view("eps_text", BF).copy_(eps[n:])
    else:
        ar.view("eps", BF).copy_(eps)
    if mode == 1:
        ar.view("resid", F32).copy_(resid_in)
    outputs = (["resid"] if mode == 0 else []) + ["out_bf16", "out2_bf16"] + ([] if alias else ["out"])
    before = ar.mem.clone()
    out_name = "x" if alias else "out"
    d = lib.DdpmEditDesc(eps=ar.ptr("eps"), eps_text=ar.ptr("eps_text") if sep_text else 0, x=ar.ptr("x"), target=ar.ptr("target") if mode == 0 else 0,
                         resid=ar.ptr("resid"), out=ar.ptr(out_name), out_bf16=ar.ptr("out_bf16"), out2_bf16=ar.ptr("out2_bf16"), nb=nb, chw=chw,
                         guidance=GUIDANCE, mode=mode, v_prediction=int(v), **f)
    runs = []
    for _ in range(2):
        ar.mem.copy_(before)
        lib.call(lib.OP_DDPM_EDIT, d, stream())
        torch.cuda.synchronize()
        runs.append(ar.mem.clone())
    tag = f"nb {nb} chw {chw} mode {mode} {'v' if v else 'eps'} {'last' if last else 'mid'} {cls}{' eps_text' if sep_text else ''}{' alias' if alias else ''}"
    assert torch.equal(runs[0], runs[1]), f"{tag}: two runs differ"
    written = outputs + (["x"] if alias else [])
    keep = torch.ones_like(ar.mem, dtype=torch.bool)
    for nm in written:
        keep[ar.off[nm]:ar.off[nm] + ar.sizes[nm]] = False
    assert torch.equal(ar.mem[keep], before[keep]), f"{tag}: a byte outside the outputs changed (fences, inputs)"
    out = ar.view(out_name, F32).cpu()
    resid = ar.view("resid", F32).cpu()
    # float64 reference on the same bf16 / fp32 inputs and the fp32 scalars
    eu, et = eps[:n], eps[n:]
    mu = ddpm_mu_reference(eu, et, x, coef, GUIDANCE, v, torch.float64)
    E = eu.double().abs() + GUIDANCE * (et.double().abs() + eu.double().abs())
    S = s_mu(f, x.double().abs(), E, v)
    worst = {}
    if mode == 0:
        t64 = target.double()
        worst["resid"] = check_elementwise(f"{tag} resid", resid, t64 - mu, N_OPS * U * S + U * (t64.abs() + mu.abs()))[0]
        worst["out"] = check_elementwise(f"{tag} out", out, t64, 3 * U * (t64.abs() + mu.abs()))[0]
    else:
        r64 = resid_in.double()
        assert torch.equal(resid, resid_in), f"{tag}: mode 1 wrote resid"
        worst["out"] = check_elementwise(f"{tag} out", out, mu + r64, (N_OPS + 1) * U * (S + r64.abs()))[0]
    assert torch.equal(ar.view("out_bf16", BF).cpu(), out.to(BF)), f"{tag}: out_bf16 is not the rounding of out"
    assert torch.equal(ar.view("out2_bf16", BF).cpu(), out.to(BF)), f"{tag}: out2_bf16 is not the rounding of out"
    print(f"[edit-kernel] {tag}: worst err / bound " + ", ".join(f"{k} {w:.3f}" for k, w in worst.items()))
    return worst


@pytest.mark.parametrize("last", [False, True], ids=["mid", "last"])
@pytest.mark.parametrize("v", [False, True], ids=["eps", "v"])
@pytest.mark.parametrize("mode", [0, 1], ids=["invert", "edit"])
def test_ddpm_edit_step_per_element(dev, mode, v, last):
    for k, (nb, chw, cls) in enumerate(itertools.product((1, 2), (1, 900, 1024), ("normal", "large", "zero_eps"))):
        run_kernel_case(dev, nb, chw, mode, v, last, cls, seed=1000 * mode + 100 * v + 50 * last + k)


@pytest.mark.parametrize("what", ["eps_text", "alias"])
@pytest.mark.parametrize("mode", [0, 1], ids=["invert", "edit"])
def test_ddpm_edit_step_separate_text_half_and_in_place(dev, mode, what):
    run_kernel_case(dev, 2, 900, mode, False, False, "normal", sep_text=what == "eps_text", alias=what == "alias", seed=77 + mode)


def test_ddpm_edit_step_modes_agree_bit_for_bit(dev):
    """mode 1 over the residual mode 0 wrote, on the same inputs, gives mode 0's out: what the whole method rests on"""
    for v, last in itertools.product((False, True), (False, True)):
        n = 2 * 900
        g = torch.Generator().manual_seed(9)
        eps = torch.randn(2 * n, generator=g).to(BF).to(dev)
        x, target = (torch.randn(n, generator=g).to(dev) for _ in range(2))
        resid, o0, o1 = (torch.full((n,), float("nan"), device=dev) for _ in range(3))
        f = fp32_coefficients(ddpm_step_coefficients(DDIMSchedule(), 0 if last else 500, 50, 1.0))
        common = dict(eps=eps.data_ptr(), x=x.data_ptr(), resid=resid.data_ptr(), nb=2, chw=900, guidance=GUIDANCE, v_prediction=int(v), **f)
        lib.call(lib.OP_DDPM_EDIT, lib.DdpmEditDesc(target=target.data_ptr(), out=o0.data_ptr(), mode=0, **common), stream())
        lib.call(lib.OP_DDPM_EDIT, lib.DdpmEditDesc(out=o1.data_ptr(), mode=1, **common), stream())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o0).all()) and torch.equal(o0, o1), (v, last)


# ---------------------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------------------
HW, STEPS, SKIP, GS = 16, 8, 2, 5.0


def _inputs(cfg, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    ctx = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).to(dev)
    pooled = torch.randn(2, cfg.pooled_dim, generator=g).to(dev) if cfg.is_xl else None
    x0 = (torch.randn(1, 4, HW, HW, generator=g) * 0.8).to(dev)
    return ctx, pooled, x0


def _editor(name, form, dev, prediction_type="epsilon"):
    cfg = CONFIGS[name]()
    eng = UNetEngine(cfg, build_unet(name, seed=0).state_dict(), dev)
    kw = {}
    if form == "store":
        store = LoraStore(cfg, rank=4, alpha=1.0, train_method="noxattn", device=dev)
        _nonzero_up(store, dev)
        kw["store"] = store
    elif form == "sliders":
        kw["sliders"] = SliderSet(cfg, [(drawn_slider(cfg, "xattn", 8, 4.0, 21), None), (drawn_slider(cfg, "noxattn", 4, 1.0, 22), -1.0)])
    return cfg, eng, SliderEditor(eng, prediction_type=prediction_type, **kw)


def _recon_within_bound(space):
    err = (space.recon.double() - space.x0.double()).abs()
    bound = 2.0 ** -22 * (2.0 * space.x0.double().abs() + space.resid[-1].double().abs())
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} elements of recon beyond 2^-22 (2 |x0| + |d_last|)"
    return float((err / bound.clamp_min(1e-300)).max())


CASES = [(n, f, "epsilon") for n in ("tiny_sdxl", "tiny_sd1") for f in ("store", "sliders", "none")] + [("tiny_sd1", "none", "v_prediction")]


@pytest.mark.parametrize("name,form,prediction", CASES)
def test_scale_zero_reproduces_the_inversion_on_the_engine(dev, monkeypatch, name, form, prediction):
    cfg, eng, ed = _editor(name, form, dev, prediction)
    ctx, pooled, x0 = _inputs(cfg, dev)
    snap = {k: v.clone() for k, v in eng.w.t.items()} if form == "sliders" else None
    restored = lambda: not ed.merger.merged and all(torch.equal(v, snap[k]) for k, v in eng.w.t.items())
    sp = ed.invert(ctx, x0, steps=STEPS, skip=SKIP, guidance_scale=GS, seed=3, pooled=pooled)
    torch.cuda.synchronize()
    assert sp.timesteps == [625, 500, 375, 250, 125, 0] and sp.resid.shape == (6, 1, 4, HW, HW) and sp.resid.dtype == torch.float32
    assert sp.prediction_type == prediction and torch.equal(sp.x0, x0) and bool(torch.isfinite(sp.resid).all())
    assert torch.equal(ed.edit_latents(sp, scale=0.0), sp.recon), "scale 0 must walk the inversion's latents again, bit for bit"
    ratio = _recon_within_bound(sp)
    a = ed.edit_latents(sp, scale=1.5, start_noise=500)
    b = ed.edit_latents(sp, scale=1.5, start_noise=500)
    assert a.dtype == torch.float32 and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    if form != "none":
        assert not torch.equal(a, sp.recon), "the slider has an effect"
    else:
        assert torch.equal(a, sp.recon), "no slider: every scale is the reconstruction"
    assert torch.equal(ed.edit_latents(sp, scale=1.5, start_noise=-1), sp.recon), "the slider never switches on"
    assert torch.equal(ed.edit_latents(sp, ctx=ctx, scale=0.0, guidance_scale=GS, pooled=pooled), sp.recon), "the same conditioning, passed in"
    other = ed.edit_latents(sp, scale=0.0, guidance_scale=GS + 1.0)
    assert bool(torch.isfinite(other).all()) and not torch.equal(other, sp.recon), "another guidance is another image"
    print(f"[edit-engine] {name} {form} {prediction}: worst |recon - x0| / bound {ratio:.3f}, "
          f"|edit(1.5) - recon| max {float((a - sp.recon).abs().max()):.3e}")
    if form != "sliders":
        return
    assert restored(), "every weight tensor has its original bits after the edits"

    class Boom(RuntimeError):
        pass
    real, calls = edit.ddpm_step_coefficients, []

    def failing(*a, **k):
        calls.append(1)
        if len(calls) == 3:
            assert ed.merger.merged, "the test must fail inside the loop, on merged weights"
            raise Boom()
        return real(*a, **k)
    monkeypatch.setattr(edit, "ddpm_step_coefficients", failing)
    with pytest.raises(Boom):
        ed.edit_latents(sp, scale=1.5, start_noise=2000)
    torch.cuda.synchronize()
    monkeypatch.setattr(edit, "ddpm_step_coefficients", real)
    assert restored(), "an exception inside the loop still restores the weights"
    assert torch.equal(ed.edit_latents(sp, scale=0.0), sp.recon)


def _hand_inputs(eng, p, ctx, pooled):
    io = p.io
    io["ctx"].tensor.copy_(ctx.to(BF))
    if eng.cfg.is_xl:
        io["time_ids"].tensor.copy_(torch.tensor([[HW * 8.0, HW * 8.0, 0.0, 0.0, HW * 8.0, HW * 8.0]] * 2).to(eng.device))
        io["add_in"].tensor[:, : eng.cfg.pooled_dim].copy_(pooled.to(BF))


def _hand_step(eng, p, sch, i, t, mult, x, resid_i, target, mode):
    """one step written out: multiplier, the program by the sampler's rule, slh_ddpm_edit_step in place on x"""
    io = p.io
    eng.set_lora(True, mult)
    io["t"].tensor.fill_(float(t))
    (p.prog if i == 0 or p.prog_text_cached is None else p.prog_text_cached).run(stream())
    chw = x[0].numel()
    f = fp32_coefficients(ddpm_step_coefficients(sch, t, STEPS, 1.0))
    lib.call(lib.OP_DDPM_EDIT, lib.DdpmEditDesc(eps=io["eps"].ptr, x=x.data_ptr(), target=0 if target is None else target.data_ptr(),
                                                 resid=resid_i.data_ptr(), out=x.data_ptr(), out_bf16=io["sample"].ptr,
                                                 out2_bf16=io["sample"].ptr + chw * 2, nb=1, chw=chw, guidance=GS, mode=mode, v_prediction=0, **f), stream())


def test_editor_equals_the_loops_written_out(dev):
    cfg, eng, ed = _editor("tiny_sdxl", "store", dev)
    ctx, pooled, x0 = _inputs(cfg, dev)
    scale, start_noise, seed = 1.5, 500, 3
    sp = ed.invert(ctx, x0, steps=STEPS, skip=SKIP, guidance_scale=GS, seed=seed, pooled=pooled)
    got = ed.edit_latents(sp, scale=scale, start_noise=start_noise)
    torch.cuda.synchronize()
    sch = DDIMSchedule()
    ts = sch.make_timesteps(STEPS)[SKIP:]
    p = eng.plan(2, HW, HW, "on")
    # the inversion
    noise = torch.randn(len(ts), 1, 4, HW, HW, generator=torch.Generator().manual_seed(seed)).to(dev)
    path = torch.stack([float(sch.alphas_cumprod[t].double().sqrt()) * x0 + float((1 - sch.alphas_cumprod[t].double()).sqrt()) * noise[i]
                        for i, t in enumerate(ts)])
    assert torch.equal(path[0], sp.x_start)
    _hand_inputs(eng, p, ctx, pooled)
    x = path[0].clone()
    p.io["sample"].tensor[:1].copy_(x.to(BF))
    p.io["sample"].tensor[1:].copy_(x.to(BF))
    resid = torch.full_like(path, float("nan"))
    for i, t in enumerate(ts):
        _hand_step(eng, p, sch, i, t, 0.0, x, resid[i], path[i + 1] if i + 1 < len(ts) else x0, 0)
    torch.cuda.synchronize()
    assert torch.equal(resid, sp.resid), "the inversion's residuals"
    assert torch.equal(x, sp.recon)
    # the edit
    x = path[0].clone()
    p.io["sample"].tensor[:1].copy_(x.to(BF))
    p.io["sample"].tensor[1:].copy_(x.to(BF))
    mults = []
    for i, t in enumerate(ts):
        mults.append(0.0 if t > start_noise else scale)
        _hand_step(eng, p, sch, i, t, mults[-1], x, resid[i], None, 1)
    eng.set_lora(False)
    torch.cuda.synchronize()
    assert 0.0 in mults and scale in mults, "the test must exercise both sides of start_noise"
    assert torch.equal(got, x), "SliderEditor.edit_latents and the hand-written loop differ"


def test_saved_inversion_edits_to_the_same_bits(dev, tmp_path):
    cfg, eng, ed = _editor("tiny_sd1", "store", dev)
    ctx, pooled, x0 = _inputs(cfg, dev)
    sp = ed.invert(ctx, x0, steps=STEPS, skip=SKIP, guidance_scale=GS, seed=4)
    path = str(tmp_path / "space.pt")
    sp.save(path)
    back = NoiseSpace.load(path, dev)
    assert back.resid.is_cuda and torch.equal(back.resid, sp.resid) and torch.equal(back.ctx, ctx)
    for s in (0.0, 1.5):
        assert torch.equal(ed.edit_latents(back, scale=s, start_noise=500), ed.edit_latents(sp, scale=s, start_noise=500)), s
    assert torch.equal(ed.edit_latents(back), sp.recon)


# ---------------------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------------------
def _pixels(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_cli_on_synthetic_weights(dev, tmp_path, monkeypatch):
    from PIL import Image
    cfg = CONFIGS["sd1"]()
    img = str(tmp_path / "photo.png")
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (256, 256, 3), dtype=np.uint8)).save(img)
    slider, other = str(tmp_path / "age_alpha1.0_rank4_noxattn.pt"), str(tmp_path / "smile_alpha4.0_rank8_full.pt")
    torch.save(drawn_slider(cfg, "noxattn", 4, 1.0, 41), slider)
    torch.save(drawn_slider(cfg, "full", 8, 4.0, 42), other)
    common = ["--model", "sd1", "--synthetic", "--lora_weight", slider, "--steps", "4", "--skip", "1", "--res", "256"]
    inv = str(tmp_path / "inversion.pt")
    out = edit.main(common + ["--image", img, "--scales=-1,0,1", "--save_inversion", inv, "--out", str(tmp_path / "first")])
    files = {n: os.path.join(out, n) for n in ("recon.png", "scale_-1.png", "scale_0.png", "scale_1.png")}
    assert all(os.path.getsize(f) > 0 for f in files.values()) and os.path.getsize(inv) > 0
    assert _pixels(files["recon.png"]).shape == (256, 256, 3)
    assert np.array_equal(_pixels(files["scale_0.png"]), _pixels(files["recon.png"])), "scale 0 is the reconstruction"
    assert not np.array_equal(_pixels(files["scale_-1.png"]), _pixels(files["scale_1.png"]))
    # a second run edits the saved inversion: no image, the same bytes
    out2 = edit.main(common + ["--inversion", inv, "--scales=1", "--out", str(tmp_path / "second")])
    assert open(os.path.join(out2, "scale_1.png"), "rb").read() == open(files["scale_1.png"], "rb").read()
    # composed with a rank-8 slider held at 0.5: the merged-weights path; it runs and leaves the weights as they were
    seen = []

    class Spy(SliderEditor):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen.append((self, {n: self.eng.w.t[n].clone() for n in self.merger.touched}))
    monkeypatch.setattr(edit, "SliderEditor", Spy)
    out3 = edit.main(common + ["--image", img, "--scales=0,1", "--compose", other + ":0.5", "--out", str(tmp_path / "third")])
    ed, snap = seen[0]
    assert len(seen) == 1 and len(snap) > 0 and not ed.merger.merged and all(torch.equal(ed.eng.w.t[n], v) for n, v in snap.items())
    assert np.array_equal(_pixels(os.path.join(out3, "scale_0.png")), _pixels(os.path.join(out3, "recon.png")))
    assert not np.array_equal(_pixels(os.path.join(out3, "scale_1.png")), _pixels(os.path.join(out3, "recon.png")))
