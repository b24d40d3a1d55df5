"""CPU: the residual DDPM noise space of sliders_amd/edit.py - the step coefficients against formulas written out here, the
reconstruction identity over a toy network (and a mutant that shows the test can see the bug the residual form avoids), the saved
NoiseSpace, slh_ddpm_edit_step's descriptor checks, the CLI's argument errors.  docs/EDIT.md derives the bounds."""
import ctypes
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sliders_amd import edit, lib
from sliders_amd.ddim import DDIMSchedule
from sliders_amd.edit import NoiseSpace, build_path, ddpm_mu_reference, ddpm_step_coefficients, edit_reference, invert_reference

GRIDS = [(50, 18), (10, 2), (4, 0)]
ETAS = [0.0, 0.5, 1.0]
SHAPES = [(1, 4, 16, 16), (2, 4, 5, 7)]


# ---------------------------------------------------------------------------------------------------------------------------------
# coefficients
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [50, 10, 4])
@pytest.mark.parametrize("eta", ETAS)
def test_coefficients_match_the_formulas_in_float64(steps, eta):
    sch = DDIMSchedule()
    ac = sch.alphas_cumprod.double().numpy()
    grid = sch.make_timesteps(steps)
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-300)
    for t in grid:
        prev = t - 1000 // steps
        at, ap = ac[t], (ac[prev] if prev >= 0 else 1.0)
        var = (1.0 - ap) / (1.0 - at) * (1.0 - at / ap)             # the DDPM variance of the step, as diffusers writes it
        sigma = eta * np.sqrt(max(var, 0.0))
        want = dict(sigma=sigma, c_dir=np.sqrt(max(0.0, 1.0 - ap - sigma ** 2)), c_sqrt_alpha_prev=np.sqrt(ap),
                    c_sqrt_beta_t=np.sqrt(1.0 - at), c_inv_sqrt_alpha_t=at ** -0.5, c_sqrt_alpha_t=np.sqrt(at))
        got = ddpm_step_coefficients(sch, t, steps, eta)
        assert set(got) == set(want)
        for k in want:
            assert rel(got[k], want[k]) <= 1e-12 or (want[k] == 0.0 and got[k] == 0.0), (t, k, got[k], want[k])
        assert abs(got["sigma"] ** 2 + got["c_dir"] ** 2 - (1.0 - ap)) <= 1e-12, t
        if eta == 0.0:
            cb, cia, cp, cd = sch.step_coefficients(t, steps)         # computed in fp32
            for k, v in (("c_sqrt_beta_t", cb), ("c_inv_sqrt_alpha_t", cia), ("c_sqrt_alpha_prev", cp), ("c_dir", cd)):
                assert rel(got[k], v) <= 1e-6 or (v == 0.0 and got[k] == 0.0), (t, k, got[k], v)
    last = ddpm_step_coefficients(sch, grid[-1], steps, eta)
    assert grid[-1] == 0 and last["sigma"] == 0.0 and last["c_dir"] == 0.0 and last["c_sqrt_alpha_prev"] == 1.0
    f32 = edit.fp32_coefficients(last)
    assert set(f32) == set(edit.COEFFICIENTS) and all(np.float32(v) == v for v in f32.values())


def test_coefficients_refuse_eta_outside_the_unit_interval():
    for eta in (-0.01, 1.01):
        with pytest.raises(ValueError):
            ddpm_step_coefficients(DDIMSchedule(), 500, 50, eta)
    with pytest.raises(ValueError):
        edit.edit_timesteps(DDIMSchedule(), 10, 10)
    assert edit.default_skip(100) == 36 and edit.default_skip(50) == 18
    assert edit.edit_timesteps(DDIMSchedule(), 50) == DDIMSchedule().make_timesteps(50)[18:]


# ---------------------------------------------------------------------------------------------------------------------------------
# the identity, over a toy network
# ---------------------------------------------------------------------------------------------------------------------------------
def toy_predict(seed=0):
    """a fixed random 3 x 3 convolution + tanh per epsilon half, bf16 in and out; the slider adds a term proportional to its multiplier"""
    g = torch.Generator().manual_seed(seed)
    wu, wt, ws = (torch.randn(4, 4, 3, 3, generator=g) * 0.2 for _ in range(3))

    def predict(x_bf16, t, multiplier):
        assert x_bf16.dtype == torch.bfloat16
        x = x_bf16.float()
        eu = torch.tanh(F.conv2d(x, wu, padding=1) + t / 1000.0)
        et = torch.tanh(F.conv2d(x, wt, padding=1) + float(multiplier) * F.conv2d(x, ws, padding=1))
        return eu.to(torch.bfloat16), et.to(torch.bfloat16)
    return predict


def recon_bound(space):
    """recon = fl(mu + fl(x0 - mu)) with d = fl(x0 - mu) the last residual: |d - (x0 - mu)| <= u |d|, so |mu + d| <= |x0| + u |d| and
    |recon - x0| <= u |d| + u (|x0| + u |d|) <= 2^-22 (2 |x0| + |d_last|) with room to spare (u = 2^-24)"""
    return 2.0 ** -22 * (2.0 * space.x0.double().abs() + space.resid[-1].double().abs())


def mutant_invert(predict, x0, sch, steps, skip, eta, guidance, seed):
    """the inversion with the bug the residual form exists to avoid: the chain continues from `target`, not from mu + d"""
    ts = edit.edit_timesteps(sch, steps, skip)
    path = build_path(sch, x0, ts, seed)
    x, resid = path[0].clone(), torch.empty_like(path)
    for i, t in enumerate(ts):
        eu, et = predict(x.to(torch.bfloat16), t, 0.0)
        mu = ddpm_mu_reference(eu, et, x, ddpm_step_coefficients(sch, t, steps, eta), guidance, False, torch.float32)
        target = path[i + 1] if i + 1 < len(ts) else x0
        resid[i] = target - mu
        x = target
    return NoiseSpace(x0=x0, x_start=path[0].clone(), resid=resid, recon=x, timesteps=list(ts), steps=steps, skip=skip, eta=eta,
                      guidance=guidance, prediction_type="epsilon", seed=seed)


CONFIGS = list(itertools.product(SHAPES, GRIDS, ETAS))


def test_scale_zero_reproduces_the_inversion_bit_for_bit():
    sch = DDIMSchedule()
    predict = toy_predict()
    mutant_broken, worst = 0, 0.0
    for n, (shape, (steps, skip), eta) in enumerate(CONFIGS):
        x0 = torch.randn(shape, generator=torch.Generator().manual_seed(100 + n))
        sp = invert_reference(predict, x0, sch, steps, skip, eta, guidance=7.5, seed=n)
        tag = f"{shape} steps {steps} skip {skip} eta {eta}"
        assert sp.timesteps == sch.make_timesteps(steps)[skip:] and sp.resid.shape == (steps - skip,) + shape and sp.resid.dtype == torch.float32
        assert torch.equal(edit_reference(predict, sp, sch, scale=0.0), sp.recon), tag
        err, bound = (sp.recon.double() - x0.double()).abs(), recon_bound(sp)
        assert bool((err <= bound).all()), f"{tag}: {int((err > bound).sum())} elements beyond the bound"
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        for s in (2.0, -2.0):
            out = edit_reference(predict, sp, sch, scale=s)
            assert bool(torch.isfinite(out).all()) and not torch.equal(out, sp.recon), f"{tag} scale {s}"
        assert torch.equal(edit_reference(predict, sp, sch, scale=2.0, start_noise=-1), sp.recon), f"{tag}: the slider never switches on"
        mu = mutant_invert(predict, x0, sch, steps, skip, eta, 7.5, n)
        assert torch.equal(mu.recon, x0)
        mutant_broken += not torch.equal(edit_reference(predict, mu, sch, scale=0.0), mu.recon)
    print(f"[edit] worst |recon - x0| / bound = {worst:.3f} over {len(CONFIGS)} configurations; the mutant breaks {mutant_broken} of them")
    assert mutant_broken >= 1, "feeding `target` back must break the bit equality somewhere, or this test cannot see that bug"


def test_v_prediction_and_the_float64_oracle():
    """the same identity with v prediction; and the fp32 recurrence stays near the float64 one over the same residuals"""
    sch = DDIMSchedule(prediction_type="v_prediction")
    predict = toy_predict(1)
    x0 = torch.randn(2, 4, 5, 7, generator=torch.Generator().manual_seed(7))
    sp = invert_reference(predict, x0, sch, 10, 2, 1.0, guidance=5.0, seed=3)
    assert sp.prediction_type == "v_prediction"
    assert torch.equal(edit_reference(predict, sp, sch, scale=0.0), sp.recon)
    assert bool(((sp.recon.double() - x0.double()).abs() <= recon_bound(sp)).all())
    sp64 = invert_reference(predict, x0, sch, 10, 2, 1.0, guidance=5.0, seed=3, dtype=torch.float64)
    assert sp64.resid.dtype == torch.float64 and torch.equal(edit_reference(predict, sp64, sch, scale=0.0, dtype=torch.float64), sp64.recon)
    assert float((sp64.recon - x0.double()).abs().max()) <= 2.0 ** -50 * float(2 * x0.abs().max() + sp64.resid[-1].abs().max())


def test_mu_reference_fp32_is_the_float64_one_within_eight_roundings():
    g = torch.Generator().manual_seed(5)
    eu, et = (torch.randn(3, 900, generator=g).to(torch.bfloat16) for _ in range(2))
    x = torch.randn(3, 900, generator=g)
    for v in (False, True):
        c = ddpm_step_coefficients(DDIMSchedule(), 500, 50, 1.0)
        m32, m64 = ddpm_mu_reference(eu, et, x, c, 7.5, v, torch.float32), ddpm_mu_reference(eu, et, x, c, 7.5, v, torch.float64)
        assert m32.dtype == torch.float32 and m64.dtype == torch.float64
        f = edit.fp32_coefficients(c)
        E = eu.double().abs() + 7.5 * (et.double().abs() + eu.double().abs())
        ax = x.double().abs()
        if v:
            S = f["c_sqrt_alpha_prev"] * (f["c_sqrt_alpha_t"] * ax + f["c_sqrt_beta_t"] * E) + f["c_dir"] * (f["c_sqrt_alpha_t"] * E + f["c_sqrt_beta_t"] * ax)
        else:
            S = f["c_sqrt_alpha_prev"] * f["c_inv_sqrt_alpha_t"] * (ax + f["c_sqrt_beta_t"] * E) + f["c_dir"] * E
        assert bool(((m32.double() - m64).abs() <= 8 * 2.0 ** -24 * S).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# NoiseSpace on disk
# ---------------------------------------------------------------------------------------------------------------------------------
def test_noise_space_round_trip(tmp_path):
    from dataclasses import fields
    x0 = torch.randn(1, 4, 6, 6, generator=torch.Generator().manual_seed(1))
    sp = invert_reference(toy_predict(), x0, DDIMSchedule(), 10, 3, 0.5, guidance=4.0, seed=11)
    sp.ctx = torch.randn(2, 77, 8).to(torch.bfloat16)
    path = str(tmp_path / "space.pt")
    sp.save(path)
    back = NoiseSpace.load(path)
    for f in fields(NoiseSpace):
        a, b = getattr(sp, f.name), getattr(back, f.name)
        if torch.is_tensor(a):
            assert a.dtype == b.dtype and torch.equal(a, b), f.name
        else:
            assert a == b and type(a) is type(b), f.name
    assert back.timesteps == [600, 500, 400, 300, 200, 100, 0] and (back.steps, back.skip, back.eta, back.guidance, back.seed) == (10, 3, 0.5, 4.0, 11)
    assert back.pooled is None and back.prediction_type == "epsilon"
    assert torch.equal(edit_reference(toy_predict(), back, DDIMSchedule(), scale=0.0), sp.recon)
    torch.save({"x0": x0}, path)
    with pytest.raises(KeyError):
        NoiseSpace.load(path)


# ---------------------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ddpm_edit_step_refuses_bad_descriptors_before_any_launch():
    l = lib.load()
    assert lib.OP_DDPM_EDIT == 39 and lib._ENTRY[lib.OP_DDPM_EDIT] == ("slh_ddpm_edit_step", lib.DdpmEditDesc)
    assert ctypes.sizeof(lib.DdpmEditDesc) == 8 * 8 + 2 * 4 + 6 * 4 + 2 * 4
    P = 0x1000                                      # never dereferenced: every case is refused on the host
    full = dict(eps=P, x=P, target=P, resid=P, out=P, out_bf16=P, out2_bf16=P, nb=1, chw=16, guidance=7.5, c_sqrt_beta_t=0.5,
                c_inv_sqrt_alpha_t=1.2, c_sqrt_alpha_t=0.8, c_sqrt_alpha_prev=0.9, c_dir=0.3)
    bad = {"mode 0 without target": dict(mode=0, target=0), "mode 0 without resid": dict(mode=0, resid=0),
           "mode 1 without resid": dict(mode=1, resid=0), "no eps": dict(mode=1, eps=0), "no x": dict(mode=0, x=0),
           "no out": dict(mode=1, out=0), "mode 2": dict(mode=2), "mode -1": dict(mode=-1)}
    for name, change in bad.items():
        d = lib.DdpmEditDesc(**{**full, **change})
        assert l.slh_ddpm_edit_step(ctypes.byref(d), None) != 0, name
        assert b"slh_ddpm_edit_step" in l.slh_last_error(), (name, l.slh_last_error())
        with pytest.raises(lib.SlidersHipError, match="slh_ddpm_edit_step"):
            lib.call(lib.OP_DDPM_EDIT, d, 0)
    assert l.slh_ddpm_edit_step(None, None) != 0 and b"slh_ddpm_edit_step" in l.slh_last_error()
    # the executor knows the opcode and checks the record's size
    prog = lib.Program()
    prog.add(lib.OP_DDPM_EDIT, lib.DdpmEditDesc(**{**full, "mode": 0, "target": 0}), "ddpm_edit")
    with pytest.raises(lib.SlidersHipError, match="slh_ddpm_edit_step"):
        prog.run(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [
    ["--image", "x.png", "--steps", "10", "--skip", "10"],
    ["--image", "x.png", "--steps", "4", "--skip", "7"],
    ["--image", "x.png", "--skip", "-1"],
    ["--image", "x.png", "--eta", "1.5"],
    ["--image", "x.png", "--eta", "-0.1"],
    ["--inversion", "a.pt", "--save_inversion", "b.pt"],
    ["--image", "x.png", "--inversion", "a.pt", "--save_inversion", "b.pt"],
    [],
    ["--image", "x.png", "--scales", "1,two"],
    ["--image", "x.png", "--compose", "no_scale.pt"],
])
def test_cli_argument_errors_exit_before_any_model_is_built(monkeypatch, argv):
    def boom(*a, **k):
        raise AssertionError("an argument error must not reach CUDA or a model")
    monkeypatch.setattr(torch.cuda, "_lazy_init", boom)
    import sliders_amd.model_util as mu
    monkeypatch.setattr(mu, "synthetic_engine", boom)
    monkeypatch.setattr(mu, "load_unet_engine", boom)
    with pytest.raises(SystemExit) as e:
        edit.main(["--model", "sd1", "--synthetic"] + argv)
    assert e.value.code not in (0, None)


def test_editor_wants_the_ddim_grid():
    with pytest.raises(ValueError, match="DDIM"):
        edit.SliderEditor(None, scheduler="euler")
