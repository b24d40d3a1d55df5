"""CPU: the second-order noise space of sliders_amd/edit.py (docs/EDIT.md, "Second-order noise space") - the coefficients against
SDE-DPM-Solver++ written out here, the reconstruction identity at order 2, the derived bound and three mutants it rejects, the order
of the method on an analytic denoiser, slh_edit_step2's refusals, the saved NoiseSpace and the command line."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from sliders_amd import edit, lib
from sliders_amd.ddim import DDIMSchedule
from sliders_amd.edit import (NoiseSpace, build_path, chain_coefficients, ddpm_mu2_reference, ddpm_step2_coefficients, ddpm_step_coefficients,
                              edit_reference, edit_timesteps, invert_reference, trajectory_reference)
from tests.edit_order2_ref import mu_oracle_and_bound, worst_ratio
from tests.test_edit_host import CONFIGS, recon_bound, toy_predict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "slh_edit_step2"
GRIDS = [(steps, skip) for steps in (10, 20, 50) for skip in (0, None)]


def _levels(sch, t):
    """alpha, sigma, lambda of a timestep (t < 0: the end of the grid, alpha_bar = 1), float64"""
    a = float(sch.alphas_cumprod[t]) if t >= 0 else float(sch.final_alpha_cumprod)
    al, si = math.sqrt(a), math.sqrt(1.0 - a)
    return al, si, (math.log(al / si) if si > 0 else math.inf)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. coefficients
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [10, 20, 50])
def test_first_order_coefficients_are_sde_dpm_solver_pp_at_eta_one(steps):
    sch = DDIMSchedule()
    worst = 0.0
    for t in sch.make_timesteps(steps)[:-1]:
        c = ddpm_step_coefficients(sch, t, steps, 1.0)
        (al_t, si_t, la_t), (al_p, si_p, la_p) = _levels(sch, t), _levels(sch, t - 1000 // steps)
        h = la_p - la_t
        B = c["c_sqrt_alpha_prev"] - c["c_dir"] * c["c_sqrt_alpha_t"] / c["c_sqrt_beta_t"]
        diffs = (c["c_dir"] / c["c_sqrt_beta_t"] - si_p / si_t * math.exp(-h), B - al_p * (1.0 - math.exp(-2.0 * h)),
                 c["sigma"] - si_p * math.sqrt(1.0 - math.exp(-2.0 * h)))
        worst = max(worst, *(abs(d) for d in diffs))
    print(f"[order2] steps {steps}: first-order coefficients against the SDE-DPM-Solver++ forms, worst |difference| {worst:.1e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("steps,skip", GRIDS)
def test_mu2_is_the_second_order_midpoint_sde_update_in_float64(steps, skip):
    """mu_2 from this module's float64 scalars against diffusers' sde-dpmsolver++ (solver_order 2, midpoint) written out from
    alpha, sigma and lambda: (s_p / s_t) e^-h x + a_p (1 - e^-2h) D0 + 1/2 a_p (1 - e^-2h) (D0 - D1) h / h_old"""
    sch = DDIMSchedule()
    ts = edit_timesteps(sch, steps, skip)
    g = torch.Generator().manual_seed(steps)
    worst = 0.0
    for i, t in enumerate(ts):
        c = chain_coefficients(sch, ts, i, steps, 1.0, order=2)
        assert ("c_corr" in c) == (0 < i < len(ts) - 1), "no correction on the first and on the last step of the grid"
        assert {k: v for k, v in c.items() if k != "c_corr"} == ddpm_step_coefficients(sch, t, steps, 1.0)
        if "c_corr" not in c:
            continue
        x, e, D1 = (torch.randn(64, generator=g, dtype=torch.float64) for _ in range(3))
        D0 = (x - c["c_sqrt_beta_t"] * e) * c["c_inv_sqrt_alpha_t"]
        mu2 = c["c_sqrt_alpha_prev"] * D0 + c["c_dir"] * e + c["c_corr"] * (D0 - D1)
        (al_t, si_t, la_t), (al_p, si_p, la_p), (_, _, la_o) = _levels(sch, t), _levels(sch, t - 1000 // steps), _levels(sch, ts[i - 1])
        h, h_old = la_p - la_t, la_t - la_o
        D0w = (x - si_t * e) / al_t
        want = si_p / si_t * math.exp(-h) * x + al_p * (1.0 - math.exp(-2.0 * h)) * D0w + 0.5 * al_p * (1.0 - math.exp(-2.0 * h)) * (D0w - D1) * h / h_old
        scale = x.abs() + e.abs() + D0w.abs() + D1.abs()
        worst = max(worst, float(((mu2 - want).abs() / scale).max()))
    print(f"[order2] steps {steps} skip {skip}: mu_2 against the midpoint SDE update, worst relative difference {worst:.1e}")
    assert worst <= 1e-12


def test_step2_coefficients_arguments():
    sch = DDIMSchedule()
    assert "c_corr" not in ddpm_step2_coefficients(sch, 500, 50, 1.0) and "c_corr" not in ddpm_step2_coefficients(sch, 0, 50, 1.0, 20)
    c = ddpm_step2_coefficients(sch, 500, 50, 1.0, 520)
    assert c["c_corr"] > 0.0 and set(edit.fp32_coefficients(c)) == set(edit.COEFFICIENTS) | {"c_corr"}
    assert set(edit.fp32_coefficients(ddpm_step_coefficients(sch, 500, 50, 1.0))) == set(edit.COEFFICIENTS)
    with pytest.raises(ValueError, match="t_older"):
        ddpm_step2_coefficients(sch, 500, 50, 1.0, 480)
    for bad in (0, 3, "2"):
        with pytest.raises(ValueError, match="order"):
            invert_reference(toy_predict(), torch.zeros(1, 4, 4, 4), sch, 4, 0, order=bad)
    x = torch.zeros(4)
    with pytest.raises(ValueError, match="go together"):
        ddpm_mu2_reference(x.bfloat16(), x.bfloat16(), x, c, 7.5)
    with pytest.raises(ValueError, match="go together"):
        ddpm_mu2_reference(x.bfloat16(), x.bfloat16(), x, ddpm_step_coefficients(sch, 500, 50, 1.0), 7.5, x0_prev=x)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the identity
# ---------------------------------------------------------------------------------------------------------------------------------
def mutant_invert2(predict, x0, sch, steps, skip, eta, guidance, seed):
    """the order-2 inversion that walks on from `target`, not from mu + d"""
    ts = edit_timesteps(sch, steps, skip)
    path = build_path(sch, x0, ts, seed)
    x, resid, hist = path[0].clone(), torch.empty_like(path), None
    for i, t in enumerate(ts):
        eu, et = predict(x.to(torch.bfloat16), t, 0.0)
        coef = chain_coefficients(sch, ts, i, steps, eta, 2)
        mu, hist = ddpm_mu2_reference(eu, et, x, coef, guidance, False, torch.float32, hist if "c_corr" in coef else None)
        target = path[i + 1] if i + 1 < len(ts) else x0
        resid[i] = target - mu
        x = target
    return NoiseSpace(x0=x0, x_start=path[0].clone(), resid=resid, recon=x, timesteps=list(ts), steps=steps, skip=skip, eta=eta,
                      guidance=guidance, prediction_type="epsilon", seed=seed, order=2)


def test_scale_zero_reproduces_the_order2_inversion_bit_for_bit():
    sch = DDIMSchedule()
    predict = toy_predict()
    worst, broken = 0.0, 0
    for n, (shape, (steps, skip), eta) in enumerate(CONFIGS):
        x0 = torch.randn(shape, generator=torch.Generator().manual_seed(100 + n))
        sp = invert_reference(predict, x0, sch, steps, skip, eta, guidance=7.5, seed=n, order=2)
        tag = f"{shape} steps {steps} skip {skip} eta {eta}"
        assert sp.order == 2 and sp.resid.shape == (steps - skip,) + shape and sp.resid.dtype == torch.float32
        assert torch.equal(edit_reference(predict, sp, sch, scale=0.0), sp.recon), tag
        one = invert_reference(predict, x0, sch, steps, skip, eta, guidance=7.5, seed=n)
        assert one.order == 1 and torch.equal(one.resid[0], sp.resid[0]) and not torch.equal(one.resid[1], sp.resid[1]), f"{tag}: the first step is first order"
        assert not torch.equal(edit_reference(predict, sp, sch, scale=0.0, order=1), sp.recon), f"{tag}: the order belongs to the space"
        err, bound = (sp.recon.double() - x0.double()).abs(), recon_bound(sp)
        assert bool((err <= bound).all()), f"{tag}: {int((err > bound).sum())} elements beyond the bound"
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        out = edit_reference(predict, sp, sch, scale=2.0)
        assert bool(torch.isfinite(out).all()) and not torch.equal(out, sp.recon), tag
        # a masked edit: the reconstruction outside the mask; a space without visited gets it from the replay
        half = torch.zeros(shape[2], shape[3])
        half[:, shape[3] // 2:] = 1.0
        masked = edit_reference(predict, sp, sch, scale=2.0, mask=half)
        keep = half.expand(shape) == 0
        assert torch.equal(masked[keep], sp.recon[keep]) and not torch.equal(masked, sp.recon), tag
        bare = NoiseSpace(**{**sp._map(lambda t: t), "visited": None})
        assert torch.equal(trajectory_reference(predict, bare, sch).visited, sp.visited), tag
        mu = mutant_invert2(predict, x0, sch, steps, skip, eta, 7.5, n)
        assert torch.equal(mu.recon, x0)
        broken += not torch.equal(edit_reference(predict, mu, sch, scale=0.0), mu.recon)
    print(f"[order2] worst |recon - x0| / bound = {worst:.3f} over {len(CONFIGS)} configurations; the mutant breaks {broken} of them")
    assert broken == len(CONFIGS), "walking on from `target` breaks the bit equality in every configuration"


def test_order2_identity_with_v_prediction_and_in_float64():
    sch = DDIMSchedule(prediction_type="v_prediction")
    predict = toy_predict(1)
    x0 = torch.randn(2, 4, 5, 7, generator=torch.Generator().manual_seed(7))
    for dtype in (torch.float32, torch.float64):
        sp = invert_reference(predict, x0, sch, 10, 2, 1.0, guidance=5.0, seed=3, dtype=dtype, order=2)
        assert sp.resid.dtype == dtype and torch.equal(edit_reference(predict, sp, sch, scale=0.0, dtype=dtype), sp.recon)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the bound admits the arithmetic and rejects mutants
# ---------------------------------------------------------------------------------------------------------------------------------
def _chain_steps(v, eta, steps=10, skip=2, seed=0):
    """the second-order steps of a float64 order-2 inversion over the toy network: per step its inputs and the x0h of the two steps
    before it"""
    sch = DDIMSchedule(prediction_type="v_prediction" if v else "epsilon")
    predict = toy_predict(seed)
    ts = edit_timesteps(sch, steps, skip)
    x0 = torch.randn(2, 4, 5, 7, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    path = build_path(sch, x0, ts, seed)
    x, hist, out = path[0].clone(), [], []
    for i, t in enumerate(ts):
        eu, et = predict(x.to(torch.bfloat16), t, 0.0)
        coef = chain_coefficients(sch, ts, i, steps, eta, 2)
        second = "c_corr" in coef
        if second and i >= 2:
            out.append(dict(sch=sch, ts=ts, i=i, steps=steps, eta=eta, eu=eu, et=et, x=x.float(), coef=coef, prev=hist[-1].float(), older=hist[-2].float()))
        mu, x0h = ddpm_mu2_reference(eu, et, x, coef, 7.5, v, torch.float64, hist[-1] if second else None)
        hist.append(x0h)
        x = path[i + 1] if i + 1 < len(ts) else x0          # (any latent will do as the next step's input)
    return out


def _swapped(s):
    """c_corr with h_old / h in place of h / h_old"""
    la = lambda t: _levels(s["sch"], t)[2]
    t, older, prev = s["ts"][s["i"]], s["ts"][s["i"] - 1], s["ts"][s["i"]] - 1000 // s["steps"]
    h, h_old = la(prev) - la(t), la(t) - la(older)
    return dict(s["coef"], c_corr=s["coef"]["c_corr"] * (h_old / h) ** 2)


def test_fp32_restatement_within_the_bound_and_three_mutants_outside():
    worst, mutants = 0.0, {"dropped": math.inf, "swapped": math.inf, "wrong_step": math.inf}
    for v in (False, True):
        for eta in (0.0, 1.0):
            for s in _chain_steps(v, eta):
                first = {k: s["coef"][k] for k in s["coef"] if k != "c_corr"}
                mu, x0, b_mu, b_x0, n, _ = mu_oracle_and_bound(s["eu"], s["et"], s["x"], s["coef"], 7.5, v, s["prev"])
                assert n == 11
                got, got_x0 = ddpm_mu2_reference(s["eu"], s["et"], s["x"], s["coef"], 7.5, v, torch.float32, s["prev"])
                assert got.dtype == torch.float32
                worst = max(worst, worst_ratio(got, mu, b_mu), worst_ratio(got_x0, x0, b_x0))
                wrong = {"dropped": ddpm_mu2_reference(s["eu"], s["et"], s["x"], first, 7.5, v, torch.float32)[0],
                         "swapped": ddpm_mu2_reference(s["eu"], s["et"], s["x"], _swapped(s), 7.5, v, torch.float32, s["prev"])[0],
                         "wrong_step": ddpm_mu2_reference(s["eu"], s["et"], s["x"], s["coef"], 7.5, v, torch.float32, s["older"])[0]}
                for name, m in wrong.items():
                    mutants[name] = min(mutants[name], worst_ratio(m, mu, b_mu))
    print(f"[order2] fp32 restatement: worst error / bound {worst:.3f}; mutants at least " + ", ".join(f"{k} {r:.1e}" for k, r in mutants.items()))
    assert worst <= 1.0
    assert all(r > 100.0 for r in mutants.values()), mutants


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the order of the method
# ---------------------------------------------------------------------------------------------------------------------------------
def flow_error(steps, skip, s2, order):
    """|chain - exact| for x = 1 at the grid's first point: eta 0, residuals 0, data N(0, s2), the exact denoiser, float64 scalars,
    stopped before the final step"""
    sch = DDIMSchedule()
    ts = edit_timesteps(sch, steps, skip)
    x, hist = 1.0, None
    for i, t in enumerate(ts[:-1]):
        c = chain_coefficients(sch, ts, i, steps, 0.0, order)
        al, si, _ = _levels(sch, t)
        x0h = al * s2 * x / (al * al * s2 + si * si)
        mu = c["c_sqrt_alpha_prev"] * x0h + c["c_dir"] * (x - al * x0h) / si
        if "c_corr" in c:
            mu += c["c_corr"] * (x0h - hist)
        x, hist = mu, x0h
    a0, a1 = float(sch.alphas_cumprod[ts[0]]), float(sch.alphas_cumprod[ts[-1]])
    return abs(x - math.sqrt((a1 * s2 + 1.0 - a1) / (a0 * s2 + 1.0 - a0)))


@pytest.mark.parametrize("skip", [0, None], ids=["skip0", "default_skip"])
@pytest.mark.parametrize("s2", [0.25, 1.0, 4.0])
def test_order_of_the_method(s2, skip):
    e = {(o, n): flow_error(n, skip, s2, o) for o in (1, 2) for n in (20, 100, 200)}
    r1, r2 = e[1, 100] / e[1, 200], e[2, 100] / e[2, 200]
    print(f"[order2] s2 {s2} skip {skip}: err(100)/err(200) order 1 {r1:.2f}, order 2 {r2:.2f}; order 2 / order 1 at 20 steps {e[2, 20] / e[1, 20]:.2f}, "
          f"100 {e[2, 100] / e[1, 100]:.3f}, 200 {e[2, 200] / e[1, 200]:.3f}; errors " + " ".join(f"{o}@{n}={v:.2e}" for (o, n), v in sorted(e.items())))
    assert 1.8 <= r1 <= 2.1 and r2 >= 2.7
    assert e[2, 100] < e[1, 100] and e[2, 200] < e[1, 200]


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def _call(ptrs, dims, coef):
    return lib.load().slh_edit_step2((C.c_void_p * 12)(*ptrs) if ptrs is not None else None, (C.c_int32 * 5)(*dims) if dims is not None else None,
                                     (C.c_float * 7)(*coef) if coef is not None else None, None)


def test_abi_declared_exported_and_refusing_on_the_host():
    hdr = open(os.path.join(ROOT, "include", "sliders_hip.h")).read()
    assert re.search(rf"^int {NAME}\(const void\* const\* ptrs, const int32_t\* dims, const float\* coef, slh_stream_t stream\);", hdr, flags=re.M)
    assert NAME in lib.EXPORTS and hasattr(lib.load(), NAME)
    assert lib.load().slh_op_info(-1, None, None, None) == 41 == len(lib._ENTRY), "no new opcode"
    # eps eps_text x x0_prev target resid keep mask out x0_out out_bf16 out2_bf16; addresses that are never dereferenced
    ok = [0x10000 * (k + 1) for k in range(12)]
    EPS, TEXT, X, PREV, TARGET, RESID, KEEP, MASK, OUT, X0OUT, B1, B2 = range(12)
    dims, coef = [1, 64, 16, 1, 0], [7.5, 0.5, 1.2, 0.8, 0.9, 0.3, 0.25]          # nb chw hw mode v; n = 64: 256 bytes fp32, 128 bf16
    invert = [0 if k in (KEEP, MASK) else v for k, v in enumerate(ok)]

    def refused(what, p=ok, d=dims, c=coef):
        assert _call(p, d, c) == -1, f"{what}: refused by a check, before any launch"
        msg = lib.last_error()
        assert NAME in msg and what in msg, (what, msg)
    without = lambda *holes, p=ok: [0 if k in holes else v for k, v in enumerate(p)]
    moved = lambda k, to, p=ok: [to if j == k else v for j, v in enumerate(p)]
    refused("null", None)
    refused("null", d=None)
    refused("null", c=None)
    for hole in (EPS, X, RESID, OUT):
        refused("null", without(hole))
    for k in (X, PREV, RESID, KEEP, MASK, OUT, X0OUT):
        refused("not 4-byte aligned", moved(k, ok[k] + 2))
    refused("not 4-byte aligned", moved(TARGET, ok[TARGET] + 2, p=invert), d=[1, 64, 16, 0, 0])          # (mode 1 does not read target)
    for k in (EPS, TEXT, B1, B2):
        refused("not 2-byte aligned", moved(k, ok[k] + 1))
    for k, name in enumerate(("nb", "chw", "hw")):
        for bad in (0, -1):
            refused(f"{name} = {bad}", d=[bad if j == k else v for j, v in enumerate(dims)])
    refused("not a multiple of hw", d=[1, 64, 24, 1, 0])
    for bad in (2, -1):
        refused(f"mode {bad}", d=[1, 64, 16, bad, 0])
        refused(f"v_prediction = {bad}", d=[1, 64, 16, 1, bad])
    refused("keep and mask go together", without(KEEP))
    refused("keep and mask go together", without(MASK))
    refused("needs target", without(TARGET, p=invert), d=[1, 64, 16, 0, 0])
    refused("takes no mask", d=[1, 64, 16, 0, 0])
    for bad in (0.0, float("inf"), float("-inf"), float("nan")):
        refused("c_corr", c=coef[:6] + [bad])
    # outputs against inputs: only out == x and x0_out == x0_prev, as the same address
    n4, n2 = 64 * 4, 64 * 2
    refused("out overlaps x", moved(OUT, ok[X] + 16))
    refused("x0_out overlaps x0_prev", moved(X0OUT, ok[PREV] + n4 - 4))
    refused("out overlaps x0_prev", moved(OUT, ok[PREV]))
    refused("x0_out overlaps x", moved(X0OUT, ok[X]))
    refused("out overlaps eps", moved(OUT, ok[EPS] + n2, p=without(TEXT)))          # without eps_text the pair is 2 n bf16 values
    refused("out overlaps eps_text", moved(OUT, ok[TEXT] + n2 - 4))
    refused("out overlaps resid", moved(OUT, ok[RESID]))
    refused("out overlaps keep", moved(OUT, ok[KEEP] + 4))
    refused("out overlaps mask", moved(OUT, ok[MASK] + 16 * 4 - 4))
    refused("x0_out overlaps keep", moved(X0OUT, ok[KEEP]))
    refused("out_bf16 overlaps mask", moved(B1, ok[MASK]))
    refused("out2_bf16 overlaps keep", moved(B2, ok[KEEP] + n4 - 2))
    refused("out_bf16 overlaps x", moved(B1, ok[X]))
    refused("resid overlaps target", moved(RESID, ok[TARGET] + 4, p=invert), d=[1, 64, 16, 0, 0])
    refused("resid overlaps x", moved(RESID, ok[X], p=invert), d=[1, 64, 16, 0, 0])
    refused("out overlaps target", moved(OUT, ok[TARGET], p=invert), d=[1, 64, 16, 0, 0])
    refused("out overlaps x0_out", moved(X0OUT, ok[OUT] + 4))
    refused("out_bf16 overlaps out2_bf16", moved(B2, ok[B1] + n2 - 2))
    # the binding raises with the library's message
    with pytest.raises(lib.SlidersHipError, match=f"{NAME}.*mode 2"):
        lib.edit_step2(0, eps=0x1000, x=0x2000, resid=0x3000, out=0x4000, nb=1, chw=64, hw=16, mode=2, guidance=7.5, c_sqrt_beta_t=0.5,
                       c_inv_sqrt_alpha_t=1.2, c_sqrt_alpha_t=0.8, c_sqrt_alpha_prev=0.9, c_dir=0.3)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. NoiseSpace and the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def test_noise_space_keeps_its_order(tmp_path):
    x0 = torch.randn(1, 4, 6, 6, generator=torch.Generator().manual_seed(1))
    sp = invert_reference(toy_predict(), x0, DDIMSchedule(), 10, 3, 0.5, guidance=4.0, seed=11, order=2)
    path = str(tmp_path / "space.pt")
    sp.save(path)
    back = NoiseSpace.load(path)
    assert back.order == 2 and type(back.order) is int and back.to("cpu").order == 2
    assert torch.equal(edit_reference(toy_predict(), back, DDIMSchedule(), scale=0.0), sp.recon)
    saved = torch.load(path, map_location="cpu")
    assert saved["order"] == 2
    # a file from before the second-order space: first order
    one = invert_reference(toy_predict(), x0, DDIMSchedule(), 10, 3, 0.5, guidance=4.0, seed=11)
    one.save(path)
    old = torch.load(path, map_location="cpu")
    del old["order"]
    torch.save(old, path)
    back = NoiseSpace.load(path)
    assert back.order == 1 and torch.equal(edit_reference(toy_predict(), back, DDIMSchedule(), scale=0.0), one.recon)
    for gone in ("resid", "eta", "x_start"):
        torch.save({k: v for k, v in old.items() if k != gone}, path)
        with pytest.raises(KeyError, match=gone):
            NoiseSpace.load(path)
    torch.save(dict(old, order=3), path)
    with pytest.raises(ValueError, match="order"):
        NoiseSpace.load(path)


@pytest.mark.parametrize("argv", [
    ["--load_inversion", "a.pt", "--order", "2"],
    ["--inversion", "a.pt", "--order", "1"],
    ["--image", "x.png", "--order", "3"],
    ["--image", "x.png", "--order", "0"],
])
def test_cli_order_argument_errors(monkeypatch, argv):
    def boom(*a, **k):
        raise AssertionError("an argument error must not reach CUDA or a model")
    monkeypatch.setattr(torch.cuda, "_lazy_init", boom)
    import sliders_amd.model_util as mu
    monkeypatch.setattr(mu, "synthetic_engine", boom)
    monkeypatch.setattr(mu, "load_unet_engine", boom)
    with pytest.raises(SystemExit) as e:
        edit.main(["--model", "sd1", "--synthetic"] + argv)
    assert e.value.code not in (0, None)


def test_cli_order_parses():
    P = lambda *argv: edit.build_parser().parse_args(list(argv))
    assert P("--image", "x.png").order is None and P("--image", "x.png", "--order", "2").order == 2
    assert P("--load_inversion", "a.pt").inversion == "a.pt" == P("--inversion", "a.pt").inversion
    with pytest.raises(SystemExit, match="--order"):
        edit.check_args(P("--synthetic", "--load_inversion", "a.pt", "--order", "2"))
    assert edit.check_args(P("--synthetic", "--image", "x.png", "--order", "2", "--scales=0,1")) == [0.0, 1.0]
