"""GPU: the second-order noise space (docs/EDIT.md, "Second-order noise space") - slh_edit_step2 element by element against float64
with the derived bounds (tests/edit_order2_ref.py), its first-order form against slh_ddpm_edit_step / slh_ddpm_edit_blend bit for bit,
SliderEditor at order 2 (reconstruction, trajectory, masks, prompt directions, the old path at order 1) and the command line."""
import itertools
import os

import numpy as np
import pytest
import torch

from sliders_amd import edit, lib
from sliders_amd.config import CONFIGS
from sliders_amd.ddim import DDIMSchedule
from sliders_amd.directions import DirectionSet
from sliders_amd.edit import (NoiseSpace, SliderEditor, build_path, chain_coefficients, ddpm_step2_coefficients, ddpm_step_coefficients,
                              fp32_coefficients, invert_reference)
from sliders_amd.passes import Pass
from sliders_amd.unet import UNetEngine
from tests.edit_order2_ref import U, mu_oracle_and_bound, step_oracle
from tests.test_direction_edit_gpu import _Hand
from tests.test_direction_sampling_gpu import _cond, _directions
from tests.test_edit_gpu import Arena, _editor
from tests.test_fewstep_sampler_gpu import HW, tiny  # noqa: F401  (tiny: the module's fixture)
from tests.util import check_elementwise, stream

pytestmark = pytest.mark.gpu

GUIDANCE = 7.5
BF, F32 = torch.bfloat16, torch.float32
SCH = DDIMSchedule()
C_CORR = ddpm_step2_coefficients(SCH, 500, 50, 1.0, 520)["c_corr"]
SHAPES = [(1, 1), (900, 225), (1024, 256)]          # (chw, hw): one element, the scalar form, the 16-byte form


def _bits(t):
    return t.contiguous().view(torch.int32)


def _per_element(mask, nb, chw, hw):
    return mask.reshape(nb, 1, hw).expand(nb, chw // hw, hw).reshape(nb * chw)


def draw_case(nb, chw, hw, last, hist, cls, seed):
    """the inputs of one launch on the CPU; coef carries c_corr exactly when there is a history (on the last step, where a chain has
    none, the mid-grid step's value: the kernel takes any)"""
    n = nb * chw
    g = torch.Generator().manual_seed(seed)
    big = 1e3 if cls == "large" else 1.0
    eps = torch.randn(2 * n, generator=g).to(BF)
    if cls == "zero_eps":
        eps.zero_()
    x, x0_prev, target, resid, keep = (torch.randn(n, generator=g) * big for _ in range(5))
    pick = torch.randint(0, 4, (nb * hw,), generator=g)
    mask = torch.where(pick == 0, torch.zeros(nb * hw), torch.where(pick == 1, torch.ones(nb * hw), torch.rand(nb * hw, generator=g).clamp(2.0 ** -20, 0.999)))
    coef = ddpm_step_coefficients(SCH, 0 if last else 500, 50, 1.0)
    if hist:
        coef = dict(coef, c_corr=C_CORR)
    return dict(eps=eps, x=x, x0_prev=x0_prev, target=target, resid=resid, keep=keep, mask=mask, coef=coef)


def run_kernel_case(dev, nb, chw, hw, mode, v, last, hist, masked, cls, sep_text=False, alias=False, seed=0):
    n = nb * chw
    c = draw_case(nb, chw, hw, last, hist, cls, seed)
    sizes = {"eps": 4 * n, "eps_text": 2 * n, "x": 4 * n, "x0_prev": 4 * n, "target": 4 * n, "resid": 4 * n, "keep": 4 * n, "mask": 4 * nb * hw,
             "out": 4 * n, "x0_out": 4 * n, "out_bf16": 2 * n, "out2_bf16": 2 * n}
    ar = Arena(dev, sizes)
    for name in ("x", "x0_prev", "target", "keep", "mask"):
        ar.view(name, F32).copy_(c[name])
    if sep_text:          # the text half lives elsewhere; what follows the uncond half is a decoy that must not be read
        ar.view("eps", BF)[:n].copy_(c["eps"][:n])
        ar.view("eps", BF)[n:].fill_(1e4)
        ar.view("eps_text", BF).copy_(c["eps"][n:])
    else:
        ar.view("eps", BF).copy_(c["eps"])
    if mode == 1:
        ar.view("resid", F32).copy_(c["resid"])
    out_name, x0_name = ("x", "x0_prev") if alias else ("out", "x0_out")
    written = (["resid"] if mode == 0 else []) + ["out_bf16", "out2_bf16", out_name, x0_name]
    before = ar.mem.clone()
    f = fp32_coefficients(c["coef"])
    call = dict(eps=ar.ptr("eps"), eps_text=ar.ptr("eps_text") if sep_text else 0, x=ar.ptr("x"), x0_prev=ar.ptr("x0_prev") if hist else 0,
                target=ar.ptr("target") if mode == 0 else 0, resid=ar.ptr("resid"), keep=ar.ptr("keep") if masked else 0,
                mask=ar.ptr("mask") if masked else 0, out=ar.ptr(out_name), x0_out=ar.ptr(x0_name), out_bf16=ar.ptr("out_bf16"),
                out2_bf16=ar.ptr("out2_bf16"), nb=nb, chw=chw, hw=hw, mode=mode, guidance=GUIDANCE, v_prediction=int(v), **f)
    runs = []
    for _ in range(2):
        ar.mem.copy_(before)
        lib.edit_step2(stream(), **call)
        torch.cuda.synchronize()
        runs.append(ar.mem.clone())
    tag = (f"nb {nb} chw {chw} mode {mode} {'v' if v else 'eps'} {'last' if last else 'mid'} {'hist' if hist else 'first-order'}"
           f"{' mask' if masked else ''} {cls}{' eps_text' if sep_text else ''}{' alias' if alias else ''}")
    assert torch.equal(runs[0], runs[1]), f"{tag}: two runs differ"
    same = torch.ones_like(ar.mem, dtype=torch.bool)
    for nm in written:
        same[ar.off[nm]:ar.off[nm] + ar.sizes[nm]] = False
    assert torch.equal(ar.mem[same], before[same]), f"{tag}: a byte outside the outputs changed (fences, inputs)"
    got = {"out": ar.view(out_name, F32).cpu(), "x0_out": ar.view(x0_name, F32).cpu(), "resid": ar.view("resid", F32).cpu()}
    want = step_oracle(c["eps"][:n], c["eps"][n:], c["x"], c["coef"], GUIDANCE, v, mode, c["x0_prev"] if hist else None,
                       c["target"], c["resid"], c["keep"] if masked else None, _per_element(c["mask"], nb, chw, hw) if masked else None)
    worst = {k: check_elementwise(f"{tag} {k}", got[k], ref, bound)[0] for k, (ref, bound) in want.items()}
    if mode == 1:
        assert torch.equal(got["resid"], c["resid"]), f"{tag}: mode 1 wrote resid"
    for nm in ("out_bf16", "out2_bf16"):
        assert torch.equal(_bits(ar.view(nm, BF).cpu().float()), _bits(got["out"].to(BF).float())), f"{tag}: {nm} is not the rounding of out"
    print(f"[edit2-kernel] {tag}: worst err / bound " + ", ".join(f"{k} {w:.3f}" for k, w in worst.items()))
    return worst


@pytest.mark.parametrize("last", [False, True], ids=["mid", "last"])
@pytest.mark.parametrize("v", [False, True], ids=["eps", "v"])
@pytest.mark.parametrize("mode", [0, 1], ids=["invert", "edit"])
def test_edit_step2_per_element(dev, mode, v, last):
    forms = [(h, m) for h in (False, True) for m in ((False, True) if mode == 1 else (False,))]
    worst = {}
    for k, (nb, (chw, hw), cls, (hist, masked)) in enumerate(itertools.product((1, 2), SHAPES, ("normal", "large", "zero_eps"), forms)):
        w = run_kernel_case(dev, nb, chw, hw, mode, v, last, hist, masked, cls, seed=4000 * mode + 2000 * v + 1000 * last + k)
        for name, r in w.items():
            key = (name, "hist" if hist else "first-order", "mask" if masked else "plain")
            worst[key] = max(worst.get(key, 0.0), r)
    print(f"[edit2-kernel] mode {mode} {'v' if v else 'eps'} {'last' if last else 'mid'}: " + "; ".join(f"{' '.join(k)} {r:.3f}" for k, r in sorted(worst.items())))


@pytest.mark.parametrize("what", ["eps_text", "alias"])
@pytest.mark.parametrize("mode", [0, 1], ids=["invert", "edit"])
def test_edit_step2_separate_text_half_and_the_two_aliases(dev, mode, what):
    for chw, hw in SHAPES[1:]:
        run_kernel_case(dev, 2, chw, hw, mode, False, False, True, mode == 1, "normal", sep_text=what == "eps_text", alias=what == "alias", seed=90 + mode)


# ---------------------------------------------------------------------------------------------------------------------------------
# without a history: slh_ddpm_edit_step / slh_ddpm_edit_blend, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chw,hw", SHAPES[1:])
def test_first_order_form_is_the_old_kernels_bit_for_bit(dev, chw, hw):
    nb, n = 2, 2 * chw
    for k, (v, last) in enumerate(itertools.product((False, True), (False, True))):
        c = {name: (t.to(dev) if torch.is_tensor(t) else t) for name, t in draw_case(nb, chw, hw, last, False, "normal", 300 + k).items()}
        f = fp32_coefficients(c["coef"])
        new = lambda: tuple(torch.full((n,), float("nan"), device=dev) for _ in range(2)) + tuple(torch.full((n,), float("nan"), device=dev, dtype=BF) for _ in range(2))
        old_common = dict(eps=c["eps"].data_ptr(), x=c["x"].data_ptr(), nb=nb, chw=chw, guidance=GUIDANCE, v_prediction=int(v), **f)
        new_common = dict(eps=c["eps"].data_ptr(), x=c["x"].data_ptr(), nb=nb, chw=chw, hw=hw, guidance=GUIDANCE, v_prediction=int(v), **f)
        # mode 0
        (o0, r0, a0, b0), (o1, r1, a1, b1) = new(), new()
        lib.call(lib.OP_DDPM_EDIT, lib.DdpmEditDesc(target=c["target"].data_ptr(), resid=r0.data_ptr(), out=o0.data_ptr(), out_bf16=a0.data_ptr(),
                                                     out2_bf16=b0.data_ptr(), mode=0, **old_common), stream())
        lib.edit_step2(stream(), target=c["target"].data_ptr(), resid=r1.data_ptr(), out=o1.data_ptr(), out_bf16=a1.data_ptr(),
                       out2_bf16=b1.data_ptr(), mode=0, **new_common)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o0).all()) and all(torch.equal(p, q) for p, q in ((o0, o1), (r0, r1), (a0, a1), (b0, b1))), ("mode 0", v, last)
        # mode 1 over those residuals: mode 0's out again, from both kernels
        (o2, _, a2, b2), (o3, _, a3, b3) = new(), new()
        lib.call(lib.OP_DDPM_EDIT, lib.DdpmEditDesc(resid=r0.data_ptr(), out=o2.data_ptr(), out_bf16=a2.data_ptr(), out2_bf16=b2.data_ptr(), mode=1,
                                                     **old_common), stream())
        lib.edit_step2(stream(), resid=r0.data_ptr(), out=o3.data_ptr(), out_bf16=a3.data_ptr(), out2_bf16=b3.data_ptr(), mode=1, **new_common)
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in ((o2, o3), (a2, a3), (b2, b3), (o3, o0))), ("mode 1", v, last)
        # with a mask: slh_ddpm_edit_blend; NaN in epsilon where the mask is 0 and in keep where it is 1 reaches neither out
        m = _per_element(c["mask"], nb, chw, hw)
        eps, keep = c["eps"].clone(), c["keep"].clone()
        eps[:n][m == 0] = float("nan")
        keep[m == 1] = float("nan")
        (o4, _, a4, b4), (o5, _, a5, b5) = new(), new()
        blend = dict(resid=c["resid"].data_ptr(), keep=keep.data_ptr(), mask=c["mask"].data_ptr())
        lib.call(lib.OP_DDPM_EDIT_BLEND, lib.DdpmEditBlendDesc(out=o4.data_ptr(), out_bf16=a4.data_ptr(), out2_bf16=b4.data_ptr(), hw=hw,
                                                               **{**old_common, "eps": eps.data_ptr()}, **blend), stream())
        lib.edit_step2(stream(), out=o5.data_ptr(), out_bf16=a5.data_ptr(), out2_bf16=b5.data_ptr(), mode=1, **{**new_common, "eps": eps.data_ptr()}, **blend)
        torch.cuda.synchronize()
        assert bool((m == 0).any()) and bool((m == 1).any()) and bool(((m > 0) & (m < 1)).any())
        assert bool(torch.isfinite(o5).all()), "a NaN on the side that is not selected never reaches out"
        assert torch.equal(_bits(o5[m == 0]), _bits(c["keep"][m == 0])), "mask 0: keep's bits"
        assert all(torch.equal(p, q) for p, q in ((o4, o5), (a4, a5), (b4, b5))), ("blend", v, last)


# ---------------------------------------------------------------------------------------------------------------------------------
# the engine: tiny SDXL, 16^2 latents, 6 steps, skip 0, start_noise on the grid's third point
# ---------------------------------------------------------------------------------------------------------------------------------
STEPS, LIVE, SCALE, GS = 6, 4, 2.0, 3.0
CHW, PIX = 4 * HW * HW, HW * HW
TS = SCH.make_timesteps(STEPS)
START = TS[STEPS - LIVE]
MOMENTUM = (0.5, 0.4)


def _spy(monkeypatch):
    """what the step launches go through: the opcodes of lib.call and the calls of lib.edit_step2"""
    seen = []
    real_call, real_step2 = lib.call, lib.edit_step2
    monkeypatch.setattr(lib, "call", lambda op, *a, **k: (seen.append(op), real_call(op, *a, **k))[1])
    monkeypatch.setattr(lib, "edit_step2", lambda *a, **k: (seen.append("edit_step2"), real_step2(*a, **k))[1])
    return seen


@pytest.mark.parametrize("form", ["none", "store", "sliders"])
def test_order2_on_the_engine(dev, monkeypatch, form):
    cfg, eng, ed = _editor("tiny_sdxl", form, dev)
    ctx, pooled, x0 = _cond(cfg, dev, seed=41)
    seen = _spy(monkeypatch)
    sp = ed.invert(ctx, x0, steps=STEPS, skip=0, guidance_scale=GS, seed=3, pooled=pooled, order=2)
    torch.cuda.synchronize()
    steps_of = lambda: [s for s in seen if s in (lib.OP_DDPM_EDIT, lib.OP_DDPM_EDIT_BLEND, "edit_step2")]
    assert sp.order == 2 and sp.timesteps == TS and steps_of() == ["edit_step2"] * STEPS, "one launch of the new entry point per step, no old one"
    assert bool(torch.isfinite(sp.resid).all()) and torch.equal(sp.visited[-1], sp.recon)
    assert torch.equal(ed.edit_latents(sp, scale=0.0), sp.recon), "scale 0 walks the inversion's latents again, bit for bit"
    err = (sp.recon.double() - x0.double()).abs()
    assert bool((err <= 2.0 ** -22 * (2.0 * x0.double().abs() + sp.resid[-1].double().abs())).all()), "the last step is first order"
    bare = NoiseSpace(**{**sp._map(lambda t: t), "visited": None})
    assert torch.equal(ed.trajectory(bare).visited, sp.visited), "trajectory rebuilds visited bit for bit"
    a = ed.edit_latents(sp, scale=SCALE, start_noise=START)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, ed.edit_latents(sp, scale=SCALE, start_noise=START))
    assert torch.equal(a, sp.recon) == (form == "none"), "a slider moves the result; without one every scale is the reconstruction"
    if form != "none":
        half = torch.zeros(HW, HW)
        half[:, HW // 2:] = 1.0
        out = ed.edit_latents(sp, scale=SCALE, start_noise=START, mask=half)
        assert torch.equal(out[..., :HW // 2], sp.recon[..., :HW // 2]), "outside the mask: the reconstruction, bit for bit"
        assert not torch.equal(out[..., HW // 2:], sp.recon[..., HW // 2:])
        assert torch.equal(ed.edit_latents(sp, scale=SCALE, start_noise=START, mask=torch.ones(HW, HW)), a), "an all-one mask is the unmasked edit"
        soft = torch.rand(HW, HW, generator=torch.Generator().manual_seed(1))
        assert torch.equal(ed.edit_latents(sp, scale=0.0, mask=soft), sp.recon), "scale 0 under any mask"
    assert lib.OP_DDPM_EDIT not in seen and lib.OP_DDPM_EDIT_BLEND not in seen
    # order 1 through the same editor: the launches it always made, and the bits of a loop over slh_ddpm_edit_step written out here
    del seen[:]
    one = ed.invert(ctx, x0, steps=STEPS, skip=0, guidance_scale=GS, seed=3, pooled=pooled)
    assert one.order == 1 and steps_of() == [lib.OP_DDPM_EDIT] * STEPS
    assert torch.equal(ed.edit_latents(one, scale=0.0), one.recon) and "edit_step2" not in seen
    assert torch.equal(one.resid[0], sp.resid[0]) and not torch.equal(one.resid[1], sp.resid[1]), "the first step is first order in both"
    path = build_path(SCH, x0, TS, 3)
    drv = Pass(eng, eng.plan(2, HW, HW, "on" if form == "store" else "off"))
    drv.load_cond(ctx, pooled, None)
    x, resid = path[0].clone(), torch.full_like(path, float("nan"))
    drv.load_latents(x)
    if form == "store":
        eng.set_lora(True, 0.0)
    for i, t in enumerate(TS):
        drv.run(t, i == 0, stream())
        smp = drv.io["sample"]
        lib.call(lib.OP_DDPM_EDIT, lib.DdpmEditDesc(eps=drv.io["eps"].ptr, x=x.data_ptr(), target=(path[i + 1] if i + 1 < STEPS else x0).data_ptr(),
                                                     resid=resid[i].data_ptr(), out=x.data_ptr(), out_bf16=smp.ptr, out2_bf16=smp.ptr + CHW * 2, nb=1,
                                                     chw=CHW, guidance=GS, mode=0, v_prediction=0,
                                                     **fp32_coefficients(ddpm_step_coefficients(SCH, t, STEPS, 1.0))), stream())
    if form == "store":
        eng.set_lora(False)
    torch.cuda.synchronize()
    assert torch.equal(resid, one.resid) and torch.equal(x, one.recon), "the order-1 inversion is the loop over slh_ddpm_edit_step"


def test_residuals_agree_with_the_fp32_reference_over_the_engines_predictions(dev, monkeypatch):
    cfg, eng, ed = _editor("tiny_sdxl", "none", dev)
    ctx, pooled, x0 = _cond(cfg, dev, seed=41)
    seen = {}
    real = ed._launch_step

    def recording(p, t, *a, **k):
        e = p.io["eps"].tensor.detach().clone().cpu()
        seen[int(t)] = (e[:1], e[1:2])
        return real(p, t, *a, **k)
    monkeypatch.setattr(ed, "_launch_step", recording)
    sp = ed.invert(ctx, x0, steps=STEPS, skip=0, guidance_scale=GS, seed=3, pooled=pooled, order=2)
    torch.cuda.synchronize()
    ref = invert_reference(lambda x_bf16, t, m: seen[int(t)], x0.cpu(), SCH, STEPS, 0, 1.0, GS, 3, torch.float32, order=2)
    assert torch.equal(ref.x_start, sp.x_start.cpu())
    # per step, both residuals are within the kernel's mode-0 bound of float64 on the reference chain's inputs
    path = build_path(SCH, x0.cpu(), TS, 3)
    hist, worst = None, 0.0
    for i, t in enumerate(TS):
        x = ref.x_start if i == 0 else ref.visited[i - 1]
        coef = chain_coefficients(SCH, TS, i, STEPS, 1.0, 2)
        mu, x0h, b_mu, _, _, _ = mu_oracle_and_bound(*seen[t], x, coef, GS, False, hist if "c_corr" in coef else None)
        target = (path[i + 1] if i + 1 < STEPS else x0.cpu()).double()
        bound = b_mu + U * (target.abs() + mu.abs())
        for name, r in (("reference", ref.resid[i]), ("engine", sp.resid[i].cpu())):
            worst = max(worst, check_elementwise(f"step {i} {name} resid", r, target - mu, bound)[0])
        hist = x0h.float()
    same = torch.equal(ref.resid, sp.resid.cpu())
    print(f"[edit2-engine] residuals against float64 over the engine's predictions: worst err / bound {worst:.3f}; "
          f"engine and fp32 reference {'agree bit for bit' if same else 'differ in bits'}; |recon - reference recon| max "
          f"{float((ref.recon - sp.recon.cpu()).abs().max()):.3e}")


def _hand_edit2(h: _Hand, sp, scale, start_noise, mask=None):
    """the order-2 direction edit from the public pieces: the engine pass, DirectionGuide's launches (_Hand) and lib.edit_step2"""
    x = sp.x_start.clone()
    hist = torch.full_like(x, float("nan"))
    h.drv.load_latents(x)
    for i, t in enumerate(sp.timesteps):
        first, live = i == 0, t <= start_noise
        if live and not h.wide:
            h.widen(x)
            first = True
        h.drv.run(t, first, h.s)
        buf, eps = h.drv.io["sample"], h.drv.io["eps"]
        coef = fp32_coefficients(ddpm_step2_coefficients(SCH, t, STEPS, 1.0, sp.timesteps[i - 1] if i else None))
        lib.edit_step2(h.s, eps=eps.ptr, eps_text=h.guide() if live else 0, x=x.data_ptr(), x0_prev=hist.data_ptr() if "c_corr" in coef else 0,
                       resid=sp.resid[i].data_ptr(), keep=0 if mask is None else sp.visited[i].data_ptr(), mask=0 if mask is None else mask.data_ptr(),
                       out=x.data_ptr(), x0_out=hist.data_ptr(), out_bf16=buf.ptr, out2_bf16=buf.ptr + CHW * 2, nb=1, chw=CHW, hw=PIX, mode=1,
                       guidance=GS, **coef)
        if live:
            h.spread()
    return x


@pytest.mark.parametrize("momentum", [None, MOMENTUM])
def test_order2_direction_edits_against_a_loop_of_the_public_pieces(dev, tiny, momentum):
    cfg, net, _, _, _ = tiny
    eng = UNetEngine(cfg, net.state_dict(), dev)
    ed = SliderEditor(eng)
    ctx, pooled, x0 = _cond(cfg, dev, seed=41)
    sp = ed.invert(ctx, x0, steps=STEPS, skip=0, guidance_scale=GS, seed=3, pooled=pooled, order=2)
    assert sum(t <= START for t in TS) == LIVE
    dirs = _directions(cfg, dev, 2)
    steer = dict(directions=dirs, direction_quantile=0.9, direction_momentum=momentum)
    assert torch.equal(ed.edit_latents(sp, scale=0.0, start_noise=START, **steer), sp.recon), "scale 0 is the reconstruction"
    got = ed.edit_latents(sp, scale=SCALE, start_noise=START, **steer)
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, sp.recon), "the directions act"
    want = _hand_edit2(_Hand(eng, sp.ctx, sp.pooled, dirs, 0.9, momentum, SCALE), sp, SCALE, START)
    assert torch.equal(got, want), "the history survives the move to the wide plan; the loop of the public pieces gives the same bits"
    half = torch.zeros(HW, HW)
    half[:, HW // 2:] = 1.0
    out = ed.edit_latents(sp, scale=SCALE, start_noise=START, mask=half, **steer)
    assert torch.equal(out[..., :HW // 2], sp.recon[..., :HW // 2]) and not torch.equal(out[..., HW // 2:], sp.recon[..., HW // 2:])
    assert torch.equal(out, _hand_edit2(_Hand(eng, sp.ctx, sp.pooled, dirs, 0.9, momentum, SCALE), sp, SCALE, START, mask=half.to(dev).contiguous()))
    assert torch.equal(ed.edit_latents(sp, scale=0.0), sp.recon), "the editor is as it was"


# ---------------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_order2_saves_and_reloads(dev, tmp_path, monkeypatch):
    from PIL import Image
    import sliders_amd.model_util as mu
    cfg = CONFIGS["tiny_sd1"]()
    engines = {}

    def tiny_engine(model, device, seed):     # --synthetic on the tiny SD-1 topology, built once for the runs below
        if seed not in engines:
            engines[seed] = UNetEngine(cfg, mu.random_state_dict(cfg, device, seed), device)
        return engines[seed]
    monkeypatch.setattr(mu, "synthetic_engine", tiny_engine)
    seen = _spy(monkeypatch)
    img = str(tmp_path / "photo.png")
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (128, 128, 3), dtype=np.uint8)).save(img)
    inv = str(tmp_path / "inversion.pt")
    common = ["--model", "sd1", "--synthetic", "--steps", "6", "--skip", "0", "--guidance_scale", "3", "--res", "128"]
    first = edit.main(common + ["--image", img, "--order", "2", "--scales=0", "--save_inversion", inv, "--out", str(tmp_path / "first")])
    assert seen.count("edit_step2") == 12 and lib.OP_DDPM_EDIT not in seen, "six steps of the inversion, six of the edit"
    assert torch.load(inv, map_location="cpu")["order"] == 2 and NoiseSpace.load(inv).order == 2
    read = lambda out, name: open(os.path.join(out, name), "rb").read()
    assert read(first, "scale_0.png") == read(first, "recon.png"), "scale 0 is the reconstruction"
    second = edit.main(common + ["--load_inversion", inv, "--scales=0", "--out", str(tmp_path / "second")])
    assert read(second, "scale_0.png") == read(first, "scale_0.png") and read(second, "recon.png") == read(first, "recon.png")
    assert seen.count("edit_step2") == 18 and lib.OP_DDPM_EDIT not in seen, "the file decides the order"
    plain = edit.main(common + ["--image", img, "--scales=0", "--out", str(tmp_path / "plain")])
    assert seen.count("edit_step2") == 18 and seen.count(lib.OP_DDPM_EDIT) == 12, "the default is order 1, on the old launches"
    assert os.path.getsize(os.path.join(plain, "scale_0.png")) > 0
