"""GPU: localised slider edits (sliders_amd/edit.py, docs/EDIT.md "Localised edits") - slh_ddpm_edit_blend and slh_eps_absdiff element by
element against float64, the identities of the masked edit on the engine in every slider form, the masked editor and the footprint
against loops written out here, the CLI.

Kernel bounds (docs/EDIT.md derives them), u = 2^-24, E = |eps_u| + g (|eps_t| + |eps_u|), S = the mu expression on absolute values:
    blend     B_e = 9 u (S + |resid|) is the bound of the unmasked step's e = mu + resid; with k = keep, m = mask
              |out - (k + m (e - k))| <= m B_e + 4 u (|k| + m |e - k|);   m == 0: out == k;   m == 1: out == slh_ddpm_edit_step's, bit for bit
    absdiff   C = chw / hw channels:  |out - sum_c |e_a - e_b|| <= (C + 4) u sum_c (E_a + E_b)
"""
import itertools
import os

import numpy as np
import pytest
import torch

from sliders_amd import edit, lib
from sliders_amd.config import CONFIGS
from sliders_amd.ddim import DDIMSchedule
from sliders_amd.edit import (NoiseSpace, SliderEditor, ddpm_mu_reference, ddpm_step_coefficients, feather_mask, footprint_mask,
                              fp32_coefficients)
from tests.test_edit_gpu import CASES, GS, HW, SKIP, STEPS, Arena, _editor, _hand_inputs, _hand_step, _inputs, s_mu
from tests.test_merge_gpu import drawn_slider
from tests.util import check_elementwise, stream

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUIDANCE = 7.5
BF, F32 = torch.bfloat16, torch.float32
SHAPES = [(4, 1), (900, 225), (1024, 256)]           # (chw, hw): one pixel; an odd size over several blocks; whole blocks
MASKS = ("uniform", "binary", "zeros", "ones", "cycle")


def draw_mask(cls, n, g):
    if cls == "uniform":
        return torch.rand(n, generator=g)
    if cls == "binary":
        return (torch.rand(n, generator=g) < 0.5).float()
    if cls == "cycle":
        return torch.tensor([0.0, 1.0, 0.5, 2.0 ** -20]).repeat(n // 4 + 1)[:n]
    return torch.full((n,), 1.0 if cls == "ones" else 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# slh_ddpm_edit_blend, element by element
# ---------------------------------------------------------------------------------------------------------------------------------
def run_blend_case(dev, nb, chw, hw, v, last, cls, mcls, sep_text=False, alias=False, keep_is_e=False, seed=0):
    n = nb * chw
    g = torch.Generator().manual_seed(seed)
    big = 1e3 if cls == "large" else 1.0
    eps = torch.randn(2 * n, generator=g).to(BF)
    if cls == "zero_eps":
        eps.zero_()
    x = torch.randn(n, generator=g) * big
    resid = torch.randn(n, generator=g) * big
    keep = torch.randn(n, generator=g) * big
    mask = draw_mask(mcls, nb * hw, g)
    coef = ddpm_step_coefficients(DDIMSchedule(), 0 if last else 500, 50, 1.0)
    f = fp32_coefficients(coef)
    # what slh_ddpm_edit_step mode 1 writes on these inputs: the m == 1 side, and `keep` of the scale-0 case
    eps_d, x_d, resid_d, e_d = eps.to(dev), x.to(dev), resid.to(dev), torch.full((n,), float("nan"), device=dev)
    lib.call(lib.OP_DDPM_EDIT, lib.DdpmEditDesc(eps=eps_d.data_ptr(), x=x_d.data_ptr(), resid=resid_d.data_ptr(), out=e_d.data_ptr(), nb=nb, chw=chw,
                                                 guidance=GUIDANCE, mode=1, v_prediction=int(v), **f), stream())
    torch.cuda.synchronize()
    e_step = e_d.cpu()
    if keep_is_e:
        keep = e_step.clone()
    sizes = {"eps": 4 * n, "eps_text": 2 * n, "x": 4 * n, "resid": 4 * n, "keep": 4 * n, "mask": 4 * nb * hw, "out": 4 * n, "out_bf16": 2 * n,
             "out2_bf16": 2 * n}
    ar = Arena(dev, sizes)
    ar.view("x", F32).copy_(x)
    ar.view("resid", F32).copy_(resid)
    ar.view("keep", F32).copy_(keep)
    ar.view("mask", F32).copy_(mask)
    if sep_text:
        ar.view("eps", BF)[:n].copy_(eps[:n])
        ar.view("eps", BF)[n:].fill_(1e4)            # a decoy after the uncond half: must not be read
        ar.view("eps_text", BF).copy_(eps[n:])
    else:
        ar.view("eps", BF).copy_(eps)
    out_name = "x" if alias else "out"
    written = ["out_bf16", "out2_bf16", out_name]
    before = ar.mem.clone()
    d = lib.DdpmEditBlendDesc(eps=ar.ptr("eps"), eps_text=ar.ptr("eps_text") if sep_text else 0, x=ar.ptr("x"), resid=ar.ptr("resid"),
                              keep=ar.ptr("keep"), mask=ar.ptr("mask"), out=ar.ptr(out_name), out_bf16=ar.ptr("out_bf16"),
                              out2_bf16=ar.ptr("out2_bf16"), nb=nb, chw=chw, hw=hw, guidance=GUIDANCE, v_prediction=int(v), **f)
    runs = []
    for _ in range(2):
        ar.mem.copy_(before)
        lib.call(lib.OP_DDPM_EDIT_BLEND, d, stream())
        torch.cuda.synchronize()
        runs.append(ar.mem.clone())
    tag = (f"nb {nb} chw {chw} hw {hw} {'v' if v else 'eps'} {'last' if last else 'mid'} {cls} mask {mcls}{' eps_text' if sep_text else ''}"
           f"{' alias' if alias else ''}{' keep = e' if keep_is_e else ''}")
    assert torch.equal(runs[0], runs[1]), f"{tag}: two runs differ"
    untouched = torch.ones_like(ar.mem, dtype=torch.bool)
    for nm in written:
        untouched[ar.off[nm]:ar.off[nm] + ar.sizes[nm]] = False
    assert torch.equal(ar.mem[untouched], before[untouched]), f"{tag}: a byte outside the outputs changed (fences, inputs)"
    out = ar.view(out_name, F32).cpu()
    assert torch.equal(ar.view("out_bf16", BF).cpu(), out.to(BF)) and torch.equal(ar.view("out2_bf16", BF).cpu(), out.to(BF)), f"{tag}: the bf16 copies"
    m = mask.reshape(nb, 1, hw).expand(nb, chw // hw, hw).reshape(n)         # element i reads mask[b * hw + i % hw]
    assert torch.equal(out[m == 0], keep[m == 0]), f"{tag}: m == 0 must give keep exactly"
    assert torch.equal(out[m == 1], e_step[m == 1]), f"{tag}: m == 1 must give slh_ddpm_edit_step's out exactly"
    if keep_is_e:
        assert torch.equal(out, keep), f"{tag}: e == keep must give keep under any mask (identity 3 at kernel level)"
    # float64 on the same inputs
    eu, et = eps[:n], eps[n:]
    e64 = ddpm_mu_reference(eu, et, x, coef, GUIDANCE, v, torch.float64) + resid.double()
    E = eu.double().abs() + GUIDANCE * (et.double().abs() + eu.double().abs())
    B_e = 9 * U * (s_mu(f, x.double().abs(), E, v) + resid.double().abs())
    k64, m64 = keep.double(), m.double()
    ref = k64 + m64 * (e64 - k64)
    bound = m64 * B_e + 4 * U * (k64.abs() + m64 * (e64 - k64).abs())
    return check_elementwise(f"{tag} out", out, ref, bound)[0]


@pytest.mark.parametrize("last", [False, True], ids=["mid", "last"])
@pytest.mark.parametrize("v", [False, True], ids=["eps", "v"])
def test_ddpm_edit_blend_per_element(dev, v, last):
    worst = {}
    cases = itertools.product((1, 2), SHAPES, ("normal", "large", "zero_eps"), MASKS)
    for k, (nb, (chw, hw), cls, mcls) in enumerate(cases):
        w = run_blend_case(dev, nb, chw, hw, v, last, cls, mcls, seed=5000 + 1000 * v + 500 * last + k)
        worst[mcls] = max(worst.get(mcls, 0.0), w)
    print(f"[edit-blend] {'v' if v else 'eps'} {'last' if last else 'mid'}: worst err / bound " + ", ".join(f"{k} {w:.3f}" for k, w in worst.items()))


@pytest.mark.parametrize("what", ["eps_text", "alias"])
def test_ddpm_edit_blend_separate_text_half_and_in_place(dev, what):
    for mcls in ("uniform", "cycle"):
        run_blend_case(dev, 2, 900, 225, False, False, "normal", mcls, sep_text=what == "eps_text", alias=what == "alias", seed=91)


def test_ddpm_edit_blend_returns_keep_where_the_edit_equals_it(dev):
    """keep = what slh_ddpm_edit_step mode 1 wrote on the same inputs: out == keep under every mask - identity 3 at kernel level"""
    for k, (v, last, mcls) in enumerate(itertools.product((False, True), (False, True), MASKS)):
        run_blend_case(dev, 2, 900, 225, v, last, "normal", mcls, keep_is_e=True, seed=7000 + k)
        run_blend_case(dev, 1, 1024, 256, v, last, "large", mcls, keep_is_e=True, alias=True, seed=7100 + k)


# ---------------------------------------------------------------------------------------------------------------------------------
# slh_eps_absdiff, element by element
# ---------------------------------------------------------------------------------------------------------------------------------
def run_absdiff_case(dev, nb, chw, hw, cls, sep_text=False, seed=0):
    n = nb * chw
    g = torch.Generator().manual_seed(seed)
    big = 1e3 if cls == "large" else 1.0
    a = (torch.randn(2 * n, generator=g) * big).to(BF)
    b = a.clone() if cls == "equal" else (torch.randn(2 * n, generator=g) * big).to(BF)
    sizes = {"a": 4 * n, "a_text": 2 * n, "b": 4 * n, "b_text": 2 * n, "out": 4 * nb * hw}
    ar = Arena(dev, sizes)
    for nm, t in (("a", a), ("b", b)):
        if sep_text:
            ar.view(nm, BF)[:n].copy_(t[:n])
            ar.view(nm, BF)[n:].fill_(1e4)           # decoys
            ar.view(nm + "_text", BF).copy_(t[n:])
        else:
            ar.view(nm, BF).copy_(t)
    before = ar.mem.clone()
    d = lib.EpsAbsdiffDesc(eps_a=ar.ptr("a"), eps_a_text=ar.ptr("a_text") if sep_text else 0, eps_b=ar.ptr("b"),
                           eps_b_text=ar.ptr("b_text") if sep_text else 0, out=ar.ptr("out"), nb=nb, chw=chw, hw=hw, guidance=GUIDANCE)
    runs = []
    for _ in range(2):
        ar.mem.copy_(before)
        lib.call(lib.OP_EPS_ABSDIFF, d, stream())
        torch.cuda.synchronize()
        runs.append(ar.mem.clone())
    tag = f"absdiff nb {nb} chw {chw} hw {hw} {cls}{' eps_text' if sep_text else ''}"
    assert torch.equal(runs[0], runs[1]), f"{tag}: two runs differ"
    untouched = torch.ones_like(ar.mem, dtype=torch.bool)
    untouched[ar.off["out"]:ar.off["out"] + ar.sizes["out"]] = False
    assert torch.equal(ar.mem[untouched], before[untouched]), f"{tag}: a byte outside the output changed"
    out = ar.view("out", F32).cpu().reshape(nb, hw)
    C = chw // hw
    ua, ta, ub, tb = (t.double().reshape(nb, C, hw) for t in (a[:n], a[n:], b[:n], b[n:]))
    ea, eb = ua + GUIDANCE * (ta - ua), ub + GUIDANCE * (tb - ub)
    ref = (ea - eb).abs().sum(1)
    Ea, Eb = ua.abs() + GUIDANCE * (ta.abs() + ua.abs()), ub.abs() + GUIDANCE * (tb.abs() + ub.abs())
    bound = (C + 4) * U * (Ea + Eb).sum(1)
    if cls == "equal":
        assert torch.equal(out, torch.zeros(nb, hw)), f"{tag}: equal pairs must give exact zeros"
    else:
        assert float(out.min()) > 0.0, tag
    return check_elementwise(tag, out, ref, bound)[0]


def test_eps_absdiff_per_element(dev):
    worst = 0.0
    for k, (nb, (chw, hw), cls) in enumerate(itertools.product((1, 2), SHAPES, ("normal", "large", "equal"))):
        worst = max(worst, run_absdiff_case(dev, nb, chw, hw, cls, seed=300 + k))
    for k, (nb, (chw, hw)) in enumerate(itertools.product((1, 2), SHAPES)):
        worst = max(worst, run_absdiff_case(dev, nb, chw, hw, "normal", sep_text=True, seed=400 + k))
    print(f"[edit-absdiff] worst err / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------------------
SCALE, START = 1.5, 500


def engine_masks(dev):
    half = torch.zeros(HW, HW)
    half[:, HW // 2:] = 1.0                              # the right half-plane: binary
    square = torch.zeros(HW, HW)
    square[4:11, 3:12] = 1.0
    return {"half": half.to(dev), "feathered": feather_mask(square, 1.0).to(dev)}


@pytest.mark.parametrize("name,form,prediction", CASES)
def test_masked_edit_identities_on_the_engine(dev, monkeypatch, name, form, prediction):
    cfg, eng, ed = _editor(name, form, dev, prediction)
    ctx, pooled, x0 = _inputs(cfg, dev)
    snap = {k: v.clone() for k, v in eng.w.t.items()} if form == "sliders" else None
    restored = lambda: not ed.merger.merged and all(torch.equal(v, snap[k]) for k, v in eng.w.t.items())
    sp = ed.invert(ctx, x0, steps=STEPS, skip=SKIP, guidance_scale=GS, seed=3, pooled=pooled)
    torch.cuda.synchronize()
    assert sp.visited.shape == sp.resid.shape and sp.visited.dtype == torch.float32 and torch.equal(sp.visited[-1], sp.recon)
    plain = ed.edit_latents(sp, scale=SCALE, start_noise=START)
    assert torch.equal(ed.edit_latents(sp, scale=0.0), sp.recon)
    ms = engine_masks(dev)
    kw = dict(scale=SCALE, start_noise=START)
    # 1 and 2
    assert torch.equal(ed.edit_latents(sp, mask=torch.ones(HW, HW), **kw), plain), "identity 1: all ones is the unmasked edit"
    assert torch.equal(ed.edit_latents(sp, mask=torch.zeros(1, 1, HW, HW, device=dev), **kw), sp.recon), "identity 2: all zeros is the reconstruction"
    for mname, m in ms.items():
        # 3
        assert torch.equal(ed.edit_latents(sp, scale=0.0, mask=m), sp.recon), f"identity 3, {mname}"
        out = ed.edit_latents(sp, mask=m, **kw)
        assert out.dtype == torch.float32 and bool(torch.isfinite(out).all())
        # 4 (for the soft mask: where it is exactly 0)
        off = (m == 0)[None, None].expand_as(out)
        assert bool(off.any()) and torch.equal(out[off], sp.recon[off]), f"identity 4, {mname}: outside the mask the reconstruction's bits"
        if form != "none":
            on = (m > 0.5)[None, None].expand_as(out)            # (a feathered mask need not reach 1 exactly: its taps sum to 1 up to rounding)
            assert bool(on.any()) and not torch.equal(out[on], sp.recon[on]) and not torch.equal(out, plain), f"{mname}: the slider acts inside the mask, and only there"
        else:
            assert torch.equal(out, sp.recon), "no slider: every scale is the reconstruction"
        # 5
        assert torch.equal(ed.edit_latents(sp, mask=m[None], **kw), out), f"{mname}: two runs"
        bare = NoiseSpace(**{**sp._map(lambda t: t), "visited": None})
        assert torch.equal(ed.edit_latents(bare, mask=m, **kw), out) and torch.equal(bare.visited, sp.visited), f"{mname}: trajectory gives visited back"
    with pytest.raises(ValueError):
        ed.edit_latents(sp, mask=torch.full((HW, HW), 1.5), **kw)
    with pytest.raises(ValueError):
        ed.edit_latents(sp, mask=torch.ones(HW, HW + 1), **kw)
    wrong = NoiseSpace(**{**sp._map(lambda t: t), "visited": None, "recon": sp.recon + 1.0})
    with pytest.raises(RuntimeError, match="recon"):
        ed.trajectory(wrong)
    assert torch.equal(ed.edit_latents(sp, scale=SCALE, start_noise=START), plain), "the unmasked edit is what it was before the masked calls"
    if form != "sliders":
        return
    assert restored(), "every weight tensor has its original bits after the masked edits"

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
        ed.edit_latents(sp, scale=SCALE, start_noise=2000, mask=ms["half"])
    torch.cuda.synchronize()
    monkeypatch.setattr(edit, "ddpm_step_coefficients", real)
    assert restored(), "an exception inside the masked loop still restores the weights"
    assert torch.equal(ed.edit_latents(sp, scale=0.0, mask=ms["half"]), sp.recon)


def test_saved_inversion_carries_visited_and_edits_to_the_same_bits(dev, tmp_path):
    cfg, eng, ed = _editor("tiny_sd1", "store", dev)
    ctx, pooled, x0 = _inputs(cfg, dev)
    sp = ed.invert(ctx, x0, steps=STEPS, skip=SKIP, guidance_scale=GS, seed=4)
    m = engine_masks(dev)["feathered"]
    path = str(tmp_path / "space.pt")
    sp.save(path)
    back = NoiseSpace.load(path, dev)
    assert back.visited.is_cuda and torch.equal(back.visited, sp.visited)
    want = ed.edit_latents(sp, scale=SCALE, start_noise=START, mask=m)
    assert torch.equal(ed.edit_latents(back, scale=SCALE, start_noise=START, mask=m), want)
    d = torch.load(path, map_location="cpu")
    del d["visited"]                                   # a file saved before masked edits
    torch.save(d, path)
    old = NoiseSpace.load(path, dev)
    assert old.visited is None
    assert torch.equal(ed.edit_latents(old, scale=SCALE, start_noise=START, mask=m), want) and torch.equal(old.visited, sp.visited)


def _hand_start(p, x):
    p.io["sample"].tensor[:1].copy_(x.to(BF))
    p.io["sample"].tensor[1:].copy_(x.to(BF))


def _hand_inversion(eng, p, sch, ts, sp, x0, ctx, pooled):
    """the inversion with OP_DDPM_EDIT, its latents kept: (resid, visited)"""
    path = edit.build_path(sch, x0, ts, sp.seed)
    _hand_inputs(eng, p, ctx, pooled)
    x = path[0].clone()
    _hand_start(p, x)
    resid, visited = torch.full_like(path, float("nan")), torch.full_like(path, float("nan"))
    for i, t in enumerate(ts):
        _hand_step(eng, p, sch, i, t, 0.0, x, resid[i], path[i + 1] if i + 1 < len(ts) else x0, 0)
        visited[i].copy_(x)
    torch.cuda.synchronize()
    return path, resid, visited


def test_masked_editor_equals_the_loops_written_out(dev):
    cfg, eng, ed = _editor("tiny_sdxl", "store", dev)
    ctx, pooled, x0 = _inputs(cfg, dev)
    sp = ed.invert(ctx, x0, steps=STEPS, skip=SKIP, guidance_scale=GS, seed=3, pooled=pooled)
    m = engine_masks(dev)["feathered"]
    got = ed.edit_latents(sp, scale=SCALE, start_noise=START, mask=m)
    torch.cuda.synchronize()
    sch = DDIMSchedule()
    ts = sch.make_timesteps(STEPS)[SKIP:]
    p = eng.plan(2, HW, HW, "on")
    path, resid, visited = _hand_inversion(eng, p, sch, ts, sp, x0, ctx, pooled)
    assert torch.equal(resid, sp.resid) and torch.equal(visited, sp.visited), "the inversion's residuals and latents"
    x = path[0].clone()
    _hand_start(p, x)
    mask = m.reshape(1, HW * HW).contiguous()
    chw, mults, io = x[0].numel(), [], p.io
    for i, t in enumerate(ts):
        mults.append(0.0 if t > START else SCALE)
        eng.set_lora(True, mults[-1])
        io["t"].tensor.fill_(float(t))
        (p.prog if i == 0 or p.prog_text_cached is None else p.prog_text_cached).run(stream())
        lib.call(lib.OP_DDPM_EDIT_BLEND, lib.DdpmEditBlendDesc(
            eps=io["eps"].ptr, x=x.data_ptr(), resid=resid[i].data_ptr(), keep=visited[i].data_ptr(), mask=mask.data_ptr(), out=x.data_ptr(),
            out_bf16=io["sample"].ptr, out2_bf16=io["sample"].ptr + chw * 2, nb=1, chw=chw, hw=HW * HW, guidance=GS, v_prediction=0,
            **fp32_coefficients(ddpm_step_coefficients(sch, t, STEPS, 1.0))), stream())
    eng.set_lora(False)
    torch.cuda.synchronize()
    assert 0.0 in mults and SCALE in mults, "the test must exercise both sides of start_noise"
    assert torch.equal(got, x), "SliderEditor.edit_latents(mask=) and the hand-written loop differ"


# ---------------------------------------------------------------------------------------------------------------------------------
# the footprint
# ---------------------------------------------------------------------------------------------------------------------------------
def test_footprint_equals_the_loop_written_out(dev):
    cfg, eng, ed = _editor("tiny_sdxl", "store", dev)
    ctx, pooled, x0 = _inputs(cfg, dev)
    sp = ed.invert(ctx, x0, steps=STEPS, skip=SKIP, guidance_scale=GS, seed=3, pooled=pooled)
    assert sp.timesteps == [625, 500, 375, 250, 125, 0]
    for draws, idx in ((8, [1, 2, 3]), (2, [1, 3])):            # t_min = 200 <= t <= start_noise = 500
        assert edit.footprint_draws(sp.timesteps, START, draws, 200) == idx
        F = ed.footprint(sp, SCALE, start_noise=START, draws=draws)
        assert torch.equal(F, ed.footprint(sp, SCALE, start_noise=START, draws=draws)), "two calls"
        assert F.shape == (1, HW, HW) and F.dtype == torch.float32 and bool(torch.isfinite(F).all()) and float(F.min()) >= 0.0
        assert float(F.max()) > float(F.min()), "a slider's footprint is not constant"
        assert abs(float(F.mean()) - 1.0) <= 1e-5, "every draw is divided by its own mean"
        # by hand
        p = eng.plan(2, HW, HW, "on")
        _hand_inputs(eng, p, ctx, pooled)
        io = p.io
        off, A, n = [], torch.full((len(idx), 1, HW, HW), float("nan"), device=dev), 0
        for multiplier in (0.0, SCALE):
            for j, i in enumerate(idx):
                _hand_start(p, sp.x_start if i == 0 else sp.visited[i - 1])
                eng.set_lora(True, multiplier)
                io["t"].tensor.fill_(float(sp.timesteps[i]))
                (p.prog if n == 0 or p.prog_text_cached is None else p.prog_text_cached).run(stream())
                n += 1
                if multiplier == 0.0:
                    off.append(io["eps"].tensor.clone())
                else:
                    lib.call(lib.OP_EPS_ABSDIFF, lib.EpsAbsdiffDesc(eps_a=io["eps"].ptr, eps_b=off[j].data_ptr(), out=A[j].data_ptr(), nb=1,
                                                                    chw=4 * HW * HW, hw=HW * HW, guidance=GS), stream())
        eng.set_lora(False)
        torch.cuda.synchronize()
        mean = A.mean(dim=(2, 3), keepdim=True)
        assert bool((mean > 0).all())
        assert torch.equal(F, (A / mean).mean(dim=0)), f"draws {draws}: SliderEditor.footprint and the hand-written loop differ"
        mask = footprint_mask(F.cpu())
        assert mask.shape == (1, HW, HW) and 0.0 <= float(mask.min()) and float(mask.max()) <= 1.0 and float(mask.max()) > 0.0
    Z = ed.footprint(sp, 0.0, start_noise=START)
    assert torch.equal(Z, torch.zeros_like(Z)), "scale 0: the slider-on passes are the slider-off passes"
    with pytest.raises(ValueError, match="no footprint"):
        footprint_mask(Z.cpu())
    with pytest.raises(ValueError):
        ed.footprint(sp, SCALE, start_noise=100)
    assert torch.equal(ed.edit_latents(sp, scale=0.0), sp.recon), "the editor is as it was after the footprints"


@pytest.mark.parametrize("form", ["sliders", "none"])
def test_footprint_on_merged_weights(dev, form):
    cfg, eng, ed = _editor("tiny_sd1", form, dev)
    ctx, pooled, x0 = _inputs(cfg, dev)
    snap = {k: v.clone() for k, v in eng.w.t.items()}
    sp = ed.invert(ctx, x0, steps=STEPS, skip=SKIP, guidance_scale=GS, seed=3)
    bare = NoiseSpace(**{**sp._map(lambda t: t), "visited": None})
    F = ed.footprint(bare, SCALE, start_noise=START)
    torch.cuda.synchronize()
    assert torch.equal(bare.visited, sp.visited), "a space without visited goes through trajectory"
    assert all(torch.equal(v, snap[k]) for k, v in eng.w.t.items()) and (ed.merger is None or not ed.merger.merged), "the weights are restored"
    assert torch.equal(F, ed.footprint(sp, SCALE, start_noise=START))
    if form == "sliders":
        assert bool(torch.isfinite(F).all()) and float(F.max()) > float(F.min()) and abs(float(F.mean()) - 1.0) <= 1e-5
        Z = ed.footprint(sp, 0.0, start_noise=START)
        assert torch.equal(Z, torch.zeros_like(Z))
    else:
        assert torch.equal(F, torch.zeros_like(F)), "no slider: no footprint"
    assert torch.equal(ed.edit_latents(sp, scale=0.0), sp.recon)


# ---------------------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------------------
def _pixels(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_cli_masks_on_synthetic_weights(dev, tmp_path, monkeypatch):
    from PIL import Image
    import sliders_amd.model_util as mu
    engines, real = {}, mu.synthetic_engine

    def one_engine(*a):                      # the five runs below build the same random UNet: build it once
        if a not in engines:
            engines[a] = real(*a)
        return engines[a]
    monkeypatch.setattr(mu, "synthetic_engine", one_engine)
    cfg = CONFIGS["sd1"]()
    img = str(tmp_path / "photo.png")
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (256, 256, 3), dtype=np.uint8)).save(img)
    slider = str(tmp_path / "age_alpha1.0_rank4_noxattn.pt")
    torch.save(drawn_slider(cfg, "noxattn", 4, 1.0, 41), slider)
    masks = {}
    half = np.zeros((256, 256), dtype=np.uint8)
    half[:, 128:] = 255
    for name, arr in (("half", half), ("black", np.zeros((64, 64), dtype=np.uint8)), ("white", np.full((64, 64), 255, dtype=np.uint8))):
        masks[name] = str(tmp_path / f"{name}.png")
        Image.fromarray(arr).save(masks[name])
    common = ["--model", "sd1", "--synthetic", "--lora_weight", slider, "--steps", "4", "--skip", "1", "--res", "256"]
    inv = str(tmp_path / "inversion.pt")
    plain = edit.main(common + ["--image", img, "--scales=0,1", "--save_inversion", inv, "--out", str(tmp_path / "plain")])
    recon = _pixels(os.path.join(plain, "recon.png"))
    assert NoiseSpace.load(inv).visited.shape == (3, 1, 4, 32, 32), "--save_inversion files carry visited"
    assert not np.array_equal(_pixels(os.path.join(plain, "scale_1.png")), recon)
    saved = str(tmp_path / "half_latent.png")
    out = edit.main(common + ["--inversion", inv, "--scales=0,1", "--mask", masks["half"], "--save_mask", saved, "--out", str(tmp_path / "half")])
    assert np.array_equal(_pixels(os.path.join(out, "scale_0.png")), _pixels(os.path.join(out, "recon.png"))), "--mask at scale 0 is the reconstruction"
    assert np.array_equal(_pixels(os.path.join(out, "recon.png")), recon)
    assert not np.array_equal(_pixels(os.path.join(out, "scale_1.png")), recon)
    want = np.zeros((32, 32), dtype=np.uint8)
    want[:, 16:] = 255
    assert np.array_equal(_pixels(saved), want)
    out = edit.main(common + ["--inversion", inv, "--scales=1", "--mask", masks["black"], "--out", str(tmp_path / "black")])
    assert np.array_equal(_pixels(os.path.join(out, "scale_1.png")), recon), "an all-black mask: every scale is the reconstruction"
    out = edit.main(common + ["--inversion", inv, "--scales=1", "--mask", masks["half"], "--mask_invert", "--mask_feather", "1", "--out", str(tmp_path / "inv")])
    assert not np.array_equal(_pixels(os.path.join(out, "scale_1.png")), _pixels(os.path.join(str(tmp_path / "half"), "scale_1.png")))
    out = edit.main(common + ["--inversion", inv, "--scales=1", "--mask", masks["white"], "--out", str(tmp_path / "white")])
    assert open(os.path.join(out, "scale_1.png"), "rb").read() == open(os.path.join(plain, "scale_1.png"), "rb").read(), "an all-white mask is the unmasked edit"
    auto = str(tmp_path / "auto.png")
    out = edit.main(common + ["--inversion", inv, "--scales=0,1", "--auto_mask", "--auto_mask_draws", "2", "--save_mask", auto, "--out", str(tmp_path / "auto")])
    m = _pixels(auto)
    assert m.shape == (32, 32) and m.dtype == np.uint8 and m.max() > 0
    assert np.array_equal(_pixels(os.path.join(out, "scale_0.png")), recon) and os.path.getsize(os.path.join(out, "scale_1.png")) > 0
    assert len(engines) == 1
