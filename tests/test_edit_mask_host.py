"""CPU: localised slider edits (sliders_amd/edit.py, docs/EDIT.md "Localised edits") - the five identities of the masked edit in the
float32 reference over a toy network, the float32 blend against the float64 one within the derived bound, two mutants the identities
must catch, the mask helpers, NoiseSpace.visited on disk, the descriptor checks of slh_ddpm_edit_blend and slh_eps_absdiff, the CLI's
new argument errors.

Bound of one masked step against float64 on the same inputs, u = 2^-24 (docs/EDIT.md):
    |out - ref| <= m B_e + 4 u (|k| + m |e - k|),    B_e = 9 u (S_mu + |resid|) the mode-1 bound of the unmasked step
"""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

from sliders_amd import edit, lib
from sliders_amd.ddim import DDIMSchedule
from sliders_amd.edit import (NoiseSpace, blend_reference, ddpm_mu_reference, ddpm_step_coefficients, edit_reference, feather_mask,
                              footprint_mask, invert_reference, load_mask)
from tests.test_edit_host import toy_predict
from tests.test_host import library_ops

U = 2.0 ** -24
SHAPE = (2, 4, 9, 7)
STEPS, SKIP, GUIDANCE, START = 10, 2, 7.5, 500
SCALES = (2.0, -1.5)


def masks(shape=SHAPE, seed=0):
    bs, _, h, w = shape
    g = torch.Generator().manual_seed(seed)
    square = torch.zeros(h, w)
    square[2:6, 1:5] = 1.0
    return {"zeros": torch.zeros(bs, h, w), "ones": torch.ones(bs, 1, h, w), "binary": (torch.rand(bs, h, w, generator=g) < 0.5).float(),
            "uniform": torch.rand(bs, 1, h, w, generator=g), "feathered": feather_mask(square, 1.0)}


_spaces = {}


def space(prediction, eta):
    """one inversion per (prediction, eta), shared by the tests and never written to"""
    if (prediction, eta) not in _spaces:
        sch = DDIMSchedule(prediction_type=prediction)
        predict = toy_predict(3)
        x0 = torch.randn(SHAPE, generator=torch.Generator().manual_seed(17))
        _spaces[prediction, eta] = (sch, predict, invert_reference(predict, x0, sch, STEPS, SKIP, eta, guidance=GUIDANCE, seed=5))
    return _spaces[prediction, eta]


def full(mask):
    return edit.as_mask(mask, SHAPE[0], SHAPE[2], SHAPE[3]).expand(SHAPE)


CONFIGS = list(itertools.product(("epsilon", "v_prediction"), (0.0, 1.0)))


@pytest.mark.parametrize("prediction,eta", CONFIGS)
def test_the_inversion_keeps_its_latents(prediction, eta):
    sch, predict, sp = space(prediction, eta)
    assert sp.visited.shape == sp.resid.shape and sp.visited.dtype == torch.float32
    assert torch.equal(sp.visited[-1], sp.recon)
    assert torch.equal(edit_reference(predict, sp, sch, scale=0.0), sp.recon), "the unmasked edit is what it was"
    x = sp.x_start.clone()
    v = prediction == "v_prediction"
    for i, t in enumerate(sp.timesteps):                  # visited[i] is the latent the scale-0 chain has after step i
        eu, et = predict(x.to(torch.bfloat16), t, 0.0)
        x = ddpm_mu_reference(eu, et, x, ddpm_step_coefficients(sch, t, STEPS, eta), GUIDANCE, v, torch.float32) + sp.resid[i]
        assert torch.equal(x, sp.visited[i]), i


@pytest.mark.parametrize("prediction,eta", CONFIGS)
def test_identities_in_the_float32_reference(prediction, eta):
    sch, predict, sp = space(prediction, eta)
    ms = masks()
    for s in SCALES:
        plain = edit_reference(predict, sp, sch, scale=s, start_noise=START)
        assert not torch.equal(plain, sp.recon)
        # 1: all ones is the unmasked edit;  2: all zeros is the reconstruction
        assert torch.equal(edit_reference(predict, sp, sch, scale=s, start_noise=START, mask=ms["ones"]), plain), ("identity 1", s)
        assert torch.equal(edit_reference(predict, sp, sch, scale=s, start_noise=START, mask=ms["zeros"]), sp.recon), ("identity 2", s)
        # 4: a binary mask keeps the reconstruction's bits outside and edits inside
        for name in ("binary", "zeros", "ones"):
            out = edit_reference(predict, sp, sch, scale=s, start_noise=START, mask=ms[name])
            on = full(ms[name]) == 1
            assert torch.equal(out[~on], sp.recon[~on]), ("identity 4", name, s)
            assert name == "zeros" or not torch.equal(out[on], sp.recon[on]), ("the edit acts inside the mask", name, s)
        for name in ("uniform", "feathered"):
            out = edit_reference(predict, sp, sch, scale=s, start_noise=START, mask=ms[name])
            off = full(ms[name]) == 0
            assert bool(torch.isfinite(out).all()) and torch.equal(out[off], sp.recon[off]) and not torch.equal(out, sp.recon), (name, s)
    # 3: any mask at scale 0 is the reconstruction
    for name, m in ms.items():
        assert torch.equal(edit_reference(predict, sp, sch, scale=0.0, mask=m), sp.recon), ("identity 3", name)
        assert torch.equal(edit_reference(predict, sp, sch, scale=2.0, start_noise=-1, mask=m), sp.recon), ("the slider never switches on", name)
    # the three accepted shapes are one mask
    m3 = ms["binary"]
    want = edit_reference(predict, sp, sch, scale=2.0, start_noise=START, mask=m3)
    assert torch.equal(edit_reference(predict, sp, sch, scale=2.0, start_noise=START, mask=m3[:, None]), want)
    same = m3[0][None].expand(2, -1, -1)
    assert torch.equal(edit_reference(predict, sp, sch, scale=2.0, start_noise=START, mask=m3[0]),
                       edit_reference(predict, sp, sch, scale=2.0, start_noise=START, mask=same))


def test_identity_5_runs_files_and_trajectory(tmp_path):
    sch, predict, sp = space("epsilon", 1.0)
    m = masks()["feathered"]
    a = edit_reference(predict, sp, sch, scale=2.0, start_noise=START, mask=m)
    assert torch.equal(a, edit_reference(predict, sp, sch, scale=2.0, start_noise=START, mask=m)), "two runs"
    path = str(tmp_path / "space.pt")
    sp.save(path)
    back = NoiseSpace.load(path)
    assert back.visited.dtype == torch.float32 and torch.equal(back.visited, sp.visited)
    assert torch.equal(edit_reference(predict, back, sch, scale=2.0, start_noise=START, mask=m), a), "a saved and reloaded space"
    d = torch.load(path, map_location="cpu")
    del d["visited"]                                   # a file from before masked edits
    torch.save(d, path)
    old = NoiseSpace.load(path)
    assert old.visited is None and torch.equal(old.resid, sp.resid)
    assert torch.equal(edit_reference(predict, old, sch, scale=2.0, start_noise=START), edit_reference(predict, sp, sch, scale=2.0, start_noise=START))
    assert old.visited is None, "an unmasked edit needs no trajectory"
    assert edit.trajectory_reference(predict, old, sch) is old and torch.equal(old.visited, sp.visited), "trajectory gives the same latents back"
    old.visited = None
    assert torch.equal(edit_reference(predict, old, sch, scale=2.0, start_noise=START, mask=m), a) and torch.equal(old.visited, sp.visited)
    other = NoiseSpace.load(path)
    other.recon = other.recon + 1.0
    with pytest.raises(RuntimeError, match="recon"):
        edit.trajectory_reference(predict, other, sch)
    del d["resid"]
    torch.save(d, path)
    with pytest.raises(KeyError):
        NoiseSpace.load(path)


def test_mask_argument_errors():
    sch, predict, sp = space("epsilon", 1.0)
    bs, _, h, w = SHAPE
    bad = {"values above 1": torch.full((h, w), 1.5), "negative values": torch.full((bs, h, w), -0.1), "nan": torch.full((h, w), float("nan")),
           "transposed": torch.ones(w, h), "a channel dimension": torch.ones(bs, 4, h, w), "another batch": torch.ones(bs + 1, h, w),
           "five dimensions": torch.ones(1, bs, 1, h, w), "integers": torch.ones(h, w, dtype=torch.int64), "a list": [[1.0] * w] * h}
    for name, m in bad.items():
        with pytest.raises(ValueError):
            edit_reference(predict, sp, sch, scale=1.0, mask=m)
        with pytest.raises(ValueError):
            edit.as_mask(m, bs, h, w)
    ok = edit.as_mask(torch.ones(h, w, dtype=torch.bool), bs, h, w)
    assert ok.shape == (bs, 1, h, w) and ok.dtype == torch.float32 and ok.is_contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# the blend against float64, per step on the same inputs; exact ends
# ---------------------------------------------------------------------------------------------------------------------------------
def s_mu(f, ax, E, v):
    if v:
        return f["c_sqrt_alpha_prev"] * (f["c_sqrt_alpha_t"] * ax + f["c_sqrt_beta_t"] * E) + f["c_dir"] * (f["c_sqrt_alpha_t"] * E + f["c_sqrt_beta_t"] * ax)
    return f["c_sqrt_alpha_prev"] * f["c_inv_sqrt_alpha_t"] * (ax + f["c_sqrt_beta_t"] * E) + f["c_dir"] * E


def blend_bound(f, eu, et, x, resid, keep, m, e64, guidance, v):
    """m B_e + 4 u (|k| + m |e - k|), every term in float64 on the inputs"""
    E = eu.double().abs() + guidance * (et.double().abs() + eu.double().abs())
    B_e = 9 * U * (s_mu(f, x.double().abs(), E, v) + resid.double().abs())
    m, k = m.double(), keep.double()
    return m * B_e + 4 * U * (k.abs() + m * (e64 - k).abs())


@pytest.mark.parametrize("prediction,eta", CONFIGS)
def test_float32_reference_within_the_blend_bound_of_float64_at_every_step(prediction, eta):
    """the float32 masked chain; at every step float32 and float64 take that step from the chain's own fp32 inputs"""
    sch, predict, sp = space(prediction, eta)
    v = prediction == "v_prediction"
    worst = 0.0
    for name in ("uniform", "feathered", "binary"):
        m = edit.as_mask(masks()[name], SHAPE[0], SHAPE[2], SHAPE[3])
        x = sp.x_start.clone()
        for i, t in enumerate(sp.timesteps):
            eu, et = predict(x.to(torch.bfloat16), t, 0.0 if t > START else 2.0)
            coef = ddpm_step_coefficients(sch, t, STEPS, eta)
            e32 = ddpm_mu_reference(eu, et, x, coef, GUIDANCE, v, torch.float32) + sp.resid[i]
            e64 = ddpm_mu_reference(eu, et, x, coef, GUIDANCE, v, torch.float64) + sp.resid[i].double()
            got = blend_reference(e32, sp.visited[i], m, torch.float32)
            want = blend_reference(e64, sp.visited[i], m, torch.float64)
            assert got.dtype == torch.float32 and want.dtype == torch.float64
            bound = blend_bound(edit.fp32_coefficients(coef), eu, et, x, sp.resid[i], sp.visited[i], m.expand(SHAPE), e64, GUIDANCE, v)
            err = (got.double() - want).abs()
            assert bool((err <= bound).all()), (name, i, float((err / bound.clamp_min(1e-300)).max()))
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            x = got
        assert torch.equal(x, edit_reference(predict, sp, sch, scale=2.0, start_noise=START, mask=m)), "the loop above is edit_reference"
    print(f"[edit-mask] {prediction} eta {eta}: worst |fp32 - fp64| / bound over the masked steps {worst:.3f}")


def test_blend_reference_ends_are_exact_and_the_middle_is_within_4u():
    g = torch.Generator().manual_seed(2)
    worst = 0.0
    for big in (1e-3, 1.0, 1e3):
        e = torch.randn(1, 4, 64, 64, generator=g) * big
        k = torch.where(torch.rand(e.shape, generator=g) < 0.5, e * (1 + 2.0 ** -20 * torch.randn(e.shape, generator=g)), torch.randn(e.shape, generator=g) * big)
        m = torch.rand(1, 1, 64, 64, generator=g)
        m[0, 0, 0], m[0, 0, 1], m[0, 0, 2] = 0.0, 1.0, 2.0 ** -20
        out = blend_reference(e, k, m, torch.float32)
        assert torch.equal(out[..., 0, :], k[..., 0, :]) and torch.equal(out[..., 1, :], e[..., 1, :])
        assert torch.equal(blend_reference(k, k, m, torch.float32), k), "e == keep: keep under any mask"
        ref = blend_reference(e, k, m, torch.float64)
        bound = 4 * U * (k.double().abs() + m.double() * (e.double() - k.double()).abs())
        err = (out.double() - ref).abs()
        assert bool((err <= bound).all())
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    print(f"[edit-mask] blend alone: worst error / 4u term {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# mutants: the identities can see the bugs the design avoids
# ---------------------------------------------------------------------------------------------------------------------------------
def masked_edit(predict, sp, sch, scale, mask, keep_of, blend):
    """edit_reference's masked loop with the source of `keep` and the blend passed in"""
    v = sch.prediction_type == "v_prediction"
    m = edit.as_mask(mask, SHAPE[0], SHAPE[2], SHAPE[3])
    x = sp.x_start.clone()
    for i, t in enumerate(sp.timesteps):
        eu, et = predict(x.to(torch.bfloat16), t, 0.0 if t > START else float(scale))
        e = ddpm_mu_reference(eu, et, x, ddpm_step_coefficients(sch, t, sp.steps, sp.eta), sp.guidance, v, torch.float32) + sp.resid[i]
        x = blend(e, keep_of(i), m)
    return x


def test_mutants_break_identity_3():
    sch, predict, sp = space("epsilon", 1.0)
    path = edit.build_path(sch, sp.x0, sp.timesteps, sp.seed)
    visited = lambda i: sp.visited[i]
    target = lambda i: path[i + 1] if i + 1 < len(sp.timesteps) else sp.x0          # the constructed target, one rounding off the latent
    good = lambda e, k, m: blend_reference(e, k, m, torch.float32)
    lerp = lambda e, k, m: m * e + (1.0 - m) * k                                     # the textbook blend: does not return k where e == k
    ms = masks()
    for name in ("uniform", "feathered", "binary"):
        assert torch.equal(masked_edit(predict, sp, sch, 0.0, ms[name], visited, good), sp.recon), name
        assert torch.equal(masked_edit(predict, sp, sch, 2.0, ms[name], visited, good),
                           edit_reference(predict, sp, sch, scale=2.0, start_noise=START, mask=ms[name])), name
        assert not torch.equal(masked_edit(predict, sp, sch, 0.0, ms[name], target, good), sp.recon), f"keep = the constructed path, {name} mask"
    for name in ("uniform", "feathered"):
        assert not torch.equal(masked_edit(predict, sp, sch, 0.0, ms[name], visited, lerp), sp.recon), f"m e + (1 - m) k, {name} mask"


# ---------------------------------------------------------------------------------------------------------------------------------
# mask helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_load_mask(tmp_path):
    from PIL import Image
    img = np.zeros((64, 64), dtype=np.uint8)
    img[16:40, 20:48] = 255                     # rows 16..39: latent rows 2..4; columns 20..47: latent columns 2 (half), 3, 4, 5
    path = str(tmp_path / "mask.png")
    Image.fromarray(img).save(path)
    m = load_mask(path, 64)
    assert m.shape == (8, 8) and m.dtype == torch.float32
    want = torch.zeros(8, 8)
    want[2:5, 3:6] = 1.0
    want[2:5, 2] = 0.5
    assert torch.equal(m, want)
    assert torch.equal(load_mask(path, 64, invert=True), 1.0 - want)
    big = load_mask(path, 128)                   # resized: the same square on a 16 x 16 grid
    assert big.shape == (16, 16) and torch.equal(big[4:10, 5:12], torch.ones(6, 7)) and float(big[:4].abs().max()) == 0.0
    Image.fromarray(np.stack([img] * 3, -1)).save(path)          # an RGB file is read through its grey levels
    assert torch.equal(load_mask(path, 64), want)
    with pytest.raises(ValueError):
        load_mask(path, 60)


def test_feather_mask():
    g = torch.Generator().manual_seed(0)
    m = torch.rand(2, 12, 10, generator=g)
    assert feather_mask(m, 0) is m and torch.equal(feather_mask(m, 0.0), m)
    for sigma in (0.5, 1.0, 2.0):
        f = feather_mask(m, sigma)
        assert f.shape == m.shape and f.dtype == torch.float32 and float(f.min()) >= 0.0 and float(f.max()) <= 1.0
    sq = torch.zeros(24, 24)
    sq[6:18, 6:18] = 1.0
    f = feather_mask(sq, 1.0)                                      # radius 3
    assert torch.equal(f[9:15, 9:15], torch.ones(6, 6)) or float((f[9:15, 9:15] - 1.0).abs().max()) <= 4 * 2.0 ** -24, "an interior constant region keeps its value"
    assert float(f[:3].abs().max()) == 0.0 and 0.0 < float(f[5, 12]) < 0.5 < float(f[6, 12]) < 1.0
    assert abs(float(f.sum()) - 144.0) <= 1e-3, "the taps sum to 1: away from the border the mass is preserved"
    const = torch.full((1, 1, 8, 8), 0.75)
    assert float((feather_mask(const, 1.5) - 0.75).abs().max()) <= 4 * 2.0 ** -24, "replicate padding: a constant stays constant up to the border"
    assert feather_mask(torch.ones(1, 1, 8, 8), 3.0).shape == (1, 1, 8, 8)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            feather_mask(sq, bad)


def test_footprint_mask():
    F = torch.full((2, 16, 16), 0.1)
    F[0, 5:9, 6:10] = 3.0
    F[1, 2:6, 9:13] = 2.0
    for dilate, sigma in ((1, 1.0), (1, 0.0), (0, 0.0), (2, 0.5)):
        m = footprint_mask(F, dilate=dilate, feather=sigma)
        assert m.shape == F.shape and m.dtype == torch.float32 and float(m.min()) >= 0.0 and float(m.max()) <= 1.0
        reach = dilate + int(math.ceil(3 * sigma)) + 1
        for b, (r0, c0) in enumerate(((5, 6), (2, 9))):
            on = torch.zeros(16, 16, dtype=torch.bool)
            on[max(r0 - dilate, 0):r0 + 4 + dilate, max(c0 - dilate, 0):c0 + 4 + dilate] = True
            ii, jj = torch.meshgrid(torch.arange(16), torch.arange(16), indexing="ij")
            dist = torch.maximum(torch.clamp(torch.maximum(r0 - ii, ii - (r0 + 3)), min=0), torch.clamp(torch.maximum(c0 - jj, jj - (c0 + 3)), min=0))
            far = dist >= reach
            assert bool(far.any()) and float(m[b][far].abs().max()) == 0.0, (dilate, sigma, b)
            if sigma == 0.0:
                assert torch.equal(m[b], on.float())
            else:
                # the square lies `dilate` inside the binary region: where that covers the blur's radius it stays 1, up to the rounding
                # of the 2 x (2r + 1) <= 14 fp32 taps that sum to 1 (2^-20 is ample); else it is a blurred edge above 1/2
                lo = float(m[b][dist == 0].min())
                assert (lo >= 1.0 - 2.0 ** -20) if dilate >= int(math.ceil(3 * sigma)) else (0.5 < lo <= 1.0), (dilate, sigma, b, lo)
    m = footprint_mask(F[0], dilate=1, feather=0.0)
    assert m.shape == (16, 16) and torch.equal(m, footprint_mask(F, dilate=1, feather=0.0)[0])
    with pytest.raises(ValueError, match="no footprint"):
        footprint_mask(torch.zeros(1, 16, 16))
    with pytest.raises(ValueError, match="no footprint"):
        footprint_mask(torch.stack([F[0], torch.zeros(16, 16)]))
    for kw in (dict(quantile=0.0), dict(quantile=1.5), dict(threshold=0.0), dict(dilate=-1)):
        with pytest.raises(ValueError):
            footprint_mask(F, **kw)


def test_footprint_draws_and_mean():
    ts = edit.edit_timesteps(DDIMSchedule(), 50, 18)                # 620, 600, ..., 0
    assert edit.footprint_draws(ts, 750, 8, 200) == [0, 3, 6, 9, 12, 15, 18, 21] and ts[21] == 200
    assert edit.footprint_draws(ts, 500, 4, 200) == [6, 11, 16, 21]
    assert edit.footprint_draws(ts, 750, 100, 200) == list(range(22)), "fewer eligible steps than draws: all of them"
    assert edit.footprint_draws([625, 500, 375, 250, 125, 0], 500, 8, 200) == [1, 2, 3]
    assert edit.footprint_draws(ts, 750, 1, 200) == [0]
    with pytest.raises(ValueError):
        edit.footprint_draws(ts, 100, 8, 200)
    with pytest.raises(ValueError):
        edit.footprint_draws(ts, 750, 0, 200)
    A = torch.rand(3, 2, 4, 5, generator=torch.Generator().manual_seed(0))
    A[1, 0] = 0.0                                                   # a draw without any difference contributes 0 to that sample
    F = edit.footprint_mean(A)
    assert F.shape == (2, 4, 5) and torch.allclose(F[1].mean(), torch.tensor(1.0), atol=1e-6) and torch.allclose(F[0].mean(), torch.tensor(2.0 / 3.0), atol=1e-6)
    assert torch.equal(edit.footprint_mean(torch.zeros(3, 2, 4, 5)), torch.zeros(2, 4, 5))


# ---------------------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def _refused(l, opcode, entry, desc_type, full, bad):
    fn = getattr(l, entry)
    for name, change in bad.items():
        d = desc_type(**{**full, **change})
        assert fn(ctypes.byref(d), None) != 0, name
        assert entry.encode() in l.slh_last_error(), (name, l.slh_last_error())
        with pytest.raises(lib.SlidersHipError, match=entry):
            lib.call(opcode, d, 0)
        prog = lib.Program()
        prog.add(opcode, d, entry)
        with pytest.raises(lib.SlidersHipError, match=entry):
            prog.run(0)
    assert fn(None, None) != 0 and entry.encode() in l.slh_last_error()


def test_ddpm_edit_blend_refuses_bad_descriptors_before_any_launch():
    l = lib.load()
    assert lib.OP_DDPM_EDIT == 39 and lib.OP_DDPM_EDIT_BLEND == 40
    assert lib._ENTRY[lib.OP_DDPM_EDIT_BLEND] == ("slh_ddpm_edit_blend", lib.DdpmEditBlendDesc)
    assert ctypes.sizeof(lib.DdpmEditBlendDesc) == 9 * 8 + 3 * 4 + 6 * 4 + 4 == 112
    assert ctypes.sizeof(lib.DdpmEditDesc) == 104, "slh_ddpm_edit_desc is what it was"
    ops = library_ops()                             # the library's own table lists the three ops of the edit under their opcodes
    assert (ops[39], ops[40], ops[41]) == (("slh_ddpm_edit_step", 104), ("slh_ddpm_edit_blend", 112), ("slh_eps_absdiff", 56))
    # never dereferenced: every case is refused on the host.  nb * chw * 4 = 256 bytes per fp32 buffer, the buffers 0x1000 apart
    full = dict(eps=0x1000, x=0x2000, resid=0x3000, keep=0x4000, mask=0x5000, out=0x6000, out_bf16=0x7000, out2_bf16=0x8000, nb=1, chw=64, hw=16,
                guidance=7.5, c_sqrt_beta_t=0.5, c_inv_sqrt_alpha_t=1.2, c_sqrt_alpha_t=0.8, c_sqrt_alpha_prev=0.9, c_dir=0.3)
    bad = {"no eps": dict(eps=0), "no x": dict(x=0), "no resid": dict(resid=0), "no out": dict(out=0), "no keep": dict(keep=0), "no mask": dict(mask=0),
           "nb 0": dict(nb=0), "nb < 0": dict(nb=-1), "chw 0": dict(chw=0), "hw 0": dict(hw=0), "hw < 0": dict(hw=-16),
           "chw no multiple of hw": dict(hw=24), "hw > chw": dict(hw=128), "2^31 elements": dict(nb=32768, chw=65536, hw=65536),
           "keep is out": dict(keep=0x6000), "keep overlaps the end of out": dict(keep=0x6000 + 252), "out overlaps the end of keep": dict(out=0x4000 + 128),
           "mask is out": dict(mask=0x6000), "mask inside out": dict(mask=0x6000 + 192), "keep is out is x": dict(keep=0x2000, out=0x2000)}
    _refused(l, lib.OP_DDPM_EDIT_BLEND, "slh_ddpm_edit_blend", lib.DdpmEditBlendDesc, full, bad)
    # the executor checks the record's size
    prog = lib.Program()
    prog.add(lib.OP_DDPM_EDIT_BLEND, lib.DdpmEditDesc(eps=0x1000, x=0x2000, resid=0x3000, out=0x6000, nb=1, chw=64, mode=1), "wrong descriptor")
    with pytest.raises(lib.SlidersHipError, match="ddpm_edit_blend descriptor is 104 bytes"):
        prog.run(0)


def test_eps_absdiff_refuses_bad_descriptors_before_any_launch():
    l = lib.load()
    assert lib.OP_EPS_ABSDIFF == 41 and lib._ENTRY[lib.OP_EPS_ABSDIFF] == ("slh_eps_absdiff", lib.EpsAbsdiffDesc)
    assert ctypes.sizeof(lib.EpsAbsdiffDesc) == 5 * 8 + 3 * 4 + 4 == 56
    full = dict(eps_a=0x1000, eps_a_text=0x2000, eps_b=0x3000, eps_b_text=0x4000, out=0x5000, nb=2, chw=64, hw=16, guidance=7.5)
    bad = {"no eps_a": dict(eps_a=0), "no eps_b": dict(eps_b=0), "no out": dict(out=0), "nb 0": dict(nb=0), "nb < 0": dict(nb=-2), "chw 0": dict(chw=0),
           "hw 0": dict(hw=0), "hw < 0": dict(hw=-1), "chw no multiple of hw": dict(hw=48), "hw > chw": dict(hw=128), "2^31 elements": dict(nb=32768, chw=65536, hw=65536)}
    _refused(l, lib.OP_EPS_ABSDIFF, "slh_eps_absdiff", lib.EpsAbsdiffDesc, full, bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [
    ["--mask", "MASK", "--auto_mask", "--lora_weight", "a_alpha1.0_rank4_noxattn.pt"],
    ["--mask", "no_such_file.png"],
    ["--mask_invert"],
    ["--mask_invert", "--auto_mask", "--lora_weight", "a_alpha1.0_rank4_noxattn.pt"],
    ["--mask_feather", "1.0"],
    ["--save_mask", "m.png"],
    ["--mask", "MASK", "--mask_feather", "-1"],
    ["--mask", "MASK", "--mask_feather", "nan"],
    ["--mask", "MASK", "--auto_mask_scale", "2"],
    ["--auto_mask_draws", "4"],
    ["--auto_mask_threshold", "0.5"],
    ["--auto_mask_dilate", "1"],
    ["--auto_mask"],                                                                              # no slider: no footprint
    ["--auto_mask", "--lora_weight", "a_alpha1.0_rank4_noxattn.pt", "--scales", "0"],
    ["--auto_mask", "--lora_weight", "a_alpha1.0_rank4_noxattn.pt", "--auto_mask_scale", "0"],
    ["--auto_mask", "--lora_weight", "a_alpha1.0_rank4_noxattn.pt", "--auto_mask_draws", "0"],
    ["--auto_mask", "--lora_weight", "a_alpha1.0_rank4_noxattn.pt", "--auto_mask_threshold", "0"],
    ["--auto_mask", "--lora_weight", "a_alpha1.0_rank4_noxattn.pt", "--auto_mask_threshold", "1.5"],
    ["--auto_mask", "--lora_weight", "a_alpha1.0_rank4_noxattn.pt", "--auto_mask_dilate", "-1"],
    ["--auto_mask", "--lora_weight", "a_alpha1.0_rank4_noxattn.pt", "--start_noise", "100"],    # no step between t_min and start_noise
])
def test_cli_mask_argument_errors_exit_before_any_model_is_built(monkeypatch, tmp_path, argv):
    from PIL import Image

    def boom(*a, **k):
        raise AssertionError("an argument error must not reach CUDA, a model or a slider file")
    monkeypatch.setattr(torch.cuda, "_lazy_init", boom)
    monkeypatch.setattr(torch, "load", boom)
    import sliders_amd.model_util as mu
    monkeypatch.setattr(mu, "synthetic_engine", boom)
    monkeypatch.setattr(mu, "load_unet_engine", boom)
    mask = str(tmp_path / "mask.png")
    Image.fromarray(np.full((32, 32), 255, dtype=np.uint8)).save(mask)
    argv = [mask if a == "MASK" else a for a in argv]
    with pytest.raises(SystemExit) as e:
        edit.main(["--model", "sd1", "--synthetic", "--image", "x.png"] + argv)
    assert e.value.code not in (0, None)


def test_cli_mask_arguments_that_pass_the_checks(tmp_path):
    from PIL import Image
    mask = str(tmp_path / "mask.png")
    Image.fromarray(np.full((32, 32), 255, dtype=np.uint8)).save(mask)
    base = ["--model", "sd1", "--synthetic", "--image", "x.png"]
    a = edit.build_parser().parse_args(base + ["--mask", mask, "--mask_invert", "--mask_feather", "1.5", "--save_mask", "m.png"])
    assert edit.check_args(a) == [-2.0, -1.0, 0.0, 1.0, 2.0] and a.mask_feather == 1.5
    a = edit.build_parser().parse_args(base + ["--mask", mask])
    edit.check_args(a)
    assert a.mask_feather is None, "no feathering unless asked for"
    a = edit.build_parser().parse_args(base + ["--auto_mask", "--lora_weight", "s.pt", "--scales=-3,0,2"])
    edit.check_args(a)
    assert a.auto_mask_scale == -3.0, "the largest |scale| of --scales"
    a = edit.build_parser().parse_args(base + ["--auto_mask", "--compose", "s.pt:1", "--auto_mask_scale", "1.5", "--auto_mask_draws", "3",
                                               "--auto_mask_threshold", "0.4", "--auto_mask_dilate", "0", "--mask_feather", "0"])
    edit.check_args(a)
    assert (a.auto_mask_scale, a.auto_mask_draws, a.auto_mask_threshold, a.auto_mask_dilate, a.mask_feather) == (1.5, 3, 0.4, 0, 0.0)
