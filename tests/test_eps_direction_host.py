"""Prompt-direction sampling, host side (docs/SAMPLING.md, "Prompt-direction sampling"; no GPU):

1. the two C entry points are declared, exported, add no opcode, and refuse bad arguments before any launch;
2. the kernels' fp32 arithmetic stays within the derived bound of float64 (tests/eps_direction_ref.py);
3. six wrong kernels exceed it by a wide factor;
4. DirectionSet: from a prompts.yaml, its coefficients, n_keep;
5. python -m sliders_amd.generate refuses every bad combination of the direction options before a model is built.
"""
import ctypes as C
import os
import re

import pytest
import torch

from sliders_amd import generate, lib, prompt_util
from sliders_amd.directions import Direction, DirectionSet
from tests.eps_direction_ref import MUTANTS, kept, oracle_and_bound, restate, worst_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def draw_rows(cls, n, K, g):
    """(t, pos[K], neg[K]) flat bf16 [n]"""
    t = torch.randn(n, generator=g).to(BF)
    pos, neg = [], []
    for k in range(K):
        if cls == "ties":                # rows from {-1, 0, 1}: |d| in {0, 1, 2}, heavy ties at every threshold
            p, m = (torch.randint(-1, 2, (n,), generator=g).float() for _ in range(2))
        elif cls == "low_byte":          # |d| = 1 + j / 128: the keys differ in their low 7 bits only (the second radix pass)
            p = 1.0 + torch.randint(0, 128, (n,), generator=g).float() / 128.0
            m = torch.zeros(n)
        elif cls == "below_key":         # d = 256 - {0.25, 0.5, 0.75, 1}: exact fp32 differences in [255, 256), which differ below the key only
            p = torch.full((n,), 256.0)
            m = torch.randint(1, 5, (n,), generator=g).float() / 4.0
        elif cls == "equal":             # e+ == e-
            p = torch.randn(n, generator=g)
            m = p.clone()
        else:
            p, m = torch.randn(n, generator=g) * (k + 1.0), torch.randn(n, generator=g)
        pos.append(p.to(BF))
        neg.append(m.to(BF))
    return t, pos, neg


# ---------------------------------------------------------------------------------------------------------------------------
# 1. ABI
# ---------------------------------------------------------------------------------------------------------------------------
def _thr_call(ptrs, dims):
    return lib.load().slh_direction_threshold((C.c_void_p * 7)(*ptrs), (C.c_int32 * 7)(*dims), None, None)


def _dir_call(ptrs, dims, coef=(1.0, 1.0, 1.0)):
    return lib.load().slh_eps_direction((C.c_void_p * 9)(*ptrs), (C.c_int32 * 4)(*dims), (C.c_float * 3)(*coef) if coef is not None else None, None)


def test_abi_declared_exported_and_refusing_on_the_host():
    hdr = open(os.path.join(ROOT, "include", "sliders_hip.h")).read()
    for name in ("slh_direction_threshold", "slh_eps_direction"):
        assert re.search(rf"^int {name}\(const void\* const\* ptrs, const int32_t\* dims, const float\* coef, slh_stream_t stream\);", hdr, flags=re.M)
        assert name in lib.EXPORTS and hasattr(lib.load(), name)
    assert lib.load().slh_op_info(-1, None, None, None) == 41 == len(lib._ENTRY), "no new opcode"

    def refused(call, name, what, *a, **kw):
        assert call(*a, **kw) != 0
        msg = lib.last_error()
        assert name in msg and what in msg, msg

    # (addresses that are never dereferenced: every call below is refused before the launch)
    # slh_direction_threshold: pos[3], neg[3], thr; dims nb, chw, hw, K, n_keep[3]
    ok = [0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000]
    dims = [1, 64, 16, 3, 1, 16, 8]
    T = lambda what, p=ok, d=dims: refused(_thr_call, "slh_direction_threshold", what, p, d)
    for hole in range(7):
        T("null", [0 if k == hole else v for k, v in enumerate(ok)])
    assert _thr_call([0x1000, 0, 0, 0x4000, 0, 0, 0x7000], [1, 64, 16, 1, 17, 0, 0]) != 0 and "n_keep[0] = 17" in lib.last_error(), \
        "K = 1 reads one pair: the others may be null"
    for k, name in enumerate(("nb", "chw", "hw")):
        for bad in (0, -1):
            T(f"{name} = {bad}", d=[bad if j == k else v for j, v in enumerate(dims)])
    T("not a multiple of hw", d=[1, 64, 24, 3, 1, 1, 1])
    for bad in (0, 4, -1):
        T(f"K = {bad}", d=[1, 64, 16, bad, 1, 1, 1])
    for k in range(3):
        for bad in (0, 17, -1):
            T(f"n_keep[{k}] = {bad}", d=dims[:4] + [bad if j == k else 1 for j in range(3)])
    for k in range(6):
        T("not 2-byte aligned", [v + 1 if j == k else v for j, v in enumerate(ok)])
    T("not 4-byte aligned", ok[:6] + [0x7002])
    T("thr overlaps pos[1] / neg[1]", [0x1000, 0x2000, 0x3000, 0x4000, 0x2040, 0x6000, 0x2000 + 64 * 2 + 60])
    T("thr overlaps pos[0] / neg[0]", [0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x1000 - 8])

    # slh_eps_direction: t, out, pos[3], neg[3], thr; dims nb, chw, hw, K
    ok = [0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000]
    dims = [1, 64, 16, 3]
    D = lambda what, p=ok, d=dims, **kw: refused(_dir_call, "slh_eps_direction", what, p, d, **kw)
    for hole in range(8):
        D("null", [0 if k == hole else v for k, v in enumerate(ok)])
    D("null", coef=None)
    for k, name in enumerate(("nb", "chw", "hw")):
        for bad in (0, -1):
            D(f"{name} = {bad}", d=[bad if j == k else v for j, v in enumerate(dims)])
    D("not a multiple of hw", d=[1, 64, 24, 3])
    for bad in (0, 4, -1):
        D(f"K = {bad}", d=[1, 64, 16, bad])
    for k in range(3):
        for bad in (float("inf"), float("-inf"), float("nan")):
            D(f"c[{k}]", coef=[bad if j == k else 1.0 for j in range(3)])
    D("c[1]", coef=(0.0, float("nan"), 0.0))
    for k in range(8):
        D("not 2-byte aligned", [v + 1 if j == k else v for j, v in enumerate(ok)])
    D("not 4-byte aligned", ok[:8] + [0x9002])
    D("out overlaps t", [0x1000, 0x1000 + 126] + ok[2:])
    for k in range(3):
        D(f"out overlaps pos[{k}] / neg[{k}]", [0x1000, ok[2 + k] - 2] + ok[2:])
        D(f"out overlaps pos[{k}] / neg[{k}]", [0x1000, ok[5 + k] + 126] + ok[2:])
        D(f"out overlaps pos[{k}] / neg[{k}]", [0x1000, ok[5 + k] + 126] + ok[2:], coef=[0.0 if j == k else 1.0 for j in range(3)])
    D("out overlaps thr", [0x1000, 0x9000 + 44] + ok[2:])
    # the binding raises with the library's message
    with pytest.raises(lib.SlidersHipError, match="slh_eps_direction.*K = 0"):
        lib.eps_direction(0, t=0x1000, out=0x2000, pos=[], neg=[], c=[], nb=1, chw=64, hw=16)
    with pytest.raises(lib.SlidersHipError, match="at most 3"):
        lib.eps_direction(0, t=0x1000, out=0x2000, pos=[1] * 4, neg=[1] * 4, c=[1.0] * 4, nb=1, chw=64, hw=16)
    with pytest.raises(lib.SlidersHipError, match=r"n_keep\[0\] = 17"):
        lib.direction_threshold(0, pos=[0x1000], neg=[0x2000], thr=0x3000, n_keep=[17], nb=1, chw=64, hw=16)
    with pytest.raises(lib.SlidersHipError, match="2 n_keep values for 1 directions"):
        lib.direction_threshold(0, pos=[0x1000], neg=[0x2000], thr=0x3000, n_keep=[1, 1], nb=1, chw=64, hw=16)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. / 3. the arithmetic: bound and mutants
# ---------------------------------------------------------------------------------------------------------------------------
COEF = (0.75, -1.25, 0.5)


def _ratio(nb, chw, hw, K, n_keep, cls, seed, mutant=None, c=COEF, nan_in=None):
    g = torch.Generator().manual_seed(seed)
    t, pos, neg = draw_rows(cls, nb * chw, K, g)
    if nan_in is not None:
        pos[nan_in][::3] = float("nan")
        neg[nan_in][1::3] = float("nan")
    keep = None if n_keep is None else [n_keep] * K
    ref, bnd = oracle_and_bound(t, pos, neg, c[:K], keep, nb, chw, hw)
    got = restate(t, pos, neg, c[:K], keep, nb, chw, hw, mutant)
    return worst_ratio(got.float(), ref, 1.01 * bnd)


def test_fp32_restatement_stays_within_the_derived_bound():
    worst, where = 0.0, None
    seed = 0
    for nb in (1, 2):
        for chw, hw in ((4, 1), (140, 35), (4000, 1000)):
            for K in (1, 2, 3):
                for n_keep in sorted({1, min(2, hw), max(1, hw // 20), max(1, hw - 1), hw}) + [None]:
                    for cls in ("normal", "ties", "low_byte", "below_key", "equal"):
                        seed += 1
                        r = _ratio(nb, chw, hw, K, n_keep, cls, seed)
                        if r > worst:
                            worst, where = r, (nb, chw, hw, K, n_keep, cls)
    print(f"[bound] fp32 restatement, worst error / bound {worst:.3f} {where}")
    assert worst <= 1.0
    # a skipped term's NaN stays out, in the oracle as in the restatement
    assert _ratio(2, 4000, 1000, 3, 50, "normal", 5, c=(0.75, 0.0, 0.5), nan_in=1) <= 1.0


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_break_the_bound(mutant):
    """nb = 2, four channels of 1000 pixels, normal draws (direction k's positive row k + 1 times as wide, so the channels' and the
    directions' thresholds differ), 50 kept per channel; the NaN leak: c_1 = 0 over rows with NaN.  'wide': more than 100 x the bound"""
    kw = dict(c=(0.75, 0.0, 0.5), nan_in=1) if mutant == "zero_multiplied" else {}
    cls = "ties" if mutant == "strict_greater" else "normal"
    honest = _ratio(2, 4000, 1000, 3, 50, cls, 11, **kw)
    broken = _ratio(2, 4000, 1000, 3, 50, cls, 11, mutant=mutant, **kw)
    print(f"[mutant] {mutant}: honest {honest:.3f}, mutant {broken:.3e}")
    assert honest <= 1.0 and broken > 100.0


def test_the_kept_set_keeps_every_tie_and_at_least_n_keep():
    g = torch.Generator().manual_seed(3)
    nb, chw, hw = 2, 4000, 1000
    for cls, n_keep in (("ties", 50), ("ties", 999), ("normal", 1), ("below_key", 2), ("equal", 7), ("low_byte", 500)):
        _, pos, neg = draw_rows(cls, nb * chw, 1, g)
        keep, tau = kept(pos[0], neg[0], n_keep, nb, chw, hw)
        counts = keep.reshape(nb, chw // hw, hw).sum(2)
        assert bool((counts >= n_keep).all()) and tau.shape == (nb, 4)
        if cls in ("below_key", "equal"):        # one key: everything ties, everything is kept
            assert bool(keep.all()) and (cls != "equal" or bool((tau == 0).all()))
        if cls == "ties" and n_keep == 50:       # |d| = 2 about 222 times per channel: tau is 2's key and all of them are kept
            assert bool((tau == 0x4000).all()) and bool((counts > 150).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 4. DirectionSet
# ---------------------------------------------------------------------------------------------------------------------------
def test_direction_set_from_a_prompts_file():
    entries = prompt_util.load_prompts_from_yaml(os.path.join(ROOT, "tests", "golden", "prompts_sample.yaml"))
    seen = []

    def encode(text):
        seen.append(text)
        return torch.full((1, 77, 8), float(len(seen))), torch.full((1, 4), float(len(seen)))

    ds = DirectionSet.from_settings(entries, encode)
    assert seen == ["person, smiling", "person, frowning", "dog, fluffy", "dog, shaved"] and len(ds) == 2
    assert [(d.eta, d.sign) for d in ds.directions] == [(4.0, 1.0), (1.0, -1.0)], "enhance at eta 4; erase at the default guidance_scale"
    assert ds.coefficients(2.0, 8.0, single=False) == [1.0, -0.25] and ds.coefficients(2.0, 8.0, single=True) == [8.0, -2.0]
    assert ds.coefficients(0.0, 8.0, single=False) == [0.0, 0.0] and ds.coefficients(0.0, 0.0, single=False) == [0.0, 0.0]
    with pytest.raises(ValueError, match="guidance"):
        ds.coefficients(1.0, 0.0, single=False)
    ctx, pooled = ds.rows(2, "cpu")
    assert ctx.shape == (8, 77, 8) and pooled.shape == (8, 4)
    assert [float(ctx[r, 0, 0]) for r in range(8)] == [1, 1, 2, 2, 3, 3, 4, 4], "blocks e+_1, e-_1, e+_2, e-_2 of bs rows each"
    sw = ds.swapped()
    assert sw.directions[0].ctx_pos is ds.directions[0].ctx_neg and sw.coefficients(-2.0, 8.0, False) == [-1.0, 0.25]
    with pytest.raises(ValueError, match="1 to 3"):
        DirectionSet(ds.directions * 2)
    with pytest.raises(ValueError, match="1 to 3"):
        DirectionSet([])
    with pytest.raises(ValueError, match="sign"):
        DirectionSet([Direction(ctx, ctx, eta=1.0, sign=0.5)])


def test_n_keep():
    assert DirectionSet.n_keep(4096, 0.0) == 4096 and DirectionSet.n_keep(4096, 0.9) == 4096 - 3686 and DirectionSet.n_keep(1000, 0.95) == 50
    assert DirectionSet.n_keep(4096, 1.0 - 2.0 ** -30) == 1 and DirectionSet.n_keep(35, 0.999) == 1, "q -> 1: one entry stays"
    assert DirectionSet.n_keep(1, 0.0) == 1 and DirectionSet.n_keep(1, 0.99) == 1
    for bad in (1.0, -0.1, 2.0, float("nan")):
        with pytest.raises(ValueError, match="expected 0 <= q < 1"):
            DirectionSet.n_keep(64, bad)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the command line's argument errors
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,what", [
    (["--direction", "smiling"], "expected POSITIVE|NEGATIVE[:ETA]"),
    (["--direction", "a|b:x"], "expected POSITIVE|NEGATIVE[:ETA]"),
    (["--direction", "a|b:inf"], "expected a finite ETA"),
    (["--direction", "a|b"] * 4, "at most 3"),
    (["--direction", "a|b", "--direction_file", "tests/golden/prompts_sample.yaml"], "give one of them"),
    (["--direction_file", "no_such_file.yaml"], "no such file"),
    (["--direction_file", "tests/golden/prompts_sample.yaml", "--direction_entries", "0,2"], "entries 0 .. 1"),
    (["--direction_file", "tests/golden/prompts_sample.yaml", "--direction_entries", "a"], "expected comma-separated entry numbers"),
    (["--direction_entries", "0"], "--direction_entries needs --direction_file"),
    (["--direction_quantile", "0.5"], "--direction_quantile needs --direction"),
    (["--direction", "a|b", "--direction_quantile", "1"], "expected 0 <= q < 1"),
    (["--direction", "a|b", "--lora_weight", "x.pt"], "not with --lora_weight"),
    (["--direction", "a|b", "--guidance_scale", "0"], "--guidance_scale 0"),
    (["--direction", "a|b", "--mask_tokens", "3", "--scheduler", "euler"], "--fp32_latents"),
])
def test_cli_argument_errors_exit_before_a_model_is_built(monkeypatch, flags, what):
    import sliders_amd.model_util as mu

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(mu, "synthetic_engine", no_model)
    monkeypatch.setattr(torch, "load", no_model)
    monkeypatch.chdir(ROOT)
    with pytest.raises(SystemExit) as e:
        generate.main(["--synthetic"] + flags)
    assert what in str(e.value), e.value


def test_cli_direction_specs():
    P = lambda *argv: generate.build_parser().parse_args(list(argv))
    assert generate.direction_specs(P()) == []
    assert generate.direction_specs(P("--direction", "smiling person|frowning person:4", "--direction", "old|young")) == \
        [("smiling person", "frowning person", 4.0, 1.0), ("old", "young", 1.0, 1.0)]
    assert generate.direction_specs(P("--direction", "a: b|c")) == [("a: b", "c", 1.0, 1.0)], "the ETA follows the last colon of the negative"
    path = os.path.join(ROOT, "tests", "golden", "prompts_sample.yaml")
    assert generate.direction_specs(P("--direction_file", path)) == \
        [("person, smiling", "person, frowning", 4.0, 1.0), ("dog, fluffy", "dog, shaved", 1.0, -1.0)]
    assert generate.direction_specs(P("--direction_file", path, "--direction_entries", "1")) == [("dog, fluffy", "dog, shaved", 1.0, -1.0)]
    # --compose stays legal next to --direction, and the plain command line checks nothing new
    a = P("--direction", "a|b", "--compose", "x.pt:1", "--scales=0,1")
    assert generate.check_args(a) == [0.0, 1.0]
    assert generate.check_args(P("--negative_prompt", "blurry")) == [-2.0, -1.0, 0.0, 1.0, 2.0]
