"""slh_eps_direction_momentum and the momentum / direction options above it, host side (docs/SAMPLING.md, "Prompt-direction sampling";
docs/EDIT.md, "Prompt-direction edits"; no GPU):

1. the C entry point is declared, exported, adds no opcode, and refuses bad arguments before any launch;
2. the kernel's fp32 arithmetic stays within the derived bound of float64 (tests/eps_momentum_ref.py);
3. six wrong kernels exceed it by a wide factor;
4. DirectionGuide's momentum validation;
5. python -m sliders_amd.generate / .edit refuse every bad combination of the new options before a model is built, and --auto_mask
   takes a direction in place of a slider.
"""
import ctypes as C
import itertools
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

from sliders_amd import edit, generate, lib
from sliders_amd.directions import Direction, DirectionGuide, DirectionSet, check_momentum
from tests.eps_momentum_ref import MUTANTS, f32, omb_of, oracle_and_bound, restate, worst_ratio
from tests.test_eps_direction_host import COEF, draw_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "slh_eps_direction_momentum"
MOMENTA = ((0.5, 0.4), (-1.25, 0.0), (2.0, 0.9))          # (s_m, beta)


def draw_nu(cls, n, g):
    """the state: zero, of the terms' size, or 100 x larger"""
    return torch.zeros(n) if cls == "zero" else torch.randn(n, generator=g) * (100.0 if cls == "big" else 1.0)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. ABI
# ---------------------------------------------------------------------------------------------------------------------------
def _call(ptrs, dims, coef=(1.0, 1.0, 1.0, 0.5, 0.4, 0.6)):
    return lib.load().slh_eps_direction_momentum((C.c_void_p * 11)(*ptrs), (C.c_int32 * 4)(*dims),
                                                 (C.c_float * 6)(*coef) if coef is not None else None, None)


def test_abi_declared_exported_and_refusing_on_the_host():
    hdr = open(os.path.join(ROOT, "include", "sliders_hip.h")).read()
    assert re.search(rf"^int {NAME}\(const void\* const\* ptrs, const int32_t\* dims, const float\* coef, slh_stream_t stream\);", hdr, flags=re.M)
    assert NAME in lib.EXPORTS and hasattr(lib.load(), NAME)
    assert lib.load().slh_op_info(-1, None, None, None) == 41 == len(lib._ENTRY), "no new opcode"

    # (addresses that are never dereferenced: every call below is refused before the launch)
    # t, out, pos[3], neg[3], thr, mom_in, mom_out; dims nb, chw, hw, K: bf16 rows of 128 bytes, thr of 48, fp32 rows of 256
    ok = [0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000, 0xA000, 0xB000]
    dims = [1, 64, 16, 3]
    good = (1.0, 1.0, 1.0, 0.5, 0.4, 0.6)

    def D(what, p=ok, d=dims, coef=good):
        assert _call(p, d, coef) != 0
        msg = lib.last_error()
        assert msg.startswith(NAME + ":") and what in msg, (what, msg)

    def at(k, v):
        return [v if j == k else x for j, x in enumerate(ok)]

    # everything slh_eps_direction refuses
    for hole in range(8):
        D("null", at(hole, 0))
    D("null", coef=None)
    for k, name in enumerate(("nb", "chw", "hw")):
        for bad in (0, -1):
            D(f"{name} = {bad}", d=[bad if j == k else v for j, v in enumerate(dims)])
    D("not a multiple of hw", d=[1, 64, 24, 3])
    for bad in (0, 4, -1):
        D(f"K = {bad}", d=[1, 64, 16, bad])
    for k in range(3):
        for bad in (float("inf"), float("-inf"), float("nan")):
            D(f"c[{k}]", coef=tuple(bad if j == k else v for j, v in enumerate(good)))
    D("c[1]", coef=(0.0, float("nan"), 0.0, 0.5, 0.4, 0.6))
    for k in range(8):
        D("not 2-byte aligned", at(k, ok[k] + 1))
    D("thr pointer", at(8, 0x9002))
    D("out overlaps t", at(1, 0x1000 + 126))
    for k in range(3):
        D(f"out overlaps pos[{k}] / neg[{k}]", at(1, ok[2 + k] - 2))
        D(f"out overlaps pos[{k}] / neg[{k}]", at(1, ok[5 + k] + 126))
        D(f"out overlaps pos[{k}] / neg[{k}]", at(1, ok[5 + k] + 126), coef=tuple(0.0 if j == k else v for j, v in enumerate(good)))
    D("out overlaps thr", at(1, 0x9000 + 44))
    # the state
    D("null mom_in / mom_out", at(9, 0))
    D("null mom_in / mom_out", at(10, 0))
    for k in (9, 10):
        for off in (1, 2, 3):
            D("fp32 pointer", at(k, ok[k] + off))
            D("not 4-byte aligned", at(k, ok[k] + off))
    for k, name in ((3, "s_m"), (4, "beta"), (5, "omb")):
        for bad in (float("inf"), float("-inf"), float("nan")):
            D("not finite", coef=tuple(bad if j == k else v for j, v in enumerate(good)))
            assert f"{name} = " in lib.last_error()
    for zero in (0.0, -0.0):
        D("s_m == 0", coef=(1.0, 1.0, 1.0, zero, 0.4, 0.6))
        assert "call slh_eps_direction " in lib.last_error(), "momentum off is the other entry point"
    D("mom_out overlaps mom_in", at(10, 0xA000 + 252))
    D("mom_out overlaps mom_in", at(10, 0xA000 - 252))
    D("mom_out overlaps t", at(10, 0x1000 + 124))
    D("mom_out overlaps t", at(10, 0x1000 - 252))
    for k in range(3):
        D(f"mom_out overlaps pos[{k}] / neg[{k}]", at(10, ok[2 + k] + 124))
        D(f"mom_out overlaps pos[{k}] / neg[{k}]", at(10, ok[5 + k] - 252))
        D(f"mom_out overlaps pos[{k}] / neg[{k}]", at(10, ok[5 + k] - 252), coef=tuple(0.0 if j == k else v for j, v in enumerate(good)))
    D("mom_out overlaps thr", at(10, 0x9000 + 44))
    D("out overlaps mom_in", at(1, 0xA000 + 254))
    D("out overlaps mom_in", at(1, 0xA000 - 126))
    D("out overlaps mom_out", at(1, 0xB000 + 254))
    D("out overlaps mom_out", at(1, 0xB000 - 126))
    # mom_out == mom_in exactly is not an overlap: the call gets past that check and is refused for the next reason
    alias = at(10, 0xA000)
    alias[1] = 0xA000 + 128
    D("out overlaps mom_in", alias)
    # the binding raises with the library's message, and forms omb itself
    with pytest.raises(lib.SlidersHipError, match=NAME + ".*s_m == 0"):
        lib.eps_direction_momentum(0, t=0x1000, out=0x2000, pos=[0x3000], neg=[0x6000], c=[1.0], mom_in=0xA000, mom_out=0xA000, s_m=0.0, beta=0.4,
                                   nb=1, chw=64, hw=16)
    with pytest.raises(lib.SlidersHipError, match="2 coefficients for 1 directions"):
        lib.eps_direction_momentum(0, t=0x1000, out=0x2000, pos=[0x3000], neg=[0x6000], c=[1.0, 1.0], mom_in=0xA000, mom_out=0xA000, s_m=1.0,
                                   beta=0.4, nb=1, chw=64, hw=16)
    with pytest.raises(lib.SlidersHipError, match="at most 3"):
        lib.eps_direction_momentum(0, t=0x1000, out=0x2000, pos=[1] * 4, neg=[1] * 4, c=[1.0] * 4, mom_in=0xA000, mom_out=0xA000, s_m=1.0,
                                   beta=0.4, nb=1, chw=64, hw=16)
    for beta in (0.4, 0.1, 1.0 - 2.0 ** -12 + 2.0 ** -26):
        assert C.c_float(lib.one_minus(beta)).value == omb_of(beta), "1 - beta in double, rounded once"
    assert omb_of(1.0 - 2.0 ** -12 + 2.0 ** -26) != f32(1.0 - f32(1.0 - 2.0 ** -12 + 2.0 ** -26)), "not the fp32 subtraction of the rounded beta"


# ---------------------------------------------------------------------------------------------------------------------------
# 2. / 3. the arithmetic: bound and mutants
# ---------------------------------------------------------------------------------------------------------------------------
def _ratios(nb, chw, hw, K, n_keep, cls, nu_cls, seed, mutant=None, c=COEF, nan_in=None, momentum=MOMENTA[0], coef3=None):
    """(worst error / (1.01 x bound) of out, of nu')"""
    g = torch.Generator().manual_seed(seed)
    t, pos, neg = draw_rows(cls, nb * chw, K, g)
    nu = draw_nu(nu_cls, nb * chw, g)
    if nan_in is not None:
        pos[nan_in][::3] = float("nan")
        neg[nan_in][1::3] = float("nan")
    keep = None if n_keep is None else [n_keep] * K
    s_m, beta, omb = coef3 if coef3 is not None else (momentum[0], momentum[1], omb_of(momentum[1]))
    ref, bnd, ref_nu, bnd_nu = oracle_and_bound(t, pos, neg, c[:K], keep, nb, chw, hw, nu, s_m, beta, omb)
    out, nu_new = restate(t, pos, neg, c[:K], keep, nb, chw, hw, nu, s_m, beta, omb, mutant)
    return worst_ratio(out.float(), ref, 1.01 * bnd), worst_ratio(nu_new, ref_nu, 1.01 * bnd_nu)


def test_fp32_restatement_stays_within_the_derived_bound():
    worst, where = [0.0, 0.0], [None, None]
    for seed, ((chw, hw), K, cls, nu_cls) in enumerate(itertools.product(((4, 1), (140, 35), (4000, 1000)), (1, 2, 3),
                                                                        ("normal", "ties", "low_byte", "below_key", "equal"),
                                                                        ("zero", "normal", "big"))):
        for j, n_keep in enumerate(sorted({1, min(2, hw), max(1, hw // 20), max(1, hw - 1), hw}) + [None]):
            nb, momentum = 1 + (seed + j) % 2, MOMENTA[(seed // 3 + j) % 3]
            r = _ratios(nb, chw, hw, K, n_keep, cls, nu_cls, 100 * seed + j, momentum=momentum)
            for o in range(2):
                if r[o] > worst[o]:
                    worst[o], where[o] = r[o], (nb, chw, hw, K, n_keep, cls, nu_cls, momentum)
    print(f"[bound] fp32 restatement, worst error / bound: out {worst[0]:.3f} {where[0]}, nu' {worst[1]:.3f} {where[1]}")
    assert max(worst) <= 1.0
    # a skipped term's NaN stays out, in the oracle as in the restatement
    assert max(_ratios(2, 4000, 1000, 3, 50, "normal", "normal", 5, c=(0.75, 0.0, 0.5), nan_in=1)) <= 1.0


def test_an_element_without_a_kept_term_and_without_state_is_exact():
    g = torch.Generator().manual_seed(9)
    nb, chw, hw = 2, 4000, 1000
    t, pos, neg = draw_rows("normal", nb * chw, 2, g)
    nu = torch.zeros(nb * chw)
    _, bnd, _, bnd_nu = oracle_and_bound(t, pos, neg, COEF[:2], [50, 50], nb, chw, hw, nu, 0.5, 0.4, omb_of(0.4))
    out, nu_new = restate(t, pos, neg, COEF[:2], [50, 50], nb, chw, hw, nu, 0.5, 0.4, omb_of(0.4))
    idle = bnd == 0
    assert 0.85 < float(idle.double().mean()) < 0.95 and torch.equal(idle, bnd_nu == 0), "about 0.95^2 of the elements keep no term"
    assert torch.equal(out[idle].float(), t[idle].float()) and bool((nu_new[idle] == 0).all())


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_break_the_bound(mutant):
    """nb = 2, four channels of 1000 pixels, normal draws, 50 kept per channel, nu of the terms' size, s_m = 0.5, beta = 0.4.  The one
    that recomputes omb is only visible where 1 - beta is small next to an ulp of beta and the state does not hide it: beta one ulp
    above 1 - 2^-12 with the omb of 1 - 2^-12 (the host's double beta rounds either way), nu = 0.  'wide': more than 100 x the bound"""
    kw = {}
    if mutant == "omb_in_kernel":
        beta = 1.0 - 2.0 ** -12
        kw = dict(nu_cls="zero", coef3=(0.5, float(torch.nextafter(torch.tensor(beta, dtype=torch.float32), torch.tensor(1.0))), omb_of(beta)))
    kw.setdefault("nu_cls", "normal")
    honest = _ratios(2, 4000, 1000, 3, 50, "normal", seed=11, **kw)
    broken = _ratios(2, 4000, 1000, 3, 50, "normal", seed=11, mutant=mutant, **kw)
    print(f"[mutant] {mutant}: honest out {honest[0]:.3f} nu' {honest[1]:.3f}, mutant out {broken[0]:.3e} nu' {broken[1]:.3e}")
    assert max(honest) <= 1.0 and max(broken) > 100.0


# ---------------------------------------------------------------------------------------------------------------------------
# 4. DirectionGuide
# ---------------------------------------------------------------------------------------------------------------------------
def test_direction_guide_momentum_validation():
    assert check_momentum(None) is None
    assert check_momentum((0.5, 0.4)) == (0.5, 0.4) and check_momentum([-2, 0]) == (-2.0, 0.0)
    for off in ((0.0, 0.4), (-0.0, 0.0), (1e-60, 0.4)):
        assert check_momentum(off) is None, "an s_m whose fp32 value is 0: no momentum"
    for bad in ((float("inf"), 0.4), (float("nan"), 0.4), (1e60, 0.4), (0.5, 1.0), (0.5, -0.1), (0.5, float("nan")), (0.5,), 0.5, ("a", 0.4)):
        with pytest.raises(ValueError, match="direction_momentum"):
            check_momentum(bad)
    eng = SimpleNamespace(cfg=SimpleNamespace(out_channels=4))
    ctx = torch.zeros(1, 77, 8)
    dirs = DirectionSet([Direction(ctx, ctx)])
    make = lambda m: DirectionGuide(eng, dirs, [1.0], 0.0, "off", 1, 4, 4, False, ctx, None, None, 750, momentum=m)
    assert make(None).momentum is None and make((0.0, 0.4)).momentum is None and make((0.5, 0.4)).momentum == (0.5, 0.4)
    assert make((0.5, 0.4)).mom is None, "the state is allocated when the plan is entered"
    with pytest.raises(ValueError, match="0 <= beta < 1"):
        make((0.5, 1.0))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the command lines
# ---------------------------------------------------------------------------------------------------------------------------
def _no_model(monkeypatch):
    import sliders_amd.model_util as mu

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(mu, "synthetic_engine", no_model)
    monkeypatch.setattr(torch, "load", no_model)
    monkeypatch.chdir(ROOT)


MOMENTUM_ERRORS = [
    (["--direction_momentum", "1"], "--direction_momentum needs --direction"),
    (["--direction", "a|b", "--direction_momentum", "x"], "expected S_M[:BETA]"),
    (["--direction", "a|b", "--direction_momentum", "1:y"], "expected S_M[:BETA]"),
    (["--direction", "a|b", "--direction_momentum", "1:2:3"], "expected S_M[:BETA]"),
    (["--direction", "a|b", "--direction_momentum", "inf"], "expected a finite s_m"),
    (["--direction", "a|b", "--direction_momentum", "1:1"], "0 <= beta < 1"),
    (["--direction", "a|b", "--direction_momentum=1:-0.5"], "0 <= beta < 1"),
]


@pytest.mark.parametrize("flags,what", MOMENTUM_ERRORS)
def test_generate_refuses_bad_momentum_before_a_model_is_built(monkeypatch, flags, what):
    _no_model(monkeypatch)
    with pytest.raises(SystemExit) as e:
        generate.main(["--synthetic"] + flags)
    assert what in str(e.value), e.value


@pytest.mark.parametrize("flags,what", MOMENTUM_ERRORS + [
    (["--direction", "smiling"], "expected POSITIVE|NEGATIVE[:ETA]"),
    (["--direction", "a|b:inf"], "expected a finite ETA"),
    (["--direction", "a|b"] * 4, "at most 3"),
    (["--direction", "a|b", "--direction_file", "tests/golden/prompts_sample.yaml"], "give one of them"),
    (["--direction_file", "no_such_file.yaml"], "no such file"),
    (["--direction_file", "tests/golden/prompts_sample.yaml", "--direction_entries", "0,2"], "entries 0 .. 1"),
    (["--direction_entries", "0"], "--direction_entries needs --direction_file"),
    (["--direction_quantile", "0.5"], "--direction_quantile needs --direction"),
    (["--direction", "a|b", "--direction_quantile", "1"], "expected 0 <= q < 1"),
    (["--direction", "a|b", "--lora_weight", "x.pt"], "not with --lora_weight"),
    (["--direction", "a|b", "--guidance_scale", "0"], "--guidance_scale 0"),
    (["--direction", "a|b", "--edit_guidance_scale", "0"], "--edit_guidance_scale 0"),
    (["--direction", "a|b", "--auto_mask", "--scales=0"], "non-zero scale"),
    (["--auto_mask"], "--auto_mask is the slider's footprint: it needs --lora_weight (or --compose)"),
])
def test_edit_refuses_bad_direction_options_before_a_model_is_built(monkeypatch, flags, what):
    _no_model(monkeypatch)
    with pytest.raises(SystemExit) as e:
        edit.main(["--synthetic", "--image", "x.png"] + flags)
    assert what in str(e.value), e.value


def test_auto_mask_takes_a_direction_in_place_of_a_slider():
    E = lambda *argv: edit.build_parser().parse_args(["--synthetic", "--image", "x.png"] + list(argv))
    G = lambda *argv: generate.build_parser().parse_args(["--synthetic"] + list(argv))
    a = E("--direction", "a|b:2", "--auto_mask", "--scales=-1,0,1", "--direction_momentum", "0.5")
    assert edit.check_args(a) == [-1.0, 0.0, 1.0] and a.auto_mask_scale == -1.0
    assert generate.direction_momentum(a) == (0.5, generate.DEFAULT_MOMENTUM_BETA) == (0.5, 0.4)
    assert generate.direction_momentum(E("--direction", "a|b", "--direction_momentum", "0:0.9")) == (0.0, 0.9)
    assert edit.check_args(E("--direction_file", "tests/golden/prompts_sample.yaml", "--auto_mask", "--compose", "x.pt:1")) == [-2.0, -1.0, 0.0, 1.0, 2.0]
    assert edit.check_args(E("--direction", "a|b", "--edit_prompt", "another", "--mask_tokens", "3")) == [-2.0, -1.0, 0.0, 1.0, 2.0]
    assert generate.check_args(G("--direction", "a|b", "--auto_mask", "--scales=0,2")) == [0.0, 2.0]
    # with neither a slider nor a direction today's refusal and its text stay, in both command lines
    for check, a in ((edit.check_args, E("--auto_mask")), (generate.check_args, G("--auto_mask"))):
        with pytest.raises(SystemExit) as e:
            check(a)
        assert str(e.value) == "--auto_mask is the slider's footprint: it needs --lora_weight (or --compose)"
    # the plain command lines check nothing new
    assert edit.check_args(E()) == [-2.0, -1.0, 0.0, 1.0, 2.0] and generate.check_args(G()) == [-2.0, -1.0, 0.0, 1.0, 2.0]
    assert math.isclose(generate.DEFAULT_MOMENTUM_BETA, 0.4)
