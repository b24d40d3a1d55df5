"""slh_latent_blend and the masked sampler's command line, host side (docs/SAMPLING.md, "Localised sampling"; no GPU):

1. the C entry point is declared, exported, adds no opcode, and refuses bad arguments before any launch;
2. the kernel's fp32 arithmetic (edit.blend_reference) stays within the derived bound of float64 (tests/latent_blend_ref.py);
3. five wrong kernels exceed it by a wide factor;
4. python -m sliders_amd.generate refuses every bad combination of the mask options before a model is built;
5. SampleTrace hands out the UNet inputs of its chain.
"""
import ctypes as C
import os
import re

import pytest
import torch

from sliders_amd import generate, lib
from sliders_amd.sampler import SampleTrace
from tests.latent_blend_ref import MUTANTS, bound, expand_mask, oracle, restate, worst_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(4, 1), (900, 225), (1024, 256), (4356, 1089), (5, 5), (1023, 341), (48, 12)]
MASKS = ("zeros", "ones", "binary", "fractional", "mixed")


def draw_mask(cls, n, g):
    if cls == "fractional":
        return torch.rand(n, generator=g).clamp(2.0 ** -20, 1.0 - 2.0 ** -20)
    if cls == "binary":
        return (torch.rand(n, generator=g) < 0.5).float()
    if cls == "mixed":            # exact 0 and 1 next to fractions, a tiny one among them
        return torch.tensor([0.0, 1.0, 0.5, 2.0 ** -20, 0.8125]).repeat(n // 5 + 1)[:n]
    return torch.full((n,), 1.0 if cls == "ones" else 0.0)


def draw_inputs(cls, n, mask_flat, g, bf16):
    """(e, keep) flat [n]; mask_flat: the mask per element, which decides where a NaN may sit"""
    big = 1e3 if cls == "large" else 1.0
    e, keep = torch.randn(n, generator=g) * big, torch.randn(n, generator=g) * big
    if cls == "nan_e":
        e[mask_flat == 0] = float("nan")
    if cls == "nan_keep":
        keep[mask_flat == 1] = float("nan")
    return (e.to(torch.bfloat16), keep.to(torch.bfloat16)) if bf16 else (e, keep)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. ABI
# ---------------------------------------------------------------------------------------------------------------------------
def _raw_call(ptrs, dims, coef=(1.0,)):
    l = lib.load()
    return l.slh_latent_blend((C.c_void_p * 6)(*ptrs), (C.c_int32 * 4)(*dims), (C.c_float * 1)(*coef) if coef is not None else None, None)


def test_abi_declared_exported_and_refusing_on_the_host():
    hdr = open(os.path.join(ROOT, "include", "sliders_hip.h")).read()
    assert re.search(r"^int slh_latent_blend\(const void\* const\* ptrs, const int32_t\* dims, const float\* coef, slh_stream_t stream\);",
                     hdr, flags=re.M)
    assert "slh_latent_blend" in lib.EXPORTS and hasattr(lib.load(), "slh_latent_blend")
    assert lib.load().slh_op_info(-1, None, None, None) == 41 == len(lib._ENTRY), "no new opcode"
    ok = [0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000]          # (never dereferenced: every call below is refused before the launch)
    f32, b16 = [1, 64, 16, 1], [1, 64, 16, 0]

    def refused(ptrs, dims, what, **kw):
        assert _raw_call(ptrs, dims, **kw) != 0
        msg = lib.last_error()
        assert "slh_latent_blend" in msg and what in msg, msg

    for hole in range(4):
        for dims in (f32, b16):
            refused([0 if k == hole else v for k, v in enumerate(ok)], dims, "null e / keep / mask / out")
    for k, name in enumerate(("nb", "chw", "hw")):
        for bad in (0, -1):
            refused(ok, [bad if j == k else v for j, v in enumerate(f32)], f"{name} = {bad}")
    refused(ok, [1, 64, 24, 1], "not a multiple of hw")
    refused(ok, [1, 64, 16, 2], "dtype 2")
    refused(ok, [1, 64, 16, -1], "dtype -1")
    refused(ok, f32, "needs coef", coef=None)
    for bad in (float("inf"), float("-inf"), float("nan")):
        refused(ok, f32, "not finite", coef=(bad,))
    assert _raw_call([0 if k == 0 else v for k, v in enumerate(ok)], b16, coef=(float("nan"),)) != 0 and "null e" in lib.last_error(), \
        "dtype 0 does not read s_next"
    for k in (0, 1, 3):
        refused([v + 2 if j == k else v for j, v in enumerate(ok)], f32, "not 4-byte aligned")
        refused([v + 1 if j == k else v for j, v in enumerate(ok)], b16, "not 2-byte aligned")
    for k in (4, 5):
        refused([v + 1 if j == k else v for j, v in enumerate(ok)], f32, "not 2-byte aligned")
    refused([0x1000, 0x2000, 0x3002, 0x4000, 0, 0], f32, "mask pointer")
    refused([0x1000, 0x4080, 0x3000, 0x4000, 0, 0], f32, "keep overlaps out")
    refused([0x1000, 0x2000, 0x5010, 0x4000, 0x5000, 0], f32, "mask overlaps in_bf16")
    with pytest.raises(lib.SlidersHipError, match="slh_latent_blend"):
        lib.latent_blend(0, e=0x1000, keep=0x2000, mask=0, out=0x4000, nb=1, chw=64, hw=16, fp32=True)
    with pytest.raises(lib.SlidersHipError, match="not finite"):
        lib.latent_blend(0, e=0x1000, keep=0x2000, mask=0x3000, out=0x4000, nb=1, chw=64, hw=16, fp32=True, s_next=float("inf"))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. / 3. the kernel's arithmetic: bound and mutants
# ---------------------------------------------------------------------------------------------------------------------------
S_NEXT = float(torch.tensor(0.37, dtype=torch.float32))          # fp32-valued, as the kernel reads it


def _ratios(nb, chw, hw, mcls, icls, bf16, seed, mutant=None, s_next=S_NEXT):
    g = torch.Generator().manual_seed(seed)
    n = nb * chw
    mask = draw_mask(mcls, nb * hw, g)
    e, keep = draw_inputs(icls, n, expand_mask(mask, nb, chw, hw), g, bf16)
    s = 1.0 if bf16 else s_next
    got = restate(e, keep, mask, nb, chw, hw, s, bf16_out=bf16, mutant=mutant)
    ref = oracle(e, keep, mask, nb, chw, hw, s)
    bnd = bound(e, keep, mask, nb, chw, hw, s, bf16_out=bf16)
    return [worst_ratio(a, b, 1.01 * c) for a, b, c in zip(got, ref, bnd)]


def test_fp32_restatement_stays_within_the_derived_bound():
    worst, where = [0.0, 0.0], [None, None]
    for idx, ((chw, hw), nb, mcls, icls, bf16) in enumerate(
            (s, nb, m, i, b) for s in SHAPES for nb in (1, 2) for m in MASKS for i in ("unit", "large", "nan_e", "nan_keep") for b in (False, True)):
        r = _ratios(nb, chw, hw, mcls, icls, bf16, seed=idx)
        for k in range(2):
            if r[k] > worst[k]:
                worst[k], where[k] = r[k], (nb, chw, hw, mcls, icls, bf16)
    print(f"[bound] fp32 restatement, worst error / bound: out {worst[0]:.3f} {where[0]}, scaled input {worst[1]:.3f} {where[1]}")
    assert max(worst) <= 1.0


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_break_the_bound(mutant):
    """nb = 2 and four channels: every wrong mask index reads another pixel's value somewhere; unit-normal inputs, a mask that mixes
    exact 0 and 1 with fractions.  'wide': more than 100 x the bound"""
    honest = _ratios(2, 1024, 256, "mixed", "unit", False, seed=9)
    broken = _ratios(2, 1024, 256, "mixed", "unit", False, seed=9, mutant=mutant)
    print(f"[mutant] {mutant}: honest {max(honest):.3f}, mutant {max(broken):.3e}")
    assert max(honest) <= 1.0 and max(broken) > 100.0


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the command line's argument errors
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,what", [
    (["--mask_feather", "1"], "--mask_feather / --save_mask need"),
    (["--save_mask", "m.png"], "--mask_feather / --save_mask need"),
    (["--mask", "no_such_file.png"], "no such file"),
    (["--mask_invert"], "--mask_invert needs"),
    (["--mask_tokens", "3", "--auto_mask"], "give one of them"),
    (["--mask_tokens", "a,b"], "expected comma-separated key positions"),
    (["--mask_tokens", "77"], "expected key positions in 0 .. 76"),
    (["--mask_word", "person"], "needs the model's tokenizer"),
    (["--mask_word_draws", "2"], "need --mask_word or --mask_tokens"),
    (["--save_attention", "a.png"], "need --mask_word or --mask_tokens"),
    (["--mask_tokens", "3", "--mask_word_threshold", "0"], "expected 0 < threshold <= 1"),
    (["--mask_tokens", "3", "--mask_word_draws", "0"], "expected at least 1"),
    (["--mask_tokens", "3", "--mask_feather", "-1"], "expected a finite sigma >= 0"),
    (["--auto_mask"], "it needs --lora_weight"),
    (["--auto_mask_draws", "2"], "--auto_mask_draws needs --auto_mask"),
    (["--auto_mask", "--lora_weight", "x.pt", "--scales=0"], "measured at a non-zero scale"),
    (["--auto_mask", "--lora_weight", "x.pt", "--auto_mask_threshold", "2"], "expected 0 < threshold <= 1"),
    (["--auto_mask", "--lora_weight", "x.pt", "--auto_mask_dilate", "-1"], "expected >= 0"),
    (["--auto_mask", "--lora_weight", "x.pt", "--start_noise", "100"], "--auto_mask: no step of the grid"),
    (["--mask_tokens", "3", "--scheduler", "euler"], "--fp32_latents"),
    (["--mask_tokens", "3", "--scheduler", "lms"], "--fp32_latents"),
    (["--mask_tokens", "3", "--turbo", "--fp32_latents"], "not with --no_cfg"),
])
def test_cli_argument_errors_exit_before_a_model_is_built(monkeypatch, flags, what):
    import sliders_amd.model_util as mu

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(mu, "synthetic_engine", no_model)
    monkeypatch.setattr(torch, "load", no_model)
    with pytest.raises(SystemExit) as e:
        generate.main(["--synthetic"] + flags)
    assert what in str(e.value), e.value


def test_cli_without_mask_flags_checks_nothing_new():
    for argv in (["--synthetic"], ["--synthetic", "--turbo"], ["--synthetic", "--scheduler", "lms", "--scales=1"]):
        a = generate.resolve_sampling(generate.build_parser().parse_args(argv), generate.explicit_args(argv))
        assert not generate.masked(a) and generate.check_args(a) == [float(v) for v in a.scales.split(",")]
    # an unmasked sweep keeps scale 0 as a trace only where the other scales' bits cannot change: no draws, no history, a second scale
    P = lambda *argv: generate.build_parser().parse_args(list(argv))
    assert generate.shares_prefix(P(), [-1.0, 0.0, 1.0]) and generate.shares_prefix(P("--scheduler", "euler", "--fp32_latents"), [0.0, 1.0])
    assert not generate.shares_prefix(P(), [-1.0, 1.0]) and not generate.shares_prefix(P(), [0.0])
    for other in (["--scheduler", "euler"], ["--scheduler", "euler_a", "--fp32_latents"], ["--scheduler", "ddpm", "--fp32_latents"],
                  ["--scheduler", "lms", "--fp32_latents"], ["--scheduler", "dpmpp_2m"]):
        assert not generate.shares_prefix(P(*other), [-1.0, 0.0, 1.0]), other
    # the grid the checks see is the sampler's
    a = generate.build_parser().parse_args(["--ddim_steps", "4"])
    assert generate.sampling_grid(a) == [750, 500, 250, 0]
    a = generate.build_parser().parse_args(["--ddim_steps", "4", "--scheduler", "dpmpp_2m", "--timestep_spacing", "trailing"])
    assert generate.sampling_grid(a) == [999.0, 749.0, 499.0, 249.0]


# ---------------------------------------------------------------------------------------------------------------------------
# 5. SampleTrace
# ---------------------------------------------------------------------------------------------------------------------------
def test_sample_trace_inputs():
    g = torch.Generator().manual_seed(1)
    visited = torch.randn(3, 1, 4, 2, 2, generator=g)
    x0 = torch.randn(1, 4, 2, 2, generator=g)
    common = dict(timesteps=[700.0, 400.0, 100.0], x_start=x0, final=visited[-1].to(torch.bfloat16), draws=None, ctx=torch.zeros(2, 77, 8),
                  pooled=None, time_ids=None, guidance=7.5, single=False, start_noise=750.0)
    tr = SampleTrace(visited=visited, input0=x0 * 0.5, s_in=[1.0, 0.25, 0.75], **common)
    assert tr.steps == 3 and torch.equal(tr.unet_input(0), x0 * 0.5)
    assert tr.unet_input(2).dtype == torch.bfloat16 and torch.equal(tr.unet_input(2), (visited[1] * 0.75).to(torch.bfloat16))
    bf = visited.to(torch.bfloat16)
    tr = SampleTrace(visited=bf, input0=x0.to(torch.bfloat16), s_in=None, **common)
    assert torch.equal(tr.unet_input(1), bf[0]), "ddim: the visited latent itself"
