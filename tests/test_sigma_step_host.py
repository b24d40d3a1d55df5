"""The fused fp32 sampler step, host side (docs/SAMPLING.md, "Fused fp32 step"; no GPU):

1. the rows of schedulers.step_row are the existing scheduler classes' steps;
2. the dpmpp_2m rows are DPM-Solver++(2M) as the paper states it;
3. on a Gaussian toy problem those rows converge at second order and the euler rows at first;
4. the kernel's fp32 arithmetic (tests/sigma_step_ref.py: restate) stays within the derived bound of float64;
5. six wrong kernels do not;
6. the C entry point is declared, exported, and refuses bad arguments before any launch.
"""
import ctypes as C
import math
import os
import re

import pytest
import torch

from sliders_amd import lib, schedulers
from sliders_amd.schedulers import StepRow, step_row
from tests.sigma_step_ref import MUTANTS, U, bound, dpmpp_2m_oracle, restate, worst_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = (1, 2, 4, 10, 50)
SCHEDULERS = {                      # name -> (constructor, the spacings it accepts; None: it has one grid)
    "euler": (schedulers.EulerDiscreteScheduler, ("leading", "linspace")),
    "euler_a": (schedulers.EulerAncestralDiscreteScheduler, ("linspace", "leading", "trailing")),
    "lms": (schedulers.LMSDiscreteScheduler, (None,)),
    "ddpm": (schedulers.DDPMScheduler, (None,)),
    "dpmpp_2m": (schedulers.DPMSolverPP2MScheduler, ("leading", "linspace", "trailing")),
}
CASES = [(n, s, p) for n, (_, sp) in SCHEDULERS.items() for s in sp for p in ("epsilon", "v_prediction")]


def _make(name, spacing, pred):
    cls = SCHEDULERS[name][0]
    return cls(prediction_type=pred) if spacing is None else cls(prediction_type=pred, timestep_spacing=spacing)


def _eval(row, x, m, H, noise):
    """the row in float64: (out, H0)"""
    x0 = row.p * x + row.q * m
    h0 = (x - x0) / row.sigma if row.kind == 0 else x0
    out = row.a * x + row.c[0] * h0
    for k in range(row.n_hist):
        out = out + row.c[k + 1] * H[k]
    if noise is not None:
        out = out + row.c_n * noise
    return out, h0


# ---------------------------------------------------------------------------------------------------------------------------
# 1. rows equal the classes
# ---------------------------------------------------------------------------------------------------------------------------
def _coef_errors(name, sch, i, n, row):
    """Relative error, in units of u = 2^-24, by which each coefficient of `row` may differ from the one the class's `step` uses:
    1 for the row's own rounding to fp32 plus the roundings of the class's fp32 0-dim scalar arithmetic (one per operation; a square
    root is allowed a whole ulp, 2, and halves the relative error of its argument; a difference amplifies the errors of its
    operands by their size over the result's).  Counted on sliders_amd/schedulers.py as written; nothing is fitted.
    -> dict p, q, a, c (list), c_n"""
    v = sch.prediction_type == "v_prediction"
    if name == "ddpm":
        t = int(sch.timesteps[i])
        prev_t = t - sch.num_train_timesteps // n
        a_t = float(sch.alphas_cumprod[t])
        a_p = float(sch.alphas_cumprod[prev_t]) if prev_t >= 0 else 1.0
        kappa = (a_t / a_p) / (1 - a_t / a_p)        # current_beta_t = fl(1 - fl(a_t / a_p)): the quotient's u, amplified
        # epsilon: 1 / fl(sqrt a_t) (2) + 1 | fl(1 - a_t) (1) -> sqrt (0.5 + 2), / sqrt a_t (2) + 1;  v: sqrt a_t (2) + 1 | sqrt(fl(1 - a_t)) (2.5) + 1
        p, q = (3, 4) if v else (3, 6)
        # c0 = fl(fl(sqrt(a_p) (2) * cur_beta (1 + kappa)) (1) / fl(1 - a_t) (1)) (1) + 1
        # a  = fl(fl(sqrt(cur_alpha) (0.5 + 2) * fl(1 - a_p) (1)) (1) / fl(1 - a_t) (1)) (1) + 1
        # c_n = sqrt(fl(fl(fl(1 - a_p) / fl(1 - a_t)) (3) * cur_beta (1 + kappa)) (1)) -> (5 + kappa) / 2 + 2, + 1
        return dict(p=p, q=q, a=8, c=[7 + kappa], c_n=6 + kappa / 2)
    # sigma space, _pred_original: epsilon uses sigma itself (p = 1, q = -sigma: exact on both sides);
    # v: p = 1 / fl(fl(sigma^2) + 1) (2) + 1;  q = fl(-sigma / sqrt(fl(fl(sigma^2) + 1))) : (2) / 2 + 2, the quotient 1, + 1 -> 5, taken as 6
    p, q = (3, 6) if v else (0, 0)
    s, s1 = float(sch.sigmas[i]), float(sch.sigmas[i + 1])
    if name == "euler":            # dt = fl(sigma' - sigma): the row's own rounding of the same difference
        return dict(p=p, q=q, a=0, c=[1], c_n=0)
    if name in ("lms", "dpmpp_2m"):    # python-float coefficients in the class: only the row's rounding
        return dict(p=p, q=q, a=0 if name == "lms" else 1, c=[1] * (row.n_hist + 1), c_n=0)
    assert name == "euler_a"
    if s1 == 0.0:                  # sigma_up = sigma_down = 0 exactly
        return dict(p=p, q=q, a=0, c=[2], c_n=0)
    A, B = s1 * s1, s * s
    k1 = (A + B) / (B - A)
    # sigma_up = sqrt(fl(fl(A * fl(B - A)) / B)):  A (1), B - A (1 + k1), the product 1, B (1), the quotient 1 -> 5 + k1; sqrt: / 2 + 2
    r_up = (5 + k1) / 2 + 2
    up2 = A * (B - A) / B
    R = A - up2                    # sigma_down^2 = fl(A - fl(sigma_up^2)): u A + (2 r_up + 1) u sigma_up^2, over R, + 1
    r_down = (1 + (A + (2 * r_up + 1) * up2) / R) / 2 + 2
    dt = math.sqrt(R) - s          # fl(sigma_down - sigma): r_down u sigma_down + u |dt|, and the row's own u |dt|
    return dict(p=p, q=q, a=0, c=[r_down * math.sqrt(R) / abs(dt) + 2], c_n=r_up + 1)


@pytest.mark.parametrize("name,spacing,pred", CASES)
def test_rows_equal_the_scheduler_classes(name, spacing, pred):
    """Over whole grids: at every step the row, evaluated in float64 on the class's own latent and history, gives what the class's
    `step` gives on float64 tensors with the same noise - up to the fp32 rounding of each coefficient (and, on the class's side, the
    roundings of its fp32 scalar arithmetic): |row - class| <= u sum_j e_j |coef_j operand_j|, e_j from _coef_errors, the x0 terms
    divided by sigma for the derivative rows.  1e-13 S covers the float64 arithmetic of both sides."""
    g = torch.Generator().manual_seed(5)
    worst = 0.0
    for n in GRIDS:
        sch = _make(name, spacing, pred)
        sch.set_timesteps(n)
        x = torch.randn(64, generator=g, dtype=torch.float64) * float(sch.init_noise_sigma)
        for i, t in enumerate(sch.timesteps):
            m = torch.randn(64, generator=g, dtype=torch.float64)
            nz = torch.randn(64, generator=g, dtype=torch.float64)
            row = step_row(sch, i, n)
            assert row.n_hist == len(row.c) - 1 <= schedulers.history_depth(sch, n)
            H = ([d for d in reversed(sch.derivatives)] if name == "lms" else list(sch.denoised) if name == "dpmpp_2m" else [])
            assert len(H) >= row.n_hist
            if name == "lms":
                assert row.n_hist == min(i + 1, 4) - 1                      # the order grows 1 -> 4
            if name == "ddpm" and i == n - 1:
                assert row.c_n == 0.0 and int(t) == 0                       # the last step adds no noise
            got, _ = _eval(row, x, m, H, nz if row.c_n != 0.0 else None)
            want = sch.step(m, t, x, noise=nz).prev_sample
            assert want.dtype == torch.float64
            e = _coef_errors(name, sch, i, n, row)
            px, qm = (row.p * x).abs(), (row.q * m).abs()
            e_h = U * (e["p"] * px + e["q"] * qm) / (row.sigma if row.kind == 0 else 1.0)
            x0 = row.p * x + row.q * m
            h0 = (x - x0) / row.sigma if row.kind == 0 else x0
            terms = [(e["a"], row.a * x), (e["c"][0], row.c[0] * h0)] + [(e["c"][k + 1], row.c[k + 1] * H[k]) for k in range(row.n_hist)]
            terms.append((e["c_n"], row.c_n * nz))
            S = sum(v.abs() for _, v in terms)
            bnd = U * sum(ej * v.abs() for ej, v in terms) + abs(row.c[0]) * e_h + 1e-13 * S
            worst = max(worst, worst_ratio(got, want, 1.01 * bnd))
            # the next pass's input: x s_next against the class's x / fl(sqrt(fl(fl(sigma'^2) + 1))): (2) / 2 + 2 and the row's 1
            if i + 1 < n:
                scaled = sch.scale_model_input(want, sch.timesteps[i + 1])
                assert bool(((want * row.s_next - scaled).abs() <= 4 * U * 1.01 * scaled.abs()).all())
            else:
                assert row.s_next == 1.0 or name == "ddpm"
            x = want
    print(f"[rows] {name} {spacing} {pred}: worst |row - class| / bound {worst:.3f}")
    assert worst <= 1.0


def test_step_row_refuses_what_it_cannot_state():
    sch = schedulers.EulerDiscreteScheduler()
    sch.set_timesteps(4)
    with pytest.raises(ValueError, match="set to 4 steps"):
        step_row(sch, 0, 5)
    with pytest.raises(ValueError, match="step 4 of 4"):
        step_row(sch, 4, 4)
    # the table of create() and the grids of the euler class are what they were
    assert [k for k in ("ddpm", "lms", "euler_a", "dpmpp_2m", "euler") if _created(k)] == ["ddpm", "lms", "euler_a"]
    with pytest.raises(ValueError, match="linspace and leading"):
        schedulers.EulerDiscreteScheduler(timestep_spacing="trailing")
    sch = schedulers.DPMSolverPP2MScheduler()
    assert (sch.timestep_spacing, sch.steps_offset) == ("leading", 1)
    sch.set_timesteps(4)
    assert sch.timesteps.tolist() == [751.0, 501.0, 251.0, 1.0]
    sch = schedulers.DPMSolverPP2MScheduler(timestep_spacing="trailing")
    sch.set_timesteps(4)
    assert sch.timesteps.tolist() == [999.0, 749.0, 499.0, 249.0]


def _created(key):
    try:
        schedulers.create(key)
        return True
    except ValueError:
        return False


# ---------------------------------------------------------------------------------------------------------------------------
# 2. DPM-Solver++ 2M against the paper's form
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", ["leading", "linspace", "trailing"])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_dpmpp_2m_rows_are_the_papers_algorithm(spacing, pred):
    """the unrounded rows, stepped in float64 over whole grids with a model output that depends on the latent, against
    tests/sigma_step_ref.py: dpmpp_2m_oracle (variance-preserving variables, lambda form): 1e-12 relative at every step"""
    worst = 0.0
    for n in GRIDS:
        sch = _make("dpmpp_2m", spacing, pred)
        sch.set_timesteps(n)
        sig = sch.sigmas.double().tolist()
        g = torch.Generator().manual_seed(n)
        x = torch.randn(64, generator=g, dtype=torch.float64) * float(sch.init_noise_sigma)
        w = torch.randn(64, generator=g, dtype=torch.float64)
        model = lambda x, i: torch.tanh(w * x / (sig[i] ** 2 + 1) ** 0.5 + 0.1 * i)       # any smooth function of (x, step)

        def denoise(x, i):          # the predicted clean sample of the model, written from the definitions of epsilon and v
            s = sig[i]
            if pred == "epsilon":
                return x - s * model(x, i)
            al, st = 1 / math.sqrt(s * s + 1), s / math.sqrt(s * s + 1)
            return al * (x * al) - st * model(x, i)

        want = dpmpp_2m_oracle(sig, x, denoise)
        H = []
        for i in range(n):
            row = step_row(sch, i, n, rounded=False)
            x, h0 = _eval(row, x, model(x, i), H, None)
            H = [h0]
            worst = max(worst, float((x - want[i]).abs().max() / want[i].abs().max()))
        last = step_row(sch, n - 1, n)
        assert (last.a, last.c) == (0.0, (1.0,)), "sigma' = 0: out is x0"
    print(f"[2M] {spacing} {pred}: worst relative difference to the lambda-form oracle {worst:.2e}")
    assert worst <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# 3. Gaussian toy: order of convergence
# ---------------------------------------------------------------------------------------------------------------------------
def _toy_error(name, n, s=0.5):
    """data N(0, s^2): the exact denoiser is x s^2 / (s^2 + sigma^2) and the probability-flow solution from x = sigma_0 ends at
    sigma_0 sqrt(s^2 / (s^2 + sigma_0^2)); the rows' error at the end of the leading / offset-1 grid, float64"""
    sch = _make(name, "leading", "epsilon")
    sch.set_timesteps(n)
    sig = sch.sigmas.double().tolist()
    x = torch.tensor([sig[0]], dtype=torch.float64)
    H = []
    for i in range(n):
        row = step_row(sch, i, n, rounded=False)
        eps = (x - x * s * s / (s * s + sig[i] ** 2)) / sig[i]
        x, h0 = _eval(row, x, eps, H, None)
        H = [h0]
    return abs(float(x) - sig[0] * math.sqrt(s * s / (s * s + sig[0] ** 2)))


def test_gaussian_toy_orders():
    err = {name: {n: _toy_error(name, n) for n in (20, 40, 80)} for name in ("euler", "dpmpp_2m")}
    for n in (20, 40, 80):
        print(f"[toy] {n} steps: euler {err['euler'][n]:.3e}, dpmpp_2m {err['dpmpp_2m'][n]:.3e}")
    r2, r1 = err["dpmpp_2m"][40] / err["dpmpp_2m"][80], err["euler"][40] / err["euler"][80]
    print(f"[toy] 40 -> 80 error ratio: dpmpp_2m {r2:.2f}, euler {r1:.2f}")
    assert r2 >= 3.0, "dpmpp_2m does not converge at second order (wrong r, or c1 dropped?)"
    assert r1 <= 2.2
    assert all(err["dpmpp_2m"][n] < err["euler"][n] for n in (20, 40, 80))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. / 5. the kernel's arithmetic: bound and mutants
# ---------------------------------------------------------------------------------------------------------------------------
def _inputs(n, kind, seed):
    """(u, t, x, H[3], noise): bf16-valued epsilon halves, fp32 the rest; kind: unit normal, |x| ~ 1e3, all-zero epsilon"""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(n, generator=g)
    u, t = r().to(torch.bfloat16), r().to(torch.bfloat16)
    x, H, nz = r(), [r() for _ in range(3)], r()
    if kind == "large":
        x, H = x * 1e3, [h * 1e3 for h in H]
    if kind == "zero_eps":
        u, t = torch.zeros_like(u), torch.zeros_like(t)
    return u, t, x, H, nz


def _scheduler_rows():
    """(label, row): the first, a middle and the last step of a 10-step grid of every scheduler, epsilon and v"""
    for name, (_, spacings) in SCHEDULERS.items():
        for pred in ("epsilon", "v_prediction"):
            sch = _make(name, spacings[0], pred)
            sch.set_timesteps(10)
            for i in (0, 5, 9):
                yield f"{name}/{pred}/{i}", step_row(sch, i, 10)


def _ratios(args, row, g, mutant=None, single=False):
    u, t, x, H, nz = args
    t = None if single else t
    nz = nz if row.c_n != 0.0 else None
    got = restate(u, t, x, H, nz, row, g, mutant=mutant)
    ref, bnd = bound(u, t, x, H, nz, row, g)
    return [worst_ratio(a, b, c) for a, b, c in zip(got, ref, bnd)]


def test_fp32_restatement_stays_within_the_derived_bound():
    worst = [0.0, 0.0, 0.0]
    where = [None] * 3
    for label, row in _scheduler_rows():
        for kind in ("unit", "large", "zero_eps"):
            for single in (False, True):
                r = _ratios(_inputs(4096, kind, seed=len(label)), row, 7.5, single=single)
                for k in range(3):
                    if r[k] > worst[k]:
                        worst[k], where[k] = r[k], (label, kind, single)
    print(f"[bound] fp32 restatement, worst error / bound: out {worst[0]:.3f} {where[0]}, H0 {worst[1]:.3f} {where[1]}, "
          f"scaled input {worst[2]:.3f} {where[2]}")
    assert max(worst) <= 1.0


# a row on which every mutant acts: the derivative and the denoised form, three history terms with distinct coefficients, noise,
# p != q, sigma' != sigma
_MUTANT_ROWS = [StepRow(0, 0.25, -1.75, 2.0, 1.0, (-0.75, 0.5, -0.25, 0.125), 0.5, 0.8),
                StepRow(1, 0.25, -1.75, 2.0, 0.5, (0.75, 0.5, -0.25, 0.125), 0.5, 0.8)]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_break_the_bound(mutant):
    for row in _MUTANT_ROWS:
        args = _inputs(4096, "unit", seed=9)
        honest, broken = _ratios(args, row, 7.5), _ratios(args, row, 7.5, mutant=mutant)
        print(f"[mutant] {mutant}, kind {row.kind}: honest {max(honest):.3f}, mutant {max(broken):.3e}")
        assert max(honest) <= 1.0 < max(broken)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. ABI
# ---------------------------------------------------------------------------------------------------------------------------
def _raw_call(ptrs, dims, coef=(1.0, -1.0, 1.0, 1.0, 0.5, 0, 0, 0, 0, 1.0, 7.5)):
    l = lib.load()
    return l.slh_sigma_step((C.c_void_p * 11)(*ptrs), (C.c_int32 * 5)(*dims), (C.c_float * 11)(*coef), None)


def test_abi_declared_exported_and_refusing_on_the_host():
    hdr = open(os.path.join(ROOT, "include", "sliders_hip.h")).read()
    assert re.search(r"^int slh_sigma_step\(const void\* const\* ptrs, const int32_t\* dims, const float\* coef, slh_stream_t stream\);",
                     hdr, flags=re.M)
    assert "slh_sigma_step" in lib.EXPORTS and hasattr(lib.load(), "slh_sigma_step")
    assert lib.load().slh_op_info(-1, None, None, None) == 41 == len(lib._ENTRY), "no new opcode"
    ok = [0x1000, 0, 0x2000, 0, 0, 0, 0, 0x3000, 0, 0, 0]          # (never dereferenced: every call below is refused before the launch)
    dims = [1, 64, 0, 0, 0]

    def refused(ptrs, dims, what, **kw):
        assert _raw_call(ptrs, dims, **kw) != 0
        msg = lib.last_error()
        assert "slh_sigma_step" in msg and what in msg, msg

    for hole in (0, 2, 7):
        refused([0 if k == hole else v for k, v in enumerate(ok)], dims, "null eps / x / out")
    refused(ok, [1, 64, 2, 0, 0], "H[1] is null")
    refused(ok, [1, 64, 4, 0, 0], "n_hist = 4")
    refused(ok, [1, 64, -1, 0, 0], "n_hist = -1")
    refused(ok, [0, 64, 0, 0, 0], "nb = 0")
    refused(ok, [1, 0, 0, 0, 0], "chw = 0")
    refused(ok, [1, 64, 0, 2, 0], "kind 2")
    refused(ok, dims, "sigma = 0", coef=(1.0, -1.0, 0.0, 1.0, 0.5, 0, 0, 0, 0, 1.0, 7.5))
    refused([0x1000, 0, 0x2002, 0, 0, 0, 0, 0x3000, 0, 0, 0], dims, "not 4-byte aligned")
    refused([0x1001, 0, 0x2000, 0, 0, 0, 0, 0x3000, 0, 0, 0], dims, "not 2-byte aligned")
    refused([0x1000, 0x1800, 0x2000, 0, 0, 0, 0, 0x3000, 0, 0, 0], [1, 64, 0, 0, 1], "single branch has no eps_text")
    with pytest.raises(lib.SlidersHipError, match="slh_sigma_step"):
        lib.sigma_step(0, eps=0, x=0x2000, out=0x3000, nb=1, chw=64, kind=1, p=1.0, q=-1.0)
    with pytest.raises(lib.SlidersHipError, match="at most 3"):
        lib.sigma_step(0, eps=0x1000, x=0x2000, out=0x3000, nb=1, chw=64, kind=1, p=1.0, q=-1.0, hist=[0x4000] * 4)
