"""Shared helpers for the GPU parity tests (the HIP path is always called through the C ABI)."""
import torch

from sliders_amd import lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return t.data_ptr() if t is not None else 0


def bf(t):
    return t.to(torch.bfloat16)


def rel_err(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def max_err(a, b):
    return (a.float() - b.float()).abs().max().item()


def report(name, got, ref, tol_rel):
    r = rel_err(got, ref)
    m = max_err(got, ref)
    print(f"[parity] {name}: rel_l2={r:.3e} max_abs={m:.3e} ref_rms={ref.float().pow(2).mean().sqrt().item():.3e}")
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite output"
    assert r < tol_rel, f"{name}: rel_l2 {r:.3e} >= {tol_rel:.1e} (max_abs {m:.3e})"


# ---------------------------------------------------------------------------------------------------------------------------
# Element-wise parity (tests/gemm_matrix.py, tests/test_gemm_matrix_gpu.py, the stand-in / mutant proof in tests/test_host.py)
# ---------------------------------------------------------------------------------------------------------------------------
BF16_RND = 2.0 ** -8        # bf16 keeps 8 significant bits: round-to-nearest is within 2^-8 relative (truncation: 2^-7)
FP32_EPS = 2.0 ** -24       # one fp32 rounding; an fp32 sum of n terms, in any order, is within n * 2^-24 * (sum of |terms|)
STAT_MIN_ABS = 0.1          # the rounding statistic looks at elements with |ref| above this ...
STAT_MIN_COUNT = 10000      # ... and only where there are at least this many of them
STAT_LIMIT = 0.05           # |b| of round-to-nearest is <= 0.005, of truncation 0.72


def elementwise_bound(ref, sabs, n, extra=None, rel=BF16_RND):
    """|got - ref| <= rel |ref| + n 2^-24 S + R, per element (float64 tensors).  ref: the float64 reference; sabs (S): the expression of
    ref evaluated on absolute values; n: the number of terms summed (a number, or a tensor that broadcasts); extra (R): what an
    internal bf16 rounding may add (None: nothing); rel: 2^-8 for a bf16 output, 0 for an fp32 side output."""
    b = rel * ref.abs() + n * FP32_EPS * sabs
    return b if extra is None else b + extra


def rounding_statistic(got, ref):
    """b = mean((got - ref) sign(ref) / (2^-8 |ref|)) over the elements with |ref| > 0.1: round-to-nearest centres on 0, a kernel that
    truncates towards zero sits at about -0.7.  (b, count); b is None with fewer than STAT_MIN_COUNT such elements."""
    g, r = got.double().reshape(-1), ref.double().reshape(-1)
    m = r.abs() > STAT_MIN_ABS
    cnt = int(m.sum())
    if cnt < STAT_MIN_COUNT:
        return None, cnt
    b = ((g[m] - r[m]) * torch.sign(r[m]) / (BF16_RND * r[m].abs())).mean().item()
    return b, cnt


def check_elementwise(name, got, ref, bound, statistic=True):
    """Every element of got within bound of ref, no non-finite value, and - for a bf16 output with enough large elements - the rounding
    statistic within STAT_LIMIT.  Returns (worst |got - ref| / bound, flat index of the worst element, b or None); raises
    AssertionError naming the first failure.  Elements whose bound is exactly zero must be exactly equal."""
    g, r, bd = got.double(), ref.double(), bound.double()
    assert g.shape == r.shape == bd.shape, f"{name}: shapes {tuple(g.shape)} / {tuple(r.shape)} / {tuple(bd.shape)}"
    assert bool(torch.isfinite(bd).all()) and bool((bd >= 0).all()), f"{name}: the bound itself is not finite and non-negative everywhere"
    assert bool(torch.isfinite(r).all()), f"{name}: non-finite reference"
    err = (g - r).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = torch.where(bd > 0, err / bd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    flat = ratio.reshape(-1)
    if flat.numel() == 0:
        return 0.0, -1, None
    worst, at = flat.max(0)
    worst, at = float(worst), int(at)
    b = None
    if statistic and got.dtype == torch.bfloat16:
        b, _ = rounding_statistic(got, ref)
    if worst > 1.0:
        nbad = int((flat > 1.0).sum())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(at), ratio.shape)) if ratio.dim() else ()
        raise AssertionError(f"{name}: {nbad} of {flat.numel()} elements beyond the bound; worst |got - ref| / bound = {worst:.3g} at {idx}: "
                             f"got {float(g.reshape(-1)[at])!r} ref {float(r.reshape(-1)[at])!r} bound {float(bd.reshape(-1)[at]):.3e}")
    if b is not None and abs(b) > STAT_LIMIT:
        raise AssertionError(f"{name}: rounding statistic b = {b:+.3f} beyond +-{STAT_LIMIT} (round-to-nearest: |b| <= 0.005, truncation: -0.72)")
    return worst, at, b
