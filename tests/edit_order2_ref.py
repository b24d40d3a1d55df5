"""slh_edit_step2 (include/sliders_hip.h) restated for the tests: one step's float64 oracle with the derived per-element bounds
(docs/EDIT.md, "Second-order noise space"), and the kernel's fp32 arithmetic as plain tensor operations in the kernel's order.

u = 2^-24.  E = |eps_u| + g (|eps_t| + |eps_u|) bounds |e| term by term; S_x0 and S_mu1 are the x0h and mu_1 expressions on absolute
values (6 and 8 roundings on their longest paths).  With a history the mean gains d = x0h - x0_prev, p = c_corr d, mu = mu_1 + p: three
more roundings, and S_mu = S_mu1 + |c_corr| (S_x0 + |x0_prev|).  n = 8 without a history, 11 with one.

    x0_out                |x0_out - x0h|            <= 6 u S_x0
    mode 0  resid         |resid - (target - mu)|   <= n u S_mu + u (|target| + |mu|)
    mode 0  out           |out - target|            <= 3 u (|target| + |mu|)                     (the error of mu cancels)
    mode 1  out           |out - (mu + resid)|      <= (n + 1) u (S_mu + |resid|)  =: B_e
    mode 1  with a mask   |out - (k + m (e - k))|   <= m B_e + 4 u (|k| + m |e - k|)             m = 0: k's bits
"""
import torch

from sliders_amd.edit import blend_reference, ddpm_mu2_reference, fp32_coefficients

U = 2.0 ** -24


def s_x0(f, ax, E, v):
    return f["c_sqrt_alpha_t"] * ax + f["c_sqrt_beta_t"] * E if v else f["c_inv_sqrt_alpha_t"] * (ax + f["c_sqrt_beta_t"] * E)


def s_mu1(f, ax, E, v):
    pe = f["c_sqrt_alpha_t"] * E + f["c_sqrt_beta_t"] * ax if v else E
    return f["c_sqrt_alpha_prev"] * s_x0(f, ax, E, v) + f["c_dir"] * pe


def mu_oracle_and_bound(eu, et, x, coef, g, v, x0_prev=None):
    """(mu, x0h, |mu_hat - mu| bound, |x0_hat - x0h| bound, n, S_mu), float64; coef carries c_corr exactly when x0_prev is given"""
    f = fp32_coefficients(coef)
    mu, x0 = ddpm_mu2_reference(eu, et, x, coef, g, v, torch.float64, x0_prev)
    gf = float(torch.tensor(g, dtype=torch.float32))
    E = eu.double().abs() + gf * (et.double().abs() + eu.double().abs())
    ax = x.double().abs()
    Sx0 = s_x0(f, ax, E, v)
    S, n = s_mu1(f, ax, E, v), 8
    if x0_prev is not None:
        S, n = S + abs(f["c_corr"]) * (Sx0 + x0_prev.double().abs()), 11
    return mu, x0, n * U * S, 6 * U * Sx0, n, S


def step_oracle(eu, et, x, coef, g, v, mode, x0_prev=None, target=None, resid=None, keep=None, mask=None):
    """One launch against float64: {name: (reference, bound)} for x0_out, out and (mode 0) resid.  mask: already one value per element."""
    mu, x0, b_mu, b_x0, n, S = mu_oracle_and_bound(eu, et, x, coef, g, v, x0_prev)
    want = {"x0_out": (x0, b_x0)}
    if mode == 0:
        t = target.double()
        want["resid"] = (t - mu, b_mu + U * (t.abs() + mu.abs()))
        want["out"] = (t, 3 * U * (t.abs() + mu.abs()))
        return want
    r = resid.double()
    e, b_e = mu + r, (n + 1) * U * (S + r.abs())
    if mask is None:
        want["out"] = (e, b_e)
        return want
    k, m = keep.double(), mask.double()
    ref = torch.where(m == 0, k, torch.where(m == 1, e, k + m * (e - k)))
    bound = torch.where(m == 0, torch.zeros_like(k), torch.where(m == 1, b_e, m * b_e + 4 * U * (k.abs() + m * (e - k).abs())))
    want["out"] = (ref, bound)
    return want


def step_restate(eu, et, x, coef, g, v, mode, x0_prev=None, target=None, resid=None, keep=None, mask=None):
    """The kernel's fp32 operations in its order, one tensor operation each: {x0_out, out, resid}"""
    mu, x0 = ddpm_mu2_reference(eu, et, x, coef, g, v, torch.float32, x0_prev)
    r = target.float() - mu if mode == 0 else resid.float()
    o = mu + r
    if mask is not None:
        o = blend_reference(o, keep, mask, torch.float32)
    return {"x0_out": x0, "out": o, "resid": r}


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements; an element whose bound is 0 must be equal (ratio 0, else inf)"""
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(ratio.max())
