"""What tests/test_sigma_step_host.py and tests/test_sigma_step_gpu.py share (docs/SAMPLING.md, "Fused fp32 step"):

restate   the arithmetic of slh_sigma_step (csrc/sigma_step.hip) as plain torch tensor ops in the kernel's operation order - in fp32 the
          stand-in of the kernel (one rounding per operation: every torch op is its own loop, nothing is contracted), in float64 the
          reference - and its mutants;
bound     the per-element first-order bound of the fp32 arithmetic against float64 on the same inputs;
dpmpp_2m_oracle   DPM-Solver++(2M) in float64, in the paper's own variables (alpha_t, sigma_t, lambda_t of the variance-preserving
          process), not the sigma-space coefficients of schedulers.step_row.

The bound.  u = 2^-24; the inputs (bf16 epsilon halves, fp32 x / H / noise, fp32 coefficients) are exact in both computations.

    m   = fl(u_ + fl(g fl(t_ - u_)))         |dm|   <= u (|m| + 2 |g| |t_ - u_|)                        =: E_m     (single branch: 0)
    x0  = fl(fl(p x) + fl(q m))              |dx0|  <= u (|x0| + |p x| + |q m|) + |q| E_m               =: E_x0
    H0  = fl(fl(x - x0) / sigma)   kind 0    |dH0|  <= (u |x - x0| + E_x0) / |sigma| + u |H0|           =: E_H
        = x0                       kind 1    |dH0|  <= E_x0
    out = a x + c0 H0 + ... summed left to right over T terms: T product roundings and T - 1 additions, every partial sum
          within S = sum |term|:             |dout| <= u S + (T - 1) u S + |c0| E_H = T u S + |c0| E_H  =: E_out
    in  = fl(out s_next), before its bf16 rounding:   |din| <= |s_next| E_out + u |out s_next|

The kind-0 line is where the division by sigma follows the cancellation in x - x0: x0 is within E_x0 ~ u |x| of exact while x - x0 is
only ~ sigma |m| large, so the derivative carries u |x| / sigma - which the step multiplies by |c0| <= sigma again.  FIRST_ORDER = 1.01
covers the products of first-order terms (all below 1e-5), as in docs/EDIT.md.  Nothing is fitted.
"""
import math

import torch

U = 2.0 ** -24
FIRST_ORDER = 1.01
MUTANTS = ("cfg_swapped", "pq_swapped", "history_newest_last", "cn_dropped", "s_next_from_sigma", "kind_ignored")


def restate(u, t, x, H, noise, row, g, dtype=torch.float32, mutant=None):
    """(out, H0, out * s_next) of slh_sigma_step in `dtype`, the kernel's operations in the kernel's order.  u, t: the epsilon halves
    (t None: the single branch); H: the history tensors H[1..], newest first, len(H) >= row.n_hist; noise: a tensor or None; row: a
    schedulers.StepRow (or anything with its fields) holding fp32-valued python floats."""
    c = lambda v: v.to(dtype)
    u_, x_ = c(u), c(x)
    t_ = None if t is None else c(t)
    if mutant == "cfg_swapped" and t is not None:
        u_, t_ = t_, u_
    m = u_ if t_ is None else u_ + g * (t_ - u_)
    p, q = (row.q, row.p) if mutant == "pq_swapped" else (row.p, row.q)
    x0 = p * x_ + q * m
    kind = 1 - row.kind if mutant == "kind_ignored" else row.kind       # a kernel without the branch takes the other one somewhere
    h0 = (x_ - x0) / (row.sigma if row.sigma != 0.0 else 1.0) if kind == 0 else x0
    acc = row.a * x_
    acc = acc + row.c[0] * h0
    hist = [c(h) for h in H[:row.n_hist]]
    if mutant == "history_newest_last":
        hist = hist[::-1]
    for k, h in enumerate(hist):
        acc = acc + row.c[k + 1] * h
    if noise is not None and mutant != "cn_dropped":
        acc = acc + row.c_n * c(noise)
    s_next = row.s_next
    if mutant == "s_next_from_sigma":
        s_next = float(torch.tensor(1.0 / math.sqrt(row.sigma ** 2 + 1.0), dtype=torch.float32))
    return acc, h0, acc * s_next


def bound(u, t, x, H, noise, row, g):
    """float64 reference (out, H0, in) and the bounds (E_out, E_H, E_in) of the module docstring, per element"""
    d = lambda v: v.double()
    u_, x_ = d(u), d(x)
    if t is None:
        m, e_m = u_, torch.zeros_like(u_)
    else:
        dt = d(t) - u_
        m = u_ + g * dt
        e_m = U * (m.abs() + 2 * abs(g) * dt.abs())
    px, qm = row.p * x_, row.q * m
    x0 = px + qm
    e_x0 = U * (x0.abs() + px.abs() + qm.abs()) + abs(row.q) * e_m
    if row.kind == 0:
        diff = x_ - x0
        h0 = diff / row.sigma
        e_h = (U * diff.abs() + e_x0) / abs(row.sigma) + U * h0.abs()
    else:
        h0, e_h = x0, e_x0
    terms = [row.a * x_, row.c[0] * h0] + [row.c[k + 1] * d(H[k]) for k in range(row.n_hist)]
    if noise is not None:
        terms.append(row.c_n * d(noise))
    out = sum(terms[1:], terms[0])
    S = sum(v.abs() for v in terms)
    e_out = len(terms) * U * S + abs(row.c[0]) * e_h
    e_in = abs(row.s_next) * e_out + U * (out * row.s_next).abs()
    return (out, h0, out * row.s_next), tuple(FIRST_ORDER * e for e in (e_out, e_h, e_in))


def worst_ratio(got, ref, bnd) -> float:
    """max |got - ref| / bound over the elements; inf where an element with a zero bound is not exact"""
    err = (got.double() - ref).abs()
    if bool(((bnd == 0) & (err > 0)).any()) or not bool(torch.isfinite(err).all()):
        return math.inf
    nz = bnd > 0
    return float((err[nz] / bnd[nz]).max()) if bool(nz.any()) else 0.0


def dpmpp_2m_oracle(sigmas, x, denoise):
    """DPM-Solver++(2M), Algorithm 2 of Lu et al. 2022, float64, in the paper's variables.  The sigma-space latent x (variance
    exploding) is x / sqrt(sigma^2 + 1) of the variance-preserving process with alpha_t = 1 / sqrt(sigma^2 + 1), sigma_t = sigma alpha_t,
    lambda_t = ln(alpha_t / sigma_t):

        xbar_i = (sigma_t_i / sigma_t_{i-1}) xbar_{i-1} - alpha_t_i (exp(-h_i) - 1) D_i,      h_i = lambda_i - lambda_{i-1}
        D_i    = (1 + 1 / (2 r_i)) x0_{i-1} - (1 / (2 r_i)) x0_{i-2},  r_i = h_{i-1} / h_i;   D_i = x0_{i-1} on the first step and on
                                                                                              a step that ends at sigma = 0
    sigmas: the grid, python floats, ending with 0 or not; denoise(x, i) -> the predicted clean sample at step i (float64 tensor).
    Returns the list of the latents after every step."""
    alpha = [1.0 / math.sqrt(s * s + 1.0) for s in sigmas]
    sig_t = [s * a for s, a in zip(sigmas, alpha)]
    lam = [math.log(a / s) if s > 0 else math.inf for a, s in zip(alpha, sig_t)]
    xbar = x.double() * alpha[0]
    old, out = None, []
    for i in range(1, len(sigmas)):
        x0 = denoise(xbar / alpha[i - 1], i - 1)
        h = lam[i] - lam[i - 1]
        if old is None or sigmas[i] == 0.0:
            D = x0
        else:
            r = (lam[i - 1] - lam[i - 2]) / h
            D = (1 + 1 / (2 * r)) * x0 - (1 / (2 * r)) * old
        xbar = (sig_t[i] / sig_t[i - 1]) * xbar - alpha[i] * (math.exp(-h) - 1.0) * D
        old = x0
        out.append(xbar / alpha[i])
    return out
