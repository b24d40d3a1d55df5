"""slh_eps_direction_momentum (include/sliders_hip.h) restated for the tests: the float64 oracle, the first-order bound, the kernel's fp32
operations in its order, and wrong kernels.  The keys, thresholds and kept sets are those of tests/eps_direction_ref.py.

Per element, with d_k = e+_k - e-_k, the terms k ascending that have c_k != 0 and are kept, and nu the state read from mom_in:
    G    = sum_k c_k d_k + s_m nu
    out  = t + G                                  exact arithmetic; c_k, s_m, beta, omb the fp32 values the kernel reads
    nu'  = beta nu + omb G                        (omb is an input of its own: the oracle does not form 1 - beta)
The kept set is taken from the fp32 subtraction, as in tests/eps_direction_ref.py.

Bound, u = 2^-24.  The kernel rounds d_j (u |d_j|), p_j = fl(c_j d_j) (2 u |c_j d_j| with d's error), q = fl(s_m nu) (u |q|), and every
addition.  acc_j = fl(acc_(j-1) + p_j) and the last one, fl(acc + q), cost u times their result; g_1 = fl(+0 + p_1) is exact, so only
the partial sums g_j, j >= 2, and gm = fl(g + q) cost theirs.  a = fl(beta nu), b = fl(omb gm) and nu' = fl(a + b) cost u times their
results, and gm's error reaches nu' through omb.  To first order, over the exact partial sums
    E_out = u [ sum_j (2 |c_j d_j| + |acc_j|) + |q| + |acc_final| ] + half a bf16 ulp of out
    E_nu' = u [ |a| + |b| + |nu'| ] + |omb| u [ sum_j 2 |c_j d_j| + sum_(j>=2) |g_j| + |q| + |gm| ]
An element with no kept term and nu == 0 has out == t, nu' == 0 and both bounds 0.  Asserted at 1.01 x, which pays for the second order.
"""
import torch

from tests.eps_direction_ref import U, _c32, diff32, kept
from tests.latent_blend_ref import worst_ratio  # noqa: F401  (shared by the tests of this kernel)

MUTANTS = ("nu_from_g", "beta_omb_swapped", "out_without_momentum", "q_twice", "momentum_where_kept", "omb_in_kernel")


def f32(v):
    """the fp32 rounding of a Python float, as a Python float"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def omb_of(beta):
    """what the host passes as omb: 1 - beta in double, rounded once"""
    return f32(1.0 - float(beta))


def oracle_and_bound(t, pos, neg, c, n_keep, nb, chw, hw, nu, s_m, beta, omb):
    """float64 (out, E_out, nu', E_nu') over flat [nb * chw] inputs: t, pos[k], neg[k] bf16, nu fp32; c: K coefficients; n_keep: K counts or
    None (no thr); s_m, beta, omb: taken at their fp32 values"""
    s_m, beta, omb = f32(s_m), f32(beta), f32(omb)
    acc = t.reshape(-1).double()
    nu = nu.reshape(-1).double()
    zero = torch.zeros_like(acc)
    g, e_out, e_g = zero.clone(), zero.clone(), zero.clone()
    n_kept = torch.zeros_like(acc, dtype=torch.int64)
    for k, ck in enumerate(_c32(c)):
        if ck == 0.0:
            continue
        keep, _ = kept(pos[k], neg[k], None if n_keep is None else n_keep[k], nb, chw, hw)
        p = ck * (pos[k].reshape(-1).double() - neg[k].reshape(-1).double())
        p = torch.where(keep, p, zero)                               # (a select: NaN in a dropped element stays out)
        acc, g = acc + p, g + p
        n_kept = n_kept + keep.long()
        e_out = e_out + torch.where(keep, U * (2 * p.abs() + acc.abs()), zero)
        e_g = e_g + torch.where(keep, U * 2 * p.abs(), zero) + torch.where(keep & (n_kept >= 2), U * g.abs(), zero)
    q = s_m * nu
    acc, gm = acc + q, g + q
    a, b = beta * nu, omb * gm
    nu_new = a + b
    live = (n_kept > 0) | (nu != 0)
    e_out = e_out + U * (q.abs() + acc.abs())
    e_g = e_g + U * (q.abs() + gm.abs())
    _, ex = torch.frexp(acc.abs())                                   # |out| = f 2^ex, f in [0.5, 1): 8 significant bits end at 2^(ex - 8)
    half_ulp = torch.where(acc == 0, zero, torch.ldexp(torch.ones_like(acc), ex - 9))
    e_nu = U * (a.abs() + b.abs() + nu_new.abs()) + abs(omb) * e_g
    return acc, torch.where(live, e_out + half_ulp, zero), nu_new, torch.where(live, e_nu, zero)


def restate(t, pos, neg, c, n_keep, nb, chw, hw, nu, s_m, beta, omb, mutant=None):
    """The kernel's operations in fp32, one tensor operation (one rounding) each -> (out bf16, nu' fp32); mutant: one of MUTANTS"""
    F = lambda v: torch.tensor(float(v), dtype=torch.float32)
    s_m, beta, omb = F(s_m), F(beta), F(omb)
    if mutant == "beta_omb_swapped":
        beta, omb = omb, beta
    if mutant == "omb_in_kernel":
        omb = F(1.0) - beta                                          # one fp32 subtraction of the rounded beta
    acc = t.reshape(-1).float()
    nu = nu.reshape(-1).float()
    g = torch.zeros_like(acc)
    any_kept = torch.zeros_like(acc, dtype=torch.bool)
    for k, ck in enumerate(_c32(c)):
        if ck == 0.0:
            continue
        keep, _ = kept(pos[k], neg[k], None if n_keep is None else n_keep[k], nb, chw, hw)
        p = F(ck) * diff32(pos[k], neg[k])
        acc = torch.where(keep, acc + p, acc)
        g = torch.where(keep, g + p, g)
        any_kept |= keep
    q = s_m * nu
    if mutant == "momentum_where_kept":
        q = torch.where(any_kept, q, torch.zeros_like(q))
    gm = g + q
    if mutant != "out_without_momentum":
        acc = acc + q
    if mutant == "q_twice":
        acc, gm = acc + q, gm + q
    a = beta * nu
    b = omb * (g if mutant == "nu_from_g" else gm)
    return acc.to(torch.bfloat16), a + b
