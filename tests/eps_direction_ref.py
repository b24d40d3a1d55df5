"""slh_direction_threshold / slh_eps_direction (include/sliders_hip.h) restated for the tests: the integer keys and thresholds, the
float64 oracle, the first-order bound, the kernel's fp32 operations in its order, and wrong kernels.

Per element, with d_k = e+_k - e-_k and the terms k ascending that have c_k != 0 and are kept (key(d_k) >= tau):
    out = t + sum_k c_k d_k                       exact arithmetic, c_k the fp32 value the kernel reads
The kept set is part of the definition and is taken from the FP32 subtraction, as the kernel takes it: the truncated key of an inexact
difference may differ from the key of the exact one, and an element on the wrong side of tau would be an error of |c d|, not a rounding.

Bound, u = 2^-24.  The kernel rounds d = fl(e+ - e-) (error u |d|), p = fl(c d) (u |c d|, and |c| times d's error: 2 u |c d| together)
and every addition acc_j = fl(acc_(j-1) + p_j) (u |acc_j|).  To first order
    E = u sum_j (2 |c_j d_j| + |acc_j|)           acc_j the exact partial sums
and out is stored as bf16: + half a bf16 ulp of out.  An element without a kept term has E = 0 and out = t's bits.  Everything is
asserted at 1.01 x, which pays for the second-order terms.
"""
import torch

from tests.latent_blend_ref import worst_ratio  # noqa: F401  (shared by the tests of this kernel)

U = 2.0 ** -24
MUTANTS = ("swap_pos_neg", "threshold_per_sample", "n_keep_off_by_one", "strict_greater", "zero_multiplied", "key_from_rounding")


def diff32(pos, neg):
    """one fp32 subtraction of the widened values"""
    return pos.reshape(-1).float() - neg.reshape(-1).float()


def key_of(d32, rounded=False):
    """upper 16 bits of the fp32 bit pattern of |d| (int32); rounded: the bits of the bf16 ROUNDING of |d| instead (a mutant)"""
    if rounded:
        return d32.abs().to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF
    return (d32.contiguous().view(torch.int32) & 0x7FFFFFFF) >> 16


def thresholds(keys, n_keep, nb, chw, hw, per_sample=False):
    """tau [nb][chw / hw]: the n_keep-th largest key of every group, counted with multiplicity; per_sample (a mutant): one threshold
    over a sample's chw elements, keeping the same share"""
    C = chw // hw
    if per_sample:
        srt = keys.reshape(nb, chw).sort(dim=1, descending=True).values
        return srt[:, n_keep * C - 1].reshape(nb, 1).expand(nb, C).contiguous()
    srt = keys.reshape(nb, C, hw).sort(dim=2, descending=True).values
    return srt[:, :, n_keep - 1].contiguous()


def expand_thr(tau, nb, chw, hw):
    """[nb][C] -> [nb * chw]"""
    return tau.reshape(nb, chw // hw, 1).expand(nb, chw // hw, hw).reshape(-1)


def kept(pos, neg, n_keep, nb, chw, hw, mutant=None):
    """(keep [nb * chw] bool, tau [nb][C] int32) of one direction; n_keep None: everything is kept, tau = 0"""
    d = diff32(pos, neg)
    keys = key_of(d, rounded=mutant == "key_from_rounding")
    if n_keep is None:
        return torch.ones_like(keys, dtype=torch.bool), torch.zeros(nb, chw // hw, dtype=torch.int32)
    if mutant == "n_keep_off_by_one":
        n_keep = min(hw, n_keep + 1)
    tau = thresholds(keys, n_keep, nb, chw, hw, per_sample=mutant == "threshold_per_sample")
    t = expand_thr(tau, nb, chw, hw)
    return (keys > t if mutant == "strict_greater" else keys >= t), tau


def _c32(c):
    return [float(torch.tensor(float(v), dtype=torch.float32)) for v in c]


def oracle_and_bound(t, pos, neg, c, n_keep, nb, chw, hw):
    """float64 (out, E) over flat [nb * chw] bf16 inputs; pos, neg: K tensors; c: K coefficients; n_keep: K counts or None (no thr)"""
    acc = t.reshape(-1).double()
    e = torch.zeros_like(acc)
    any_term = torch.zeros_like(acc, dtype=torch.bool)
    for k, ck in enumerate(_c32(c)):
        if ck == 0.0:
            continue
        keep, _ = kept(pos[k], neg[k], None if n_keep is None else n_keep[k], nb, chw, hw)
        p = ck * (pos[k].reshape(-1).double() - neg[k].reshape(-1).double())
        p = torch.where(keep, p, torch.zeros_like(p))            # (a select: NaN in a dropped element stays out)
        acc = acc + p
        e = e + torch.where(keep, U * (2 * p.abs() + acc.abs()), torch.zeros_like(p))
        any_term |= keep
    _, ex = torch.frexp(acc.abs())                               # |out| = f 2^ex, f in [0.5, 1): 8 significant bits end at 2^(ex - 8)
    half_ulp = torch.where(acc == 0, torch.zeros_like(acc), torch.ldexp(torch.ones_like(acc), ex - 9))
    return acc, torch.where(any_term, e + half_ulp, torch.zeros_like(acc))


def restate(t, pos, neg, c, n_keep, nb, chw, hw, mutant=None):
    """The kernels' operations in fp32, one tensor operation (one rounding) each -> out (bf16); mutant: one of MUTANTS, a wrong kernel"""
    acc = t.reshape(-1).float()
    for k, ck in enumerate(_c32(c)):
        if ck == 0.0 and mutant != "zero_multiplied":
            continue
        a, b = (neg[k], pos[k]) if mutant == "swap_pos_neg" else (pos[k], neg[k])
        keep, _ = kept(a, b, None if n_keep is None else n_keep[k], nb, chw, hw, mutant)
        p = torch.tensor(ck, dtype=torch.float32) * diff32(a, b)
        acc = torch.where(keep, acc + p, acc)
    return acc.to(torch.bfloat16)
