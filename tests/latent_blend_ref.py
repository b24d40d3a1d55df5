"""slh_latent_blend (include/sliders_hip.h) restated for the tests: the float64 oracle, the first-order bound, the kernel's fp32
operations in its order (edit.blend_reference, the restatement the masked editor already uses), and wrong kernels.

Bound, u = 2^-24, with k = keep, m = mask and out = k + m (e - k) in exact arithmetic.  The kernel rounds three times where 0 < m < 1:
d = fl(e - k), p = fl(m d), out = fl(k + p).  To first order the error of d (u |e - k|) and of p (u |m| |e - k|) reach out multiplied by
m resp. 1, and the last addition adds u |out|:
    E_out = u (|out| + 2 |m| |e - k|)               (m <= 1; m = 0 and m = 1 are selects: exact)
dtype 0 stores the bf16 rounding of that: + half a bf16 ulp of out.  dtype 1's copies are rne(fl(out * s_next)):
    E_in  = |s_next| E_out + u |out * s_next|       before the bf16 rounding
Everything is asserted at 1.01 x, which pays for the second-order terms.
"""
import torch

from sliders_amd.edit import blend_reference

U = 2.0 ** -24
MUTANTS = ("mask_per_element", "swap_e_keep", "one_minus_m", "wrong_s_next", "mask_per_channel_pixel")


def expand_mask(mask, nb, chw, hw):
    """[nb * hw] -> [nb * chw]: the value of pixel i % hw of sample b at every channel"""
    return mask.reshape(nb, 1, hw).expand(nb, chw // hw, hw).reshape(-1)


def oracle(e, keep, mask, nb, chw, hw, s_next=1.0):
    """float64: (out, out * s_next) over flat [nb * chw] inputs (any float dtype: they widen exactly) and a flat [nb * hw] mask"""
    out = blend_reference(e.reshape(-1), keep.reshape(-1), expand_mask(mask, nb, chw, hw), torch.float64)
    return out, out * float(s_next)


def bound(e, keep, mask, nb, chw, hw, s_next=1.0, bf16_out=False):
    """(E_out, E_in) of the module docstring, float64; bf16_out: dtype 0, E_out includes the half ulp of the stored bf16 and E_in is it"""
    e64, k64, m64 = e.reshape(-1).double(), keep.reshape(-1).double(), expand_mask(mask, nb, chw, hw).double()
    out, scaled = oracle(e, keep, mask, nb, chw, hw, s_next)
    lerp = (m64 != 0) & (m64 != 1)
    # a select is exact; where NaN sits on the unselected side the difference is NaN and must not enter the bound
    diff = torch.where(lerp, (e64 - k64).abs(), torch.zeros_like(out))
    e_out = torch.where(lerp, U * (out.abs() + 2 * m64.abs() * diff), torch.zeros_like(out))
    e_in = abs(float(s_next)) * e_out + U * scaled.abs()
    if bf16_out:
        _, ex = torch.frexp(out.abs())                     # |out| = f 2^ex, f in [0.5, 1): 8 significant bits end at 2^(ex - 8)
        e_out = e_out + torch.where(out == 0, torch.zeros_like(out), torch.ldexp(torch.ones_like(out), ex - 9))
        e_in = e_out                                       # the copies are out's bits (s_next is not read)
    return e_out, e_in


def restate(e, keep, mask, nb, chw, hw, s_next=1.0, bf16_out=False, mutant=None):
    """The kernel's operations in fp32, one tensor operation (one rounding) each -> (out, the scaled input before its bf16 rounding);
    mutant: one of MUTANTS, a wrong kernel"""
    n = nb * chw
    e32, k32 = e.reshape(-1).float(), keep.reshape(-1).float()
    m = expand_mask(mask, nb, chw, hw).float()
    if mutant == "mask_per_element":               # the element index, not the pixel's, into the mask
        m = mask.float()[torch.arange(n) % (nb * hw)]
    elif mutant == "mask_per_channel_pixel":       # i % hw without the sample's offset b * hw
        m = mask.float()[torch.arange(n) % hw]
    elif mutant == "swap_e_keep":
        e32, k32 = k32, e32
    elif mutant == "one_minus_m":
        m = 1.0 - m
    elif mutant is not None and mutant != "wrong_s_next":
        raise ValueError(mutant)
    out = blend_reference(e32, k32, m, torch.float32)
    if bf16_out:
        out = out.to(torch.bfloat16).float()
    s = torch.tensor(float(s_next), dtype=torch.float32)
    if mutant == "wrong_s_next":                   # the scale of another row
        s = s * 0.75
    return out, out * s


def worst_ratio(got, ref, bnd):
    """max |got - ref| / bnd; where the bound is 0 (a select) the values must be equal.  NaN anywhere -> inf"""
    err = (got.double() - ref).abs()
    if bool(torch.isnan(err).any()):
        return float("inf")
    zero = bnd == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / bnd[~zero]).max())
