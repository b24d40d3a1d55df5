"""slh_xattn_map element by element: the cases, the input classes, the float64 reference with its per-element bound, and a plain-torch
fp32 stand-in of the kernel's arithmetic with the mutants the bound must catch (tests/test_xattn_map_host.py proves that on the CPU,
tests/test_xattn_map_gpu.py runs the same cases on the device; docs/EDIT.md "A mask from a word" has the derivation in words).

The kernel (csrc/xattn_map.hip), per collected sample b, query row i and head h, all in fp32 from bf16 q and k:
    s_j  = scale * dot(q_i, k_j)                        fma chains over d, then one multiply
    keys in blocks of 8:  mn = max(m, max_block s);  alpha = exp(m - mn);  e_j = exp(s_j - mn)
                          l = l * alpha + sum e_j;  a = a * alpha + sum wt_j e_j;  m = mn
    r_h  = a / l
    term = coef * (r_0 + r_1 + ... in ascending h);   out = term, or out + term with accumulate

The bound, u = 2^-24, gamma_n = n u / (1 - n u), everything evaluated in float64 on the same bf16 inputs and the fp32 values of scale / coef:
    delta_j <= gamma_{D+2} |scale| sum_d |q_d| |k_d|      (D products and adds in any order, the multiply by scale);  Delta = max_j delta_j
    softmax of the computed logits:  |p^_j - p_j| <= p_j expm1(2 Delta)
    every e_j reaches the final sums as exp(s^_j - M^) (1 + eta_j): the arguments of its own exponential and of the alpha links after it
    telescope to X_j = M - s_j (+ 2 Delta), each argument is rounded once by the subtraction and twice inside exp (x * log2(e), the
    constant and the product), v_exp_f32 is good to one ulp = 2 u, and there are at most nblk = ceil(Tk / 8) links besides its own:
        eps_j = 3 u (X_j + 2 Delta) + 2 u (1 + nblk)
    the sums l and a round each term at most 7 + nblk times (7 adds inside a block, one fma per block); the division rounds once (2 u allowed);
    the denominator's relative error is the p-weighted mean of the terms', Ebar = sum_j p_j (eps_j + gamma_{7+nblk}):
        E_h = sum_j |wt_j| p_j (expm1(2 Delta) + eps_j + Ebar + 2 gamma_{7+nblk} + 2 u) + 2^-120 sum_j |wt_j|     (results flushed below 2^-126)
    the head sum is H - 1 adds and the multiply by coef, on |r_h| <= A_h = sum_j |wt_j| p_j:
        |term - ref| <= coef (1.01 sum_h E_h + (H + 1) u sum_h A_h)          (1.01: the products of the first-order terms, all below 1e-2)
    accumulate: one more rounding of the sum, u (|ref out| + the bound so far).
No constant is fitted to a device."""
import itertools
import math
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

U = 2.0 ** -24
KB = 8
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
FENCE = 4096

CLASSES = ("normal", "peak_in", "peak_out", "shift", "last", "zeroq")
WT_KINDS = ("onehot", "ones", "signed")
MUTANTS = ("pad_denominator", "no_scale", "head_sum", "head0_columns", "wt_row0", "ignore_accumulate")


@dataclass(frozen=True)
class Case:
    Tq: int
    Tk: int
    D: int
    H: int
    b0: int
    nb: int
    ldk_mult: int          # 3: k is the middle third of a [B][Tk][3 H D] buffer (a column view); 1: ldk = H D
    ldq_pad: int           # ldq = H D + ldq_pad
    acc: int
    cls: str
    wt: str
    B: int = 2

    @property
    def id(self) -> str:
        return (f"Tq{self.Tq}-Tk{self.Tk}-D{self.D}-H{self.H}-b{self.b0}n{self.nb}-ldk{self.ldk_mult}-q{self.ldq_pad}-acc{self.acc}-"
                f"{self.cls}-{self.wt}")

    @property
    def layers(self) -> int:
        return 3            # coef = 1 / (H * 3): a level of three layers

    @property
    def peak(self) -> int:
        return self.Tk - 1 if self.cls == "last" else self.Tk // 2


def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=F64).to(F32))


def scale_of(c: Case) -> float:
    return _f32(c.D ** -0.5)


def coef_of(c: Case) -> float:
    return _f32(1.0 / (c.H * c.layers))


def _cases() -> List[Case]:
    Tqs, Tks, Ds, Hs = (1, 63, 64, 65, 256), (1, 64, 65, 77, 128), (8, 40, 64, 160), (1, 2, 5)
    out = []

    def add(Tq, Tk, D, H, i, cls, wt):
        if Tk == 1 and cls in ("peak_in", "peak_out", "last"):
            cls = "normal"               # one key: nothing to lead
        if cls in ("peak_in", "peak_out"):
            wt = "onehot"                # the weighted set is the peak (in) or its neighbour (out)
        b0, nb = ((1, 1), (0, 2))[i % 2]
        out.append(Case(Tq, Tk, D, H, b0, nb, (3, 1)[(i // 2) % 2], (0, 8)[(i // 4) % 2], (0, 1)[(i // 3) % 2], cls, wt))
    # every (Tq, Tk, D), the other parameters cycling with coprime periods
    for i, (Tq, Tk, D) in enumerate(itertools.product(Tqs, Tks, Ds)):
        add(Tq, Tk, D, Hs[i % 3], i, CLASSES[i % len(CLASSES)], WT_KINDS[(i // len(CLASSES)) % 3])
    # every class with every weight kind at the text shape, every H with every D, both sample selections
    for i, (cls, wt) in enumerate(itertools.product(CLASSES, WT_KINDS)):
        add(65, 77, 64, Hs[i % 3], i, cls, wt)
    for i, (D, H) in enumerate(itertools.product(Ds, Hs)):
        add(63, 77, D, H, i + 1, CLASSES[(i + 2) % len(CLASSES)], WT_KINDS[i % 3])
    # all-zero q and all-ones weights at every key count (the closed forms), with accumulate on and off
    for i, Tk in enumerate(Tks):
        add(64, Tk, 40, 5, i, "zeroq", "signed")
        add(65, Tk, 64, 2, i + 1, "normal", "ones")
    seen, uniq = set(), []
    for c in out:
        if c.id not in seen:
            seen.add(c.id)
            uniq.append(c)
    return uniq


CASES = _cases()


# ---------------------------------------------------------------------------------------------------------------------------
# inputs (made on the CPU: the same values on every device)
# ---------------------------------------------------------------------------------------------------------------------------
def inputs(c: Case, seed: int) -> Dict[str, torch.Tensor]:
    """q [B][Tq][H D], k [B][Tk][H D] (bf16 values), wt [nb][Tk], prior [nb][Tq] (fp32)"""
    g = torch.Generator().manual_seed(seed)
    B, H, D, Tq, Tk = c.B, c.H, c.D, c.Tq, c.Tk
    q = torch.randn(B, Tq, H, D, generator=g)
    k = torch.randn(B, Tk, H, D, generator=g)
    a = 2.0
    lead = torch.zeros(Tk)
    if c.cls in ("peak_in", "peak_out"):
        lead[c.peak] = 60.0
    elif c.cls == "shift":
        lead[:] = 80.0
    elif c.cls == "last":
        lead = 60.0 * torch.arange(Tk, dtype=F32) / max(1, Tk - 1)        # the maximum moves in every block and ends on the last key
    if c.cls == "zeroq":
        q.zero_()
    elif bool((lead != 0).any()):
        q += a
        k += (lead / (c.D ** -0.5 * D * a)).reshape(1, Tk, 1, 1)
    if c.wt == "ones":
        wt = torch.ones(c.nb, Tk)
    elif c.wt == "signed":
        wt = torch.randn(c.nb, Tk, generator=g)
    else:
        wt = torch.zeros(c.nb, Tk)
        j = (c.peak + 1) % Tk if c.cls == "peak_out" else c.peak
        wt[:, j] = 1.0
    prior = torch.randn(c.nb, Tq, generator=g)
    return dict(q=q.reshape(B, Tq, H * D).to(BF), k=k.reshape(B, Tk, H * D).to(BF), wt=wt.to(F32), prior=prior.to(F32))


# ---------------------------------------------------------------------------------------------------------------------------
# float64 reference and the bound
# ---------------------------------------------------------------------------------------------------------------------------
def gamma(n: float) -> float:
    return n * U / (1.0 - n * U)


def reference(c: Case, L: Dict[str, torch.Tensor]):
    """-> (ref out [nb][Tq], bound [nb][Tq]) float64"""
    B, H, D, Tq, Tk = c.B, c.H, c.D, c.Tq, c.Tk
    scale, coef = scale_of(c), coef_of(c)
    nblk = (Tk + KB - 1) // KB
    gs = gamma(7 + nblk)
    q = L["q"].to(F64).reshape(B, Tq, H, D)[c.b0:c.b0 + c.nb].permute(0, 2, 1, 3)       # [nb][H][Tq][D]
    k = L["k"].to(F64).reshape(B, Tk, H, D)[c.b0:c.b0 + c.nb].permute(0, 2, 1, 3)
    wt = L["wt"].to(F64)[:, None, None, :]                                               # [nb][1][1][Tk]
    S = scale * (q @ k.transpose(-1, -2))                                                # [nb][H][Tq][Tk]
    delta = gamma(D + 2) * abs(scale) * (q.abs() @ k.abs().transpose(-1, -2))
    Delta = delta.amax(dim=-1, keepdim=True)
    P = torch.softmax(S, dim=-1)
    X = S.amax(dim=-1, keepdim=True) - S
    eps = 3 * U * (X + 2 * Delta) + 2 * U * (1 + nblk)
    Ebar = (P * (eps + gs)).sum(dim=-1, keepdim=True)
    A = (wt.abs() * P).sum(dim=-1)                                                       # [nb][H][Tq]
    E = (wt.abs() * P * (torch.expm1(2 * Delta) + eps + Ebar + 2 * gs + 2 * U)).sum(dim=-1) + 2.0 ** -120 * wt.abs().sum(dim=-1)
    term = coef * (wt * P).sum(dim=-1).sum(dim=1)
    bound = coef * (1.01 * E.sum(dim=1) + (H + 1) * U * A.sum(dim=1))
    if c.acc:
        ref = L["prior"].to(F64) + term
        bound = bound + U * (ref.abs() + bound)
    else:
        ref = term
    return ref, bound


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel's arithmetic in plain torch fp32, and its mutants
# ---------------------------------------------------------------------------------------------------------------------------
def standin(c: Case, L: Dict[str, torch.Tensor], mutant: Optional[str] = None) -> torch.Tensor:
    """fp32 [nb][Tq]: one tensor operation per operation of the kernel, in its order where the order matters (the key blocks, the
    heads); the dot products are one fp32 matmul (the bound does not depend on their order)"""
    assert mutant is None or mutant in MUTANTS
    B, H, D, Tq, Tk = c.B, c.H, c.D, c.Tq, c.Tk
    scale = torch.tensor(1.0 if mutant == "no_scale" else scale_of(c), dtype=F32)
    coef = torch.tensor(coef_of(c) * (H if mutant == "head_sum" else 1), dtype=F32)
    q = L["q"].to(F32).reshape(B, Tq, H, D)[c.b0:c.b0 + c.nb]
    k = L["k"].to(F32).reshape(B, Tk, H, D)[c.b0:c.b0 + c.nb]
    wt = L["wt"].to(F32)
    if mutant == "wt_row0":
        wt = wt[:1].expand(c.nb, Tk)
    Tkd = Tk
    if mutant == "pad_denominator":        # the keys of a 96 / 128 wide tile past Tk are counted (zero rows of k: logit 0, weight 0)
        Tkd = 96 if Tk <= 96 else 128
        k = torch.cat([k, torch.zeros(c.nb, Tkd - Tk, H, D)], dim=1)
        wt = torch.cat([wt, torch.zeros(c.nb, Tkd - Tk)], dim=1)
    tot = torch.zeros(c.nb, Tq, dtype=F32)
    for h in range(H):
        kh = k[:, :, 0 if mutant == "head0_columns" else h]
        s = (q[:, :, h] @ kh.transpose(-1, -2)) * scale                    # [nb][Tq][Tkd]
        m = torch.full((c.nb, Tq), -math.inf, dtype=F32)
        l = torch.zeros(c.nb, Tq, dtype=F32)
        a = torch.zeros(c.nb, Tq, dtype=F32)
        for j0 in range(0, Tkd, KB):
            blk = s[:, :, j0:j0 + KB]
            mn = torch.maximum(m, blk.amax(dim=-1))
            alpha = torch.exp(m - mn)
            ls = torch.zeros_like(l)
            as_ = torch.zeros_like(a)
            for jj in range(blk.shape[-1]):
                e = torch.exp(blk[:, :, jj] - mn)
                ls = ls + e
                as_ = as_ + wt[:, None, j0 + jj] * e
            l = l * alpha + ls
            a = a * alpha + as_
            m = mn
        tot = tot + a / l
    term = coef * tot
    return L["prior"] + term if c.acc and mutant != "ignore_accumulate" else term


def closed_form(c: Case, L: Dict[str, torch.Tensor]) -> Optional[torch.Tensor]:
    """The term where it is known without a softmax: all-ones weights give coef H, all-zero q gives coef H sum(wt) / Tk (float64
    [nb][Tq], the prior added with accumulate); None for every other case"""
    if c.wt == "ones":
        t = torch.full((c.nb, c.Tq), coef_of(c) * c.H, dtype=F64)
    elif c.cls == "zeroq":
        t = (coef_of(c) * c.H * L["wt"].to(F64).sum(dim=1) / c.Tk)[:, None].expand(c.nb, c.Tq)
    else:
        return None
    return L["prior"].to(F64) + t if c.acc else t


# ---------------------------------------------------------------------------------------------------------------------------
# device buffers: one pattern-filled allocation, 4 KiB fences, NaN where nothing may be read
# ---------------------------------------------------------------------------------------------------------------------------
class Arena:
    """q, k, wt, out in one 0xA5-filled allocation with fences between them.  q carries ldq_pad NaN columns, k sits in the middle
    third of its rows with NaN in the other two (ldk_mult 3); out starts as NaN, or as the prior with accumulate."""

    def __init__(self, c: Case, L: Dict[str, torch.Tensor], dev):
        HD = c.H * c.D
        self.ldq, self.ldk = HD + c.ldq_pad, HD * c.ldk_mult
        self.kcol = HD if c.ldk_mult == 3 else 0
        sizes = dict(q=c.B * c.Tq * self.ldq * 2, k=c.B * c.Tk * self.ldk * 2, wt=c.nb * c.Tk * 4, out=c.nb * c.Tq * 4)
        self.off, at = {}, FENCE
        for n, sz in sizes.items():
            self.off[n] = at
            at += (sz + 255) // 256 * 256 + FENCE
        self.sizes = sizes
        self.mem = torch.full((at,), 0xA5, dtype=torch.uint8, device=dev)
        nan = float("nan")
        qf = torch.full((c.B, c.Tq, self.ldq), nan, dtype=BF)
        qf[:, :, :HD] = L["q"]
        kf = torch.full((c.B, c.Tk, self.ldk), nan, dtype=BF)
        kf[:, :, self.kcol:self.kcol + HD] = L["k"]
        self._put("q", qf)
        self._put("k", kf)
        self._put("wt", L["wt"])
        self.start = L["prior"] if c.acc else torch.full((c.nb, c.Tq), nan, dtype=F32)
        self.reset()
        self.snap = self.mem.clone()
        self.c = c

    def _put(self, name, t):
        raw = t.contiguous().view(torch.uint8).reshape(-1)
        self.mem[self.off[name]:self.off[name] + raw.numel()] = raw.to(self.mem.device)

    def reset(self):
        self._put("out", self.start)

    def ptr(self, name) -> int:
        return self.mem.data_ptr() + self.off[name]

    def out(self) -> torch.Tensor:
        o, n = self.off["out"], self.sizes["out"]
        return self.mem[o:o + n].clone().view(F32).reshape(self.start.shape).cpu()

    def untouched_outside_out(self) -> bool:
        o, n = self.off["out"], self.sizes["out"]
        return torch.equal(self.mem[:o], self.snap[:o]) and torch.equal(self.mem[o + n:], self.snap[o + n:])

    def desc(self, lib):
        c = self.c
        return lib.XattnMapDesc(q=self.ptr("q"), k=self.ptr("k") + 2 * self.kcol, wt=self.ptr("wt"), out=self.ptr("out"), B=c.B, b0=c.b0,
                                nb=c.nb, H=c.H, D=c.D, Tq=c.Tq, Tk=c.Tk, ldq=self.ldq, ldk=self.ldk, scale=scale_of(c), coef=coef_of(c),
                                accumulate=c.acc)
