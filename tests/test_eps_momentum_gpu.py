"""slh_eps_direction_momentum on the MI355X (docs/SAMPLING.md, "Prompt-direction sampling"), through the C ABI: both outputs are within
the derived bounds of float64 (tests/eps_momentum_ref.py) and have the fp32 restatement's bits, in fenced NaN-prefilled buffers; every
case runs twice with a bit comparison.  The thresholds are slh_direction_threshold's, as in tests/test_eps_direction_gpu.py."""
import itertools

import pytest
import torch

from sliders_amd import lib
from tests.eps_direction_ref import diff32, kept
from tests.eps_momentum_ref import omb_of, oracle_and_bound, restate, worst_ratio
from tests.test_eps_direction_gpu import GUARD, C, Buffers, _bits
from tests.test_eps_direction_host import COEF, draw_rows
from tests.test_eps_momentum_host import MOMENTA, draw_nu

pytestmark = pytest.mark.gpu


class MomentumBuffers(Buffers):
    """Buffers plus the state: mom_in and mom_out as two rows of one NaN-prefilled fp32 device tensor, fenced and offset as the bf16
    rows are (off = 1: 4 bytes, so not 16-byte aligned); alias: mom_out is mom_in"""

    def __init__(self, dev, n, n_thr, K, off, t, pos, neg, nu, alias):
        super().__init__(dev, n, n_thr, K, off, t, pos, neg)
        self.alias = alias
        self.hf = torch.full((2, 2 * GUARD + (n + 1 + 7) // 8 * 8), float("nan"), dtype=torch.float32)
        self.state(self.hf, "mom_in")[:] = nu
        self.df = self.hf.to(dev)

    def state(self, tf, name):
        row = 0 if name == "mom_in" or self.alias else 1
        return tf[row, GUARD + self.off:GUARD + self.off + self.n]

    def state_ptr(self, name):
        row = 0 if name == "mom_in" or self.alias else 1
        return self.df[row].data_ptr() + (GUARD + self.off) * 4

    def combine_momentum(self, c, momentum, nb, chw, hw, thr):
        self.df.copy_(self.hf)           # (an aliased launch has overwritten its input)
        lib.eps_direction_momentum(torch.cuda.current_stream().cuda_stream, t=self.ptr("t"), out=self.ptr("out"), pos=self.rows("pos"),
                                   neg=self.rows("neg"), c=c, mom_in=self.state_ptr("mom_in"), mom_out=self.state_ptr("mom_out"),
                                   s_m=momentum[0], beta=momentum[1], nb=nb, chw=chw, hw=hw, thr=self.ptr("thr") if thr else 0)

    def read_state(self):
        torch.cuda.synchronize()
        return self.df.cpu()

    def check_state_fences(self, got):
        want = self.hf.clone()
        self.state(want, "mom_out")[:] = self.state(got, "mom_out")
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "mom_in or a fence of the state was written"


def _run(dev, nb, hw, K, off, n_keep, cls, nu_cls, alias, seed, c=COEF, momentum=MOMENTA[0], nan_in=None, swap=False):
    """one case, twice -> (out bf16 [n], nu' fp32 [n], t, pos, neg, nu); n_keep None: no thr; swap: the pairs the other way round"""
    chw, n = C * hw, nb * C * hw
    g = torch.Generator().manual_seed(seed)
    t, pos, neg = draw_rows(cls, n, K, g)
    nu = draw_nu(nu_cls, n, g)
    if nan_in is not None:
        pos[nan_in][::3] = float("nan")
        neg[nan_in][1::3] = float("nan")
    if swap:
        pos, neg = neg, pos
    b = MomentumBuffers(dev, n, nb * K * C, K, off, t, pos, neg, nu, alias)
    runs = []
    for _ in range(2):
        if n_keep is not None:
            b.threshold([n_keep] * K, nb, chw, hw)
        b.combine_momentum(c[:K], momentum, nb, chw, hw, thr=n_keep is not None)
        got, state = b.read(), b.read_state()
        b.check_fences(got, thr_written=n_keep is not None)
        b.check_state_fences(state)
        runs.append((b.window(got[0], "out").clone(), b.state(state, "mom_out").clone()))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)), \
        "a second run differs"
    return runs[0][0], runs[0][1], t, pos, neg, nu


def _check(tag, out, nu_new, t, pos, neg, nu, c, momentum, n_keep, nb, hw):
    chw, K = C * hw, len(pos)
    keep = None if n_keep is None else [n_keep] * K
    args = (t, pos, neg, c[:K], keep, nb, chw, hw, nu, momentum[0], momentum[1], omb_of(momentum[1]))
    ref, bnd, ref_nu, bnd_nu = oracle_and_bound(*args)
    want, want_nu = restate(*args)
    r = (worst_ratio(out.float(), ref, 1.01 * bnd), worst_ratio(nu_new, ref_nu, 1.01 * bnd_nu))
    same = torch.equal(_bits(out), _bits(want)) and torch.equal(nu_new.view(torch.int32), want_nu.contiguous().view(torch.int32))
    assert max(r) <= 1.0 and same, (tag, r, same)
    return r


def test_kernel_matrix(dev):
    """every (hw, n_keep or no thr, state class, alignment, aliasing) with nb, K, the input class and (s_m, beta) rotating"""
    worst, cases = [0.0, 0.0], 0
    for hw in (1, 35, 1000, 4096):
        keeps = sorted({1, max(1, hw // 20), hw}) + [None]
        for idx, (n_keep, nu_cls, off, alias) in enumerate(itertools.product(keeps, ("zero", "normal", "big"), (0, 1), (True, False))):
            nb, K = 1 + (idx // 4) % 2, 1 + (idx // 4 + idx // 24) % 3
            cls = ("normal", "ties", "low_byte", "below_key", "equal")[(idx // 4) % 5]
            momentum = MOMENTA[(idx // 2) % 3]
            tag = (nb, hw, K, off, alias, n_keep, cls, nu_cls, momentum)
            out, nu_new, t, pos, neg, nu = _run(dev, nb, hw, K, off, n_keep, cls, nu_cls, alias, seed=1000 * hw + idx, momentum=momentum)
            r = _check(tag, out, nu_new, t, pos, neg, nu, COEF, momentum, n_keep, nb, hw)
            worst = [max(a, b) for a, b in zip(worst, r)]
            cases += 1
    print(f"[eps_direction_momentum] {cases} cases, worst |got - float64| / (1.01 x bound): out {worst[0]:.3f}, nu' {worst[1]:.3f}")


@pytest.mark.parametrize("off", [0, 1])
def test_every_nb_and_K(dev, off):
    for nb, K, hw in itertools.product((1, 2), (1, 2, 3), (35, 1000)):
        n_keep = max(1, hw // 20)
        out, nu_new, t, pos, neg, nu = _run(dev, nb, hw, K, off, n_keep, "normal", "normal", True, seed=7 * hw + 10 * nb + K)
        _check((nb, hw, K, off), out, nu_new, t, pos, neg, nu, COEF, MOMENTA[0], n_keep, nb, hw)


@pytest.mark.parametrize("hw,off", [(1000, 0), (1000, 1), (35, 0)])
def test_identities(dev, hw, off):
    nb, K, chw = 2, 3, C * hw
    n_keep = max(1, hw // 20)
    s_m, beta = MOMENTA[0]
    # nu = 0: out is slh_eps_direction's (as values: s_m * 0 is a zero, and adding it turns an acc of -0 into +0, which is why
    # "momentum off" is the other kernel), and nu' = omb * g, g the kept products summed from +0
    out, nu_new, t, pos, neg, nu = _run(dev, nb, hw, K, off, n_keep, "normal", "zero", True, seed=31)
    plain = Buffers(dev, nb * chw, nb * K * C, K, off, t, pos, neg)
    plain.threshold([n_keep] * K, nb, chw, hw)
    plain.combine(COEF, nb, chw, hw)
    assert torch.equal(plain.window(plain.read()[0], "out").float(), out.float())
    g = torch.zeros(nb * chw)
    for k in range(K):
        keep, _ = kept(pos[k], neg[k], n_keep, nb, chw, hw)
        g = torch.where(keep, g + torch.tensor(COEF[k], dtype=torch.float32) * diff32(pos[k], neg[k]), g)
    assert torch.equal(nu_new, torch.tensor(omb_of(beta), dtype=torch.float32) * g)
    # the pairs the other way round under the opposite coefficients: the same out and the same nu'
    a = _run(dev, nb, hw, K, off, n_keep, "normal", "normal", False, seed=32)
    b = _run(dev, nb, hw, K, off, n_keep, "normal", "normal", False, seed=32, c=[-v for v in COEF], swap=True)
    assert torch.equal(a[0].float(), b[0].float()) and torch.equal(a[1], b[1])
    # a coefficient of 0 skips its term: NaN in its rows reaches neither output
    c = (0.75, 0.0, 0.5)
    out, nu_new, t, pos, neg, nu = _run(dev, nb, hw, K, off, n_keep, "normal", "normal", True, seed=33, c=c, nan_in=1)
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(nu_new).all())
    _check(("nan", hw, off), out, nu_new, t, pos, neg, nu, c, MOMENTA[0], n_keep, nb, hw)
