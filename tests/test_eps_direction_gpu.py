"""slh_direction_threshold and slh_eps_direction on the MI355X (docs/SAMPLING.md, "Prompt-direction sampling"), through the C ABI: the
thresholds are the reference's integers, every output is within the derived bound of float64 (tests/eps_direction_ref.py) and has the
fp32 restatement's bits, in fenced NaN-prefilled buffers; every case runs twice with a bit comparison."""
import itertools

import pytest
import torch

from sliders_amd import lib
from tests.eps_direction_ref import diff32, kept, key_of, oracle_and_bound, restate, worst_ratio
from tests.test_eps_direction_host import COEF, draw_rows

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements of fence in front of and behind every buffer
BF = torch.bfloat16
C = 4                            # latent channels
FENCE32 = -0x5A5A5A5B            # the int32 fence (thr is an integer buffer)


class Buffers:
    """Every buffer of one call inside one NaN-prefilled bf16 device tensor (one row per buffer: t, out, pos[K], neg[K]) and one
    fence-prefilled int32 tensor (thr), GUARD elements in front and behind; the rows are 16-byte aligned and a buffer begins `off`
    elements behind its guard, so off = 1 takes the 16-byte accesses away."""

    def __init__(self, dev, n, n_thr, K, off, t, pos, neg):
        self.n, self.n_thr, self.K, self.off = n, n_thr, K, off
        self.names = ["t", "out"] + [f"pos{k}" for k in range(K)] + [f"neg{k}" for k in range(K)]
        L = 2 * GUARD + (n + 1 + 7) // 8 * 8
        self.h16 = torch.full((len(self.names), L), float("nan"), dtype=BF)
        for name, v in [("t", t)] + [(f"pos{k}", pos[k]) for k in range(K)] + [(f"neg{k}", neg[k]) for k in range(K)]:
            self.window(self.h16, name)[:] = v
        self.h32 = torch.full((2 * GUARD + n_thr,), FENCE32, dtype=torch.int32)
        self.d16, self.d32 = self.h16.to(dev), self.h32.to(dev)

    def window(self, t16, name):
        return t16[self.names.index(name), GUARD + self.off:GUARD + self.off + self.n]

    def ptr(self, name):
        if name == "thr":
            return self.d32.data_ptr() + GUARD * 4
        return self.d16[self.names.index(name)].data_ptr() + (GUARD + self.off) * 2

    def rows(self, side):
        return [self.ptr(f"{side}{k}") for k in range(self.K)]

    def threshold(self, n_keep, nb, chw, hw):
        lib.direction_threshold(torch.cuda.current_stream().cuda_stream, pos=self.rows("pos"), neg=self.rows("neg"), thr=self.ptr("thr"),
                                n_keep=n_keep, nb=nb, chw=chw, hw=hw)

    def combine(self, c, nb, chw, hw, thr=True):
        lib.eps_direction(torch.cuda.current_stream().cuda_stream, t=self.ptr("t"), out=self.ptr("out"), pos=self.rows("pos"), neg=self.rows("neg"),
                          c=c, nb=nb, chw=chw, hw=hw, thr=self.ptr("thr") if thr else 0)

    def read(self):
        torch.cuda.synchronize()
        return self.d16.cpu(), self.d32.cpu()

    def check_fences(self, got, thr_written=True):
        """everything but out's window and thr has the bits it had: the inputs and every guard"""
        want16 = self.h16.clone()
        self.window(want16, "out")[:] = self.window(got[0], "out")
        assert torch.equal(got[0].view(torch.int16), want16.view(torch.int16)), "an input or a fence was written"
        want32 = self.h32.clone()
        if thr_written:
            want32[GUARD:GUARD + self.n_thr] = got[1][GUARD:GUARD + self.n_thr]
        assert torch.equal(got[1], want32), "a fence of thr was written"


def _bits(t):
    return t.contiguous().view(torch.int16)


def _n_keeps(hw):
    return sorted({1, min(2, hw), max(1, hw // 20), max(1, hw - 1), hw})


def _run(dev, nb, hw, K, off, n_keep, cls, seed, c=COEF, nan_in=None):
    """one case through both kernels, twice -> (out bf16 [n], thr int32 [nb][K][C], t, pos, neg)"""
    chw, n = C * hw, nb * C * hw
    g = torch.Generator().manual_seed(seed)
    t, pos, neg = draw_rows(cls, n, K, g)
    if nan_in is not None:
        pos[nan_in][::3] = float("nan")
        neg[nan_in][1::3] = float("nan")
    b = Buffers(dev, n, nb * K * C, K, off, t, pos, neg)
    runs = []
    for _ in range(2):
        b.threshold([n_keep] * K, nb, chw, hw)
        b.combine(c[:K], nb, chw, hw)
        got = b.read()
        b.check_fences(got)
        runs.append(got)
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1]), "a second run differs"
    return b, b.window(runs[0][0], "out").clone(), runs[0][1][GUARD:GUARD + nb * K * C].reshape(nb, K, C), t, pos, neg


def _check(tag, out, thr, t, pos, neg, c, n_keep, nb, hw, skip_thr=()):
    chw, K = C * hw, len(pos)
    for k in range(K):
        if k in skip_thr:
            continue
        keep, tau = kept(pos[k], neg[k], n_keep, nb, chw, hw)
        assert torch.equal(thr[:, k], tau), ("tau", k, tag, thr[:, k].tolist(), tau.tolist())
        mine = key_of(diff32(pos[k], neg[k])).reshape(nb, C, hw) >= thr[:, k].reshape(nb, C, 1)
        assert torch.equal(mine.sum(2), keep.reshape(nb, C, hw).sum(2)) and bool((mine.sum(2) >= n_keep).all()), ("kept count", k, tag)
    ref, bnd = oracle_and_bound(t, pos, neg, c[:K], [n_keep] * K, nb, chw, hw)
    r = worst_ratio(out.float(), ref, 1.01 * bnd)
    same = torch.equal(_bits(out), _bits(restate(t, pos, neg, c[:K], [n_keep] * K, nb, chw, hw)))
    assert r <= 1.0 and same, ("out", r, same, tag)
    return r


def test_kernel_matrix(dev):
    """every (hw, n_keep, input class, alignment) with nb and K rotating through their values"""
    worst, cases = 0.0, 0
    for hw in (1, 35, 1000, 4096):
        for idx, (n_keep, cls, off) in enumerate(itertools.product(_n_keeps(hw), ("normal", "ties", "low_byte", "below_key", "equal"), (0, 1))):
            nb, K = 1 + (idx // 2) % 2, 1 + (idx // 2 + idx // 10) % 3
            tag = (nb, hw, K, off, n_keep, cls)
            _, out, thr, t, pos, neg = _run(dev, nb, hw, K, off, n_keep, cls, seed=1000 * hw + idx)
            worst = max(worst, _check(tag, out, thr, t, pos, neg, COEF, n_keep, nb, hw))
            cases += 1
            if cls == "equal":
                assert bool((thr == 0).all()) and torch.equal(_bits(out), _bits(t)), ("e+ == e-: tau = 0 and out has t's bits", tag)
            if cls == "below_key":
                assert bool((thr == 0x437F).all()), ("one key: all tie", tag)
    print(f"[eps_direction] {cases} cases, worst |got - float64| / (1.01 x bound) {worst:.3f}")


@pytest.mark.parametrize("off", [0, 1])
def test_every_nb_and_K(dev, off):
    for nb, K, hw in itertools.product((1, 2), (1, 2, 3), (35, 1000)):
        n_keep = max(1, hw // 20)
        _, out, thr, t, pos, neg = _run(dev, nb, hw, K, off, n_keep, "normal", seed=7 * hw + 10 * nb + K)
        _check((nb, hw, K, off), out, thr, t, pos, neg, COEF, n_keep, nb, hw)


def test_the_largest_latent(dev):
    nb, K, hw = 2, 3, 16384
    _, out, thr, t, pos, neg = _run(dev, nb, hw, K, 0, hw // 20, "normal", seed=5)
    _check((nb, hw, K), out, thr, t, pos, neg, COEF, hw // 20, nb, hw)


@pytest.mark.parametrize("hw,off", [(1000, 0), (1000, 1), (35, 0)])
def test_identities(dev, hw, off):
    nb, K, chw = 2, 3, C * hw
    n_keep = max(1, hw // 20)
    # a coefficient of 0 skips its term: NaN in its rows does not reach out
    c = (0.75, 0.0, 0.5)
    _, out, thr, t, pos, neg = _run(dev, nb, hw, K, off, n_keep, "normal", seed=21, c=c, nan_in=1)
    assert bool(torch.isfinite(out.float()).all())
    _check(("nan", hw, off), out, thr, t, pos, neg, c, n_keep, nb, hw, skip_thr=(1,))
    # every coefficient 0: t's bits
    b, out, *_ = _run(dev, nb, hw, K, off, n_keep, "normal", seed=22, c=(0.0, 0.0, 0.0), nan_in=0)
    assert torch.equal(_bits(out), _bits(b.window(b.h16, "t")))
    # n_keep = hw against no thr at all: the same bits, and thr is not touched without the threshold launch
    b, out, thr, t, pos, neg = _run(dev, nb, hw, K, off, hw, "normal", seed=23)
    a = Buffers(dev, nb * chw, nb * K * C, K, off, t, pos, neg)
    a.combine(COEF, nb, chw, hw, thr=False)
    got = a.read()
    a.check_fences(got, thr_written=False)
    assert torch.equal(_bits(a.window(got[0], "out")), _bits(out))
    ref, bnd = oracle_and_bound(t, pos, neg, COEF, None, nb, chw, hw)
    assert worst_ratio(out.float(), ref, 1.01 * bnd) <= 1.0
    # the pair the other way round under the opposite coefficients: the same bits (d and c change sign, the keys read |d|)
    s, out_s, thr_s, *_ = _run(dev, nb, hw, K, off, n_keep, "normal", seed=24)
    w = Buffers(dev, nb * chw, nb * K * C, K, off, s.window(s.h16, "t"), [s.window(s.h16, f"neg{k}") for k in range(K)],
                [s.window(s.h16, f"pos{k}") for k in range(K)])
    w.threshold([n_keep] * K, nb, chw, hw)
    w.combine([-v for v in COEF], nb, chw, hw)
    got = w.read()
    assert torch.equal(got[1][GUARD:GUARD + nb * K * C].reshape(nb, K, C), thr_s) and torch.equal(_bits(w.window(got[0], "out")), _bits(out_s))
