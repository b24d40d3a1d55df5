"""slh_latent_blend on the MI355X (docs/SAMPLING.md, "Localised sampling"): the case matrix, every output within the derived bound of
float64 (tests/latent_blend_ref.py) in fenced NaN-prefilled buffers, and the exact identities with torch.equal."""
import itertools

import pytest
import torch

from sliders_amd import lib
from sliders_amd.ddim import DDIMSchedule
from sliders_amd.edit import ddpm_step_coefficients, fp32_coefficients
from tests.latent_blend_ref import bound, expand_mask, oracle, worst_ratio
from tests.test_latent_blend_host import S_NEXT, draw_inputs, draw_mask

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements of NaN in front of and behind every buffer
BF, F32 = torch.bfloat16, torch.float32


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


class Buffers:
    """Every buffer of one call inside two NaN-prefilled device tensors (one row per buffer, GUARD elements in front and behind; the rows
    are 16-byte aligned and a buffer begins `off` elements behind its guard, so off = 1 takes the 16-byte accesses away), and their
    host images."""

    def __init__(self, dev, n, n_mask, fp32, off, e, keep, mask):
        self.n, self.n_mask, self.fp32, self.off = n, n_mask, fp32, off
        self.names32 = ("e", "keep", "out", "mask") if fp32 else ("mask",)
        self.names16 = ("in1", "in2") if fp32 else ("e", "keep", "out", "in1", "in2")
        L = 2 * GUARD + (max(n, n_mask) + 1 + 7) // 8 * 8
        self.h32 = torch.full((len(self.names32), L), float("nan"))
        self.h16 = torch.full((len(self.names16), L), float("nan"), dtype=BF)
        for name, v in (("e", e), ("keep", keep), ("mask", mask)):
            self.window(self.h32 if name in self.names32 else self.h16, name)[:] = v
        self.d32, self.d16 = self.h32.to(dev), self.h16.to(dev)

    def _where(self, name):
        return (self.names32, name) if name in self.names32 else (self.names16, name)

    def window(self, t, name):
        """the buffer's elements inside t, a tensor shaped like h32 / h16"""
        names, _ = self._where(name)
        return t[names.index(name), GUARD + self.off:GUARD + self.off + (self.n_mask if name == "mask" else self.n)]

    def ptr(self, name):
        names, _ = self._where(name)
        d = self.d32 if names is self.names32 else self.d16
        return d[names.index(name)].data_ptr() + (GUARD + self.off) * d.element_size()

    def launch(self, nb, chw, hw, s_next, out="out", in2=True):
        lib.latent_blend(torch.cuda.current_stream().cuda_stream, e=self.ptr("e"), keep=self.ptr("keep"), mask=self.ptr("mask"), out=self.ptr(out),
                         nb=nb, chw=chw, hw=hw, fp32=self.fp32, s_next=s_next, in_bf16=self.ptr("in1"), in2_bf16=self.ptr("in2") if in2 else 0)
        torch.cuda.synchronize()
        return self.d32.cpu(), self.d16.cpu()

    def get(self, got, name):
        return self.window(got[0] if name in self.names32 else got[1], name)

    def check_fences(self, got, written):
        """everything but the written windows has the bits it had: the inputs, the unused buffers, every guard"""
        want = (self.h32.clone(), self.h16.clone())
        for name in written:
            self.window(want[0] if name in self.names32 else want[1], name)[:] = self.get(got, name)
        assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1])), "an input or a fence was written"


def _case(dev, nb, chw, hw, fp32, off, mcls, icls, seed):
    g = torch.Generator().manual_seed(seed)
    n = nb * chw
    mask = draw_mask(mcls, nb * hw, g)
    e, keep = draw_inputs(icls, n, expand_mask(mask, nb, chw, hw), g, not fp32)
    return Buffers(dev, n, nb * hw, fp32, off, e, keep, mask), e, keep, mask


# (chw, hw): one pixel per channel; an odd size over several blocks; whole vectors; the 33^2 tail; one channel; an odd tail; and (48, 12):
# hw a multiple of 4 but not of 8 - the fp32 form takes its 16-byte accesses, the bf16 form cannot
SHAPES = [(4, 1), (900, 225), (1024, 256), (4356, 1089), (5, 5), (1023, 341), (48, 12)]
MATRIX = list(itertools.product((1, 2), SHAPES, (True, False), (0, 1), ("zeros", "ones", "binary", "fractional", "mixed"),
                                ("unit", "large", "nan_e", "nan_keep")))


def test_kernel_matrix(dev):
    worst = {"out fp32": 0.0, "out bf16": 0.0, "in": 0.0}
    for idx, (nb, (chw, hw), fp32, off, mcls, icls) in enumerate(MATRIX):
        tag = (nb, chw, hw, fp32, off, mcls, icls)
        b, e, keep, mask = _case(dev, nb, chw, hw, fp32, off, mcls, icls, seed=idx)
        s_next = S_NEXT if fp32 else 1.0
        got = b.launch(nb, chw, hw, s_next)
        b.check_fences(got, ("out", "in1", "in2"))
        out, in1, in2 = (b.get(got, k) for k in ("out", "in1", "in2"))
        ref = oracle(e, keep, mask, nb, chw, hw, s_next)
        bnd = bound(e, keep, mask, nb, chw, hw, s_next, bf16_out=not fp32)
        r = worst_ratio(out, ref[0], 1.01 * bnd[0])
        assert r <= 1.0, ("out", r, tag)
        worst["out fp32" if fp32 else "out bf16"] = max(worst["out fp32" if fp32 else "out bf16"], r)
        m = expand_mask(mask, nb, chw, hw)
        assert torch.equal(_bits(out[m == 0]), _bits(keep[m == 0])) and torch.equal(_bits(out[m == 1]), _bits(e[m == 1])), ("select", tag)
        if fp32:          # the copies are the rounding of the kernel's own fp32 out, scaled: exact
            want_in = (out * s_next).to(BF)
            r = worst_ratio(out * s_next, ref[1], 1.01 * bnd[1])
            assert r <= 1.0, ("in", r, tag)
            worst["in"] = max(worst["in"], r)
        else:
            want_in = out
        assert torch.equal(_bits(in1), _bits(want_in)) and torch.equal(_bits(in2), _bits(want_in)), ("copies", tag)
    print(f"[latent_blend] {len(MATRIX)} cases, worst |got - float64| / (1.01 x bound): out fp32 {worst['out fp32']:.3f}, out bf16 "
          f"{worst['out bf16']:.3f}, scaled input before its bf16 rounding {worst['in']:.3f}")


@pytest.mark.parametrize("fp32", [True, False])
@pytest.mark.parametrize("chw,hw,off", [(1024, 256, 0), (1024, 256, 1), (900, 225, 0), (48, 12, 0)])
def test_kernel_identities(dev, fp32, chw, hw, off):
    nb, n = 2, 2 * chw
    s_next = S_NEXT if fp32 else 1.0
    run = lambda b, **kw: b.launch(nb, chw, hw, s_next, **kw)
    # a second run is bit-equal; inputs and fences untouched
    b, e, keep, mask = _case(dev, nb, chw, hw, fp32, off, "mixed", "unit", seed=3)
    first = run(b)
    again = run(b)
    b.check_fences(first, ("out", "in1", "in2"))
    assert torch.equal(_bits(first[0]), _bits(again[0])) and torch.equal(_bits(first[1]), _bits(again[1]))
    # out aliasing e: the bits of the call that aliases nothing
    a, _, _, _ = _case(dev, nb, chw, hw, fp32, off, "mixed", "unit", seed=3)
    got = run(a, out="e")
    a.check_fences(got, ("e", "in1", "in2"))
    assert torch.equal(_bits(a.get(got, "e")), _bits(b.get(first, "out")))
    assert torch.equal(_bits(a.get(got, "in1")), _bits(b.get(first, "in1"))) and torch.equal(_bits(a.get(got, "in2")), _bits(b.get(first, "in2")))
    # without in2 nothing is written there
    c, _, _, _ = _case(dev, nb, chw, hw, fp32, off, "mixed", "unit", seed=3)
    got = run(c, in2=False)
    c.check_fences(got, ("out", "in1"))
    assert torch.equal(_bits(c.get(got, "out")), _bits(b.get(first, "out")))
    # m = 0 gives keep, m = 1 gives e - with NaN everywhere on the other side
    for mcls, icls, src in (("zeros", "nan_e", "keep"), ("ones", "nan_keep", "e")):
        d, e, keep, _ = _case(dev, nb, chw, hw, fp32, off, mcls, icls, seed=4)
        want = keep if src == "keep" else e
        got = run(d)
        assert torch.equal(_bits(d.get(got, "out")), _bits(want)), (mcls, "out")
        assert torch.equal(_bits(d.get(got, "in1")), _bits((want * s_next).to(BF) if fp32 else want)), (mcls, "copies")
    # e == keep gives keep under any mask
    g = torch.Generator().manual_seed(5)
    keep = torch.randn(n, generator=g) * 30.0
    keep = keep if fp32 else keep.to(BF)
    f = Buffers(dev, n, nb * hw, fp32, off, keep, keep, draw_mask("fractional", nb * hw, g))
    assert torch.equal(_bits(f.get(run(f), "out")), _bits(keep))


@pytest.mark.parametrize("hw", [35, 64])          # chw = 140: the scalar form of slh_latent_blend; chw = 256: its 16-byte form
def test_agrees_with_ddpm_edit_blend(dev, hw):
    """The blend is one piece of code (csrc/step_common.h): slh_ddpm_edit_step (mode 1) followed by slh_latent_blend writes the bits
    slh_ddpm_edit_blend writes in one launch - out and both bf16 copies.  s_next = 1: the copy rne(out * 1) is rne(out)."""
    nb, chw = 2, 4 * hw
    n, s = nb * chw, torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(11)
    eps = torch.randn(2 * n, generator=g).to(BF)
    x, resid, keep = (torch.randn(n, generator=g) for _ in range(3))
    mask = torch.rand(nb * hw, generator=g)
    mask[0::3], mask[1::3] = 0.0, 1.0             # exact 0, exact 1 and fractions
    p1 = (1 - hw) % 3                             # mask[hw + p1] == 1: a pixel of sample 1
    assert mask[0] == 0 and mask[hw + p1] == 1 and 0 < mask[2] < 1
    resid[hw] = float("nan")                      # e = mu + resid is NaN at (sample 0, channel 1, pixel 0), where m == 0
    keep[chw + 2 * hw + p1] = float("nan")        # keep is NaN at (sample 1, channel 2, pixel p1), where m == 1
    f = fp32_coefficients(ddpm_step_coefficients(DDIMSchedule(), 500, 50, 1.0))
    eps_d, x_d, resid_d, keep_d, mask_d = (t.to(dev) for t in (eps, x, resid, keep, mask))
    new32 = lambda: torch.full((n,), float("nan"), device=dev)
    new16 = lambda: torch.full((n,), float("nan"), device=dev, dtype=BF)
    common = dict(eps=eps_d.data_ptr(), x=x_d.data_ptr(), resid=resid_d.data_ptr(), nb=nb, chw=chw, guidance=7.5, v_prediction=0, **f)
    e, two, one = new32(), (new32(), new16(), new16()), (new32(), new16(), new16())
    lib.call(lib.OP_DDPM_EDIT, lib.DdpmEditDesc(out=e.data_ptr(), mode=1, **common), s)
    lib.latent_blend(s, e=e.data_ptr(), keep=keep_d.data_ptr(), mask=mask_d.data_ptr(), out=two[0].data_ptr(), nb=nb, chw=chw, hw=hw, fp32=True,
                     s_next=1.0, in_bf16=two[1].data_ptr(), in2_bf16=two[2].data_ptr())
    lib.call(lib.OP_DDPM_EDIT_BLEND, lib.DdpmEditBlendDesc(keep=keep_d.data_ptr(), mask=mask_d.data_ptr(), hw=hw, out=one[0].data_ptr(),
                                                           out_bf16=one[1].data_ptr(), out2_bf16=one[2].data_ptr(), **common), s)
    torch.cuda.synchronize()
    assert torch.isnan(e[hw]), "the NaN in e is where it was put"
    for name, a, b in zip(("out", "first bf16 copy", "second bf16 copy"), two, one):
        assert not torch.isnan(a).any() and not torch.isnan(b).any(), f"{name}: a NaN from the unselected side reached it"
        assert torch.equal(_bits(a), _bits(b)), f"{name}: slh_latent_blend and slh_ddpm_edit_blend differ"
