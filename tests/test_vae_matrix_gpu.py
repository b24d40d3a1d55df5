"""Every form of the fp32 image-path kernels element by element (tests/vae_matrix.py has the cases, the float64 references and the
derivation of the bounds; docs/VAE_MATRIX.md the results).

Per case: all buffers live in one pattern-filled allocation with 4 KiB fences between them; outputs, the GroupNorm scratch (`partial`)
and padding columns are pre-filled with a NaN pattern, the tickets start from zero.  Then: every output meets its per-element bound
against the float64 reference (check_elementwise: no non-finite value, the rounding statistic within STAT_LIMIT where it applies;
noisy_bf16 equals the bf16 rounding of noisy_f32 bit for bit); every byte outside the writable regions - fences, padding columns, the
inputs - is unchanged; the tickets are left zero; a second run from the same starting state gives the same bits (no kernel of
csrc/vae.hip uses fp32 atomics).  Which sgemm kernel runs is what the library answers (lib.sgemm_form).
"""
import zlib

import pytest
import torch

from sliders_amd import lib
from tests import vae_matrix as vm
from tests.util import check_elementwise, stream

pytestmark = pytest.mark.gpu

_WORST = {}        # form -> (worst ratio, output, case id, largest |b| seen)


def _note(name, w, out, cid, b):
    cur = _WORST.get(name, (-1.0, "", "", None))
    big = b if b is not None and (cur[3] is None or abs(b) > abs(cur[3])) else cur[3]
    _WORST[name] = (w, out, cid, big) if w > cur[0] else (cur[0], cur[1], cur[2], big)


def _bits_equal(a, b):
    it = torch.int16 if a.dtype == vm.BF else torch.int32
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


@pytest.mark.parametrize("case", vm.CASES, ids=[c.id for c in vm.CASES])
def test_vae_matrix(dev, case):
    c = case
    K = vm.KINDS[c.kind]
    bufs = K["bufs"](c)
    ar = vm.Arena(bufs, dev)
    L = K["inputs"](c, dev, zlib.crc32(c.id.encode()) % (2 ** 31))
    for name, t in L.items():
        ar.full(name)[:t.shape[0], :t.shape[1]] = t
    ar.freeze()
    ops = K["descs"](c, ar.base, ar.off)
    if c.kind == "sgemm":
        real = lib.sgemm_form(ops[0][1])
        assert "sgemm " + real == vm.form_of(c), f"{c.id}: the library names {real} for the real addresses, {vm.form_of(c)} for made-up ones"
    st = stream()

    def run():
        for op, d in ops:
            lib.call(op, d, st)
        torch.cuda.synchronize()

    run()
    assert ar.untouched_outside_outputs(), f"{c.id}: bytes outside the outputs changed (a fence, padding columns or an input)"
    outs = [b.name for b in bufs if b.role == "out" or (c.kind == "softmax" and b.name == "x")]
    got = {n: ar.view(n).clone() for n in outs}
    if c.kind == "gn32":
        assert int(ar.view("ticket").view(torch.int32).abs().sum()) == 0, f"{c.id}: tickets must be left zero"
    line = []
    for label, (buf, r, bound) in K["reference"](c, L, got).items():
        if bound is None:
            assert _bits_equal(got[buf], r), f"{c.id} [{label}]: must be bit-exact"
            w, b = 0.0, None
        else:
            w, _, b = check_elementwise(f"{c.id} [{label}]", got[buf], r, bound, statistic=True)
        _note(vm.form_of(c, label), w, label, c.id, b)
        line.append(f"{label} {w:.3f}" + ("" if b is None else f" (b = {b:+.4f})"))
    # a second run from the same starting state (NaN prefill, the in-place operand, zero tickets)
    ar.restore()
    run()
    for n in outs:
        assert _bits_equal(got[n], ar.view(n)), f"{c.id}: {n} differs between two runs"
    if c.kind == "gn32":
        assert int(ar.view("ticket").view(torch.int32).abs().sum()) == 0, f"{c.id}: tickets must be left zero (second run)"
    assert ar.untouched_outside_outputs(), f"{c.id}: the second run wrote outside the outputs"
    print(f"[parity] vae matrix {c.id}: {vm.form_of(c)}; worst |got - ref| / bound: " + ", ".join(line))


def test_vae_matrix_every_form_ran(dev):
    """the sweep above reached every form vae_matrix.FORMS names (the sgemm ones as the library names them), each with a worst ratio
    <= 1.  Counts in this process: it needs the whole module run in one process."""
    big = None
    for name in vm.FORMS:
        assert name in _WORST, f"{name} never ran (run the whole module in one process)"
        w, out, cid, b = _WORST[name]
        bs = "n/a" if b is None else f"{b:+.4f}"
        print(f"[parity] vae matrix form {name}: worst |got - ref| / bound = {w:.3f} ({out}; {cid}); largest |b| = {bs}")
        assert w <= 1.0
        if b is not None and (big is None or abs(b) > abs(big)):
            big = b
    print(f"[parity] vae matrix: largest |b| over all forms = {'n/a' if big is None else f'{big:+.4f}'}")
