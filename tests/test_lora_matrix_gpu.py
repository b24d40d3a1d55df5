"""Every form of the LoRA helper kernels, forward and backward, element by element (tests/lora_matrix.py has the cases, the input
classes, the float64 references and the derivation of the bounds; docs/LORA_MATRIX.md the results).

Per case: all buffers live in one pattern-filled allocation with 4 KiB fences between them; outputs, slabs and padding columns are
pre-filled with a NaN pattern, the += targets start from random values, the tickets from zero.  Then: every output meets its
per-element bound against the float64 reference (check_elementwise: no non-finite value, the rounding statistic within STAT_LIMIT
where it applies; a_out of ln_fold and EW_COPY bit for bit); every byte outside the writable regions - fences, padding columns, the
inputs - is unchanged; the tickets of the slab forms are left zero; a second run from the same starting state gives the same bits for
every form without fp32 atomics and stays within the bound for the atomic ones.  Which skinny instantiation runs and how a weight
gradient is split is what the library answers (lib.skinny_kernel_name, lib.wgrad_geometry).
"""
import zlib

import pytest
import torch

from sliders_amd import lib
from tests import lora_matrix as lm
from tests.util import check_elementwise, stream

pytestmark = pytest.mark.gpu

_WORST = {}        # form -> (worst ratio, output, case id, largest |b| seen)


def _note(name, w, out, cid, b):
    cur = _WORST.get(name, (-1.0, "", "", None))
    big = b if b is not None and (cur[3] is None or abs(b) > abs(cur[3])) else cur[3]
    _WORST[name] = (w, out, cid, big) if w > cur[0] else (cur[0], cur[1], cur[2], big)


def _bits_equal(a, b):
    it = torch.int16 if a.dtype == lm.BF else torch.int32
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _launcher(c, ar, dev):
    """-> (a function that launches the case once, objects to keep alive)"""
    st = stream()
    if c.kind == "lnfold":
        table = torch.tensor(lm.lnfold_items(c, ar.base, ar.off), dtype=torch.int64, device=dev)
        d = lib.LoraLnFoldDesc(items=table.data_ptr(), n=len(c.rows))
        return (lambda: lib.call(lib.OP_LORA_LN_FOLD, d, st)), table
    if c.kind == "wgrad":
        descs = lm.wgrad_descs(c, ar.base, ar.off)
        if not c.form.startswith("batch"):
            return (lambda: lib.call(lib.OP_WGRAD, descs[0], st)), descs
        bd, keep = lib.batch_table(lib.OP_WGRAD_BATCH, descs, dev, arg=c.R)
        assert bd.total == sum(lm.wgrad_blocks(c)), f"{c.id}: slh_lora_wgrad_blocks and slh_lora_wgrad_geometry disagree"
        if c.form == "batch_slab":
            bd.slabs, bd.tickets = ar.base + ar.off["slabs"], ar.base + ar.off["tickets"]
        return (lambda: lib.call(lib.OP_WGRAD_BATCH, bd, st)), (bd, keep, descs)
    fn = {"skinny": lm.skinny_descs, "gemv": lm.gemv_descs, "cdgrad": lm.cdgrad_descs, "temb": lm.temb_descs, "ew": lm.ew_descs}[c.kind]
    ops = fn(c, ar.base, ar.off)
    if c.kind == "skinny":
        real = lib.skinny_kernel_name(ops[0][1])
        assert real == lm.form_of(c), f"{c.id}: the library names {real} for the real addresses, {lm.form_of(c)} for made-up ones"

    def run():
        for op, d in ops:
            lib.call(op, d, st)
    return run, ops


@pytest.mark.parametrize("case", lm.CASES, ids=[c.id for c in lm.CASES])
def test_lora_matrix(dev, case):
    c = case
    K = lm.KINDS[c.kind]
    form = lm.form_of(c)
    ar = lm.Arena(K["bufs"](c), dev)
    L = K["inputs"](c, dev, zlib.crc32(c.id.encode()) % (2 ** 31))
    for name, t in L.items():
        ar.full(name)[:t.shape[0], :t.shape[1]] = t
    ar.freeze()
    run, keep = _launcher(c, ar, dev)
    run()
    torch.cuda.synchronize()
    assert ar.untouched_outside_outputs(), f"{c.id}: bytes outside the outputs changed (a fence, padding columns or an input)"
    ref = K["reference"](c, L)
    got = {n: ar.view(n).clone() for n in ref}
    slab = c.kind == "wgrad" and c.form in ("slab", "batch_slab")
    if slab:
        assert int(ar.view("tickets").view(torch.int32).abs().sum()) == 0, f"{c.id}: tickets must be left zero"
    line = []
    for n, (r, bound) in ref.items():
        if bound is None:
            assert _bits_equal(got[n], r), f"{c.id} [{n}]: must be bit-exact"
            w, b = 0.0, None
        else:
            w, _, b = check_elementwise(f"{c.id} [{n}]", got[n], r, bound, statistic=True)
        _note(form, w, n, c.id, b)
        line.append(f"{n} {w:.3f}" + ("" if b is None else f" (b = {b:+.4f})"))
    # a second run from the same starting state (NaN prefill, starting values of the += targets, zero tickets)
    ar.restore()
    run()
    torch.cuda.synchronize()
    atomics = lm.has_atomics(c)
    for n, (r, bound) in ref.items():
        again = ar.view(n)
        if atomics:
            check_elementwise(f"{c.id} [{n}] second run", again, r, bound, statistic=False)
        else:
            assert _bits_equal(got[n], again), f"{c.id}: {n} differs between two runs"
    if slab:
        assert int(ar.view("tickets").view(torch.int32).abs().sum()) == 0, f"{c.id}: tickets must be left zero (second run)"
    assert ar.untouched_outside_outputs(), f"{c.id}: the second run wrote outside the outputs"
    print(f"[parity] lora matrix {c.id}: {form}{' (atomics)' if atomics else ''}; worst |got - ref| / bound: " + ", ".join(line))


def test_lora_matrix_every_form_ran(dev):
    """the sweep above reached every form lora_matrix.FORMS names (the skinny ones as the library names them), each with a worst ratio
    <= 1.  Counts in this process: it needs the whole module run in one process."""
    big = None
    for name in lm.FORMS:
        assert name in _WORST, f"{name} never ran (run the whole module in one process)"
        w, out, cid, b = _WORST[name]
        bs = "n/a" if b is None else f"{b:+.4f}"
        print(f"[parity] lora matrix form {name}: worst |got - ref| / bound = {w:.3f} ({out}; {cid}); largest |b| = {bs}")
        assert w <= 1.0
        if b is not None and (big is None or abs(b) > abs(big)):
            big = b
    print(f"[parity] lora matrix: largest |b| over all forms = {'n/a' if big is None else f'{big:+.4f}'}")
