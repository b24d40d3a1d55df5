"""Every slh_gemm descriptor the capability rule accepts, element by element (tests/gemm_matrix.py has the matrix, the recipes, the
float64 references and the derivation of the bounds).

Per accepted case: the kernel's outputs meet  |got - ref| <= 2^-8 |ref| + n 2^-24 S + R  at EVERY element and the rounding statistic
|b| <= 0.05; nothing outside the outputs changed (4 KiB fences around every buffer, padding columns, inputs, split-K tickets zero,
the slab beyond splitk_slabs); every output element was written; a second run into freshly filled outputs gives the same bits; tile 0
names a kernel an explicit tile code also yields and agrees with it bit for bit; the weight-touch hint changes no bit.
Per refused case (one per tile x recipe that has any): slh_gemm raises, slh_last_error says why, nothing was written.
One test id per (tile family, recipe); the last test checks that the sweep ran as many cases as the recorded table holds.
"""
import json

import pytest
import torch

from sliders_amd import lib
from tests import gemm_matrix as gm
from tests.util import check_elementwise, stream

pytestmark = pytest.mark.gpu

_ACC, _REF = gm.enumerate_cases()
_BY = {}
for _c in _ACC:
    _BY.setdefault((gm.family(_c.tile), _c.recipe.name), ([], []))[0].append(_c)
for _c in _REF:
    _BY.setdefault((gm.family(_c.tile), _c.recipe.name), ([], []))[1].append(_c)
_IDS = sorted(_BY, key=lambda k: (gm.FAMILIES.index(k[0]), [r.name for r in gm.RECIPES].index(k[1])))
_RAN = {"accepted": 0, "refused": 0}
_REF_CACHE = {}


def _seed(case):
    d = case.dims
    return (d["M"] * 7919 + d["N"] * 104729 + d["K"] * 31 + sum(map(ord, case.recipe.name))) % (2 ** 31)


def _launch(ar, tile=None, **over):
    d = ar.desc(tile)
    for k, v in over.items():
        setattr(d, k, v)
    lib.call(lib.OP_GEMM, d, stream())
    torch.cuda.synchronize()
    return d


def _bits_equal(a, b):
    it = torch.int16 if a.dtype == gm.BF else torch.int32
    return torch.equal(a.view(it), b.view(it))


def _outputs(ar):
    return {b.name: ar.view(b.name).clone() for b in ar.case.bufs if b.role == "out"}


def _same_name_tile(case, ar):
    """an explicit tile code that yields, for the same descriptor, the kernel tile 0 picked"""
    S = (case.tile >> 16) & 15
    want = lib.gemm_kernel_name(ar.desc())
    for t in gm.TILES[1:]:
        d = ar.desc(t | (S << 16))
        if lib.gemm_tile_ok(d) and lib.gemm_kernel_name(d) == want:
            return t | (S << 16), want
    return None, want


def _run_accepted(case, dev):
    r = case.recipe
    ar = gm.Arena(case, dev)
    L = gm.fill_inputs(ar, _seed(case))
    ar.fill_outputs()
    ar.freeze()
    _launch(ar)
    assert ar.untouched_outside_outputs(), f"{case.id}: bytes outside the outputs changed (fence, padding column, input, ticket or spare slab)"
    got = _outputs(ar)
    # twice the same: nothing depends on arrival order
    ar.fill_outputs()
    _launch(ar)
    again = _outputs(ar)
    for nm in got:
        assert _bits_equal(got[nm], again[nm]), f"{case.id}: {nm} differs between two runs"
    assert ar.untouched_outside_outputs(), f"{case.id}: second run wrote outside the outputs"
    if r.pf:
        ar.fill_outputs()
        _launch(ar, pf_ptr=0, pf_bytes=0)
        bare = _outputs(ar)
        assert all(_bits_equal(got[nm], bare[nm]) for nm in got), f"{case.id}: the weight-touch hint changed the result"
    if gm.family(case.tile) == "auto":
        t, name = _same_name_tile(case, ar)
        assert t is not None, f"{case.id}: tile 0 launches {name}, which no explicit tile code yields for this descriptor"
        ar.fill_outputs()
        _launch(ar, tile=t)
        ex = _outputs(ar)
        assert all(_bits_equal(got[nm], ex[nm]) for nm in got), f"{case.id}: tile 0 ({name}) differs from explicit tile 0x{t:x}"
    # references
    key = (r.name, tuple(sorted((k, v) for k, v in case.dims.items() if k != "ln_cw")))
    if key not in _REF_CACHE:
        if len(_REF_CACHE) > 8:
            _REF_CACHE.clear()
        _REF_CACHE[key] = gm.reference(case, L)
    worst = (0.0, "", None)
    for nm, ref, bound, stat in _REF_CACHE[key]:
        g = got[nm]
        if nm == "c" and r.vt == 1:
            # the V columns go to vt_out only: c keeps its NaN fill there, bit for bit
            C = case.dims["vt_C"]
            assert bool((g[:, 2 * C:].view(torch.int16) == 0x7FC1).all()), f"{case.id}: the V columns of c were written without vt_also_c"
            g, ref, bound = g[:, :2 * C], ref[:, :2 * C], bound[:, :2 * C]
        w, at, b = check_elementwise(f"{case.id} [{nm}]", g, ref, bound, statistic=stat)
        if w >= worst[0]:
            worst = (w, nm, b if b is not None else worst[2])
        elif b is not None and (worst[2] is None or abs(b) > abs(worst[2])):
            worst = (worst[0], worst[1], b)
    if r.vt == 2:
        C, B, T = case.dims["vt_C"], case.dims["vt_B"], case.dims["vt_T"]
        assert torch.equal(got["c"][:, 2 * C:].reshape(B, T, C // 64, 64).permute(0, 2, 3, 1).reshape(-1, T), got["vt"]), \
            f"{case.id}: vt_out and the V columns of c hold different bits"
    if r.ln_out:
        ref, bound = gm.ln_out_reference(case, got["c"])
        w, at, _ = check_elementwise(f"{case.id} [ln_out]", got["ln_out"], ref, bound, statistic=False)
        if w > worst[0]:
            worst = (w, "ln_out", worst[2])
    _RAN["accepted"] += 1
    return worst


def _run_refused(case, dev):
    ar = gm.Arena(case, dev)
    ar.fill_outputs()
    ar.freeze()
    d = ar.desc()
    assert not lib.gemm_tile_ok(d), f"{case.id}: the rule answers differently for real addresses"
    with pytest.raises(lib.SlidersHipError):
        lib.call(lib.OP_GEMM, d, stream())
    assert lib.last_error(), f"{case.id}: refused without a message"
    torch.cuda.synchronize()
    assert torch.equal(ar.mem, ar.snap), f"{case.id}: a refused descriptor wrote memory"
    _RAN["refused"] += 1


@pytest.mark.parametrize("fam,recipe", _IDS, ids=[f"{f}-{r}" for f, r in _IDS])
def test_gemm_matrix(dev, fam, recipe):
    acc, ref = _BY[(fam, recipe)]
    worst, worst_b, wid = (0.0, "", None), None, ""
    for case in acc:
        w = _run_accepted(case, dev)
        if w[0] >= worst[0]:
            worst, wid = w, case.id
        if w[2] is not None and (worst_b is None or abs(w[2]) > abs(worst_b)):
            worst_b = w[2]
    seen = set()
    for case in ref:
        if case.tile & 0xFFFF in seen:
            continue
        seen.add(case.tile & 0xFFFF)
        _run_refused(case, dev)
    bs = "n/a" if worst_b is None else f"{worst_b:+.4f}"
    print(f"[parity] gemm matrix {fam} {recipe}: {len(acc)} accepted cases, {len(seen)} refused; worst |got - ref| / bound = {worst[0]:.3f} "
          f"({worst[1]}; {wid}); rounding statistic b = {bs}")


def test_gemm_matrix_ran_every_accepted_case():
    """no sampling: the sweep above ran exactly the cases the recorded table holds.  Counts in this process: it needs the whole
    module run in one process (no -k selection, no distribution over workers)."""
    table = json.load(open(gm.DATA))
    held = sum(len(v) for v in table["table"].values())
    assert held == table["accepted"] == len(_ACC)
    assert _RAN["accepted"] == held, (f"{_RAN['accepted']} cases ran in this process, the table holds {held} "
                                       "(run the whole module in one process)")
