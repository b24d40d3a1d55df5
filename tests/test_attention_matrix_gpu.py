"""Every form of the attention kernels, forward and backward, element by element (tests/attention_matrix.py has the cases, the input
classes, the float64 references and the derivation of the bounds).

Per case: all buffers live in one pattern-filled allocation with 4 KiB fences between them; outputs, workspaces and the transposed
copies are pre-filled with a NaN pattern, the 64-float padding behind lse and delta holds NaN.  vt / kt / qt / dot come from
slh_transpose_heads and their zero padding is checked exactly.  Then: every output meets its per-element bound against the float64
reference (check_elementwise: no non-finite value, the rounding statistic within STAT_LIMIT where it applies); every byte outside the
writable regions - fences, padding columns, the lse / delta padding, the inputs - is unchanged; a second run gives the same bits; the
weight-touch hint changes no bit and slh_attn_fwd_carries_touch agrees with the kernel the library names.  Tk = 1: o equals v exactly.
One chained forward -> backward case per DT keeps the former whole-tensor criterion (rel-L2 1.5e-2).
"""
import zlib

import pytest
import torch

from sliders_amd import lib
from tests import attention_matrix as am
from tests.util import check_elementwise, report, stream

pytestmark = pytest.mark.gpu

_WORST = {}        # kernel name -> (worst ratio, output, case id, b)


def _seed(c):
    return zlib.crc32(c.id.encode()) % (2 ** 31)


def _note(name, w, out, cid, b):
    cur = _WORST.get(name, (-1.0, "", "", None))
    big = b if b is not None and (cur[3] is None or abs(b) > abs(cur[3])) else cur[3]
    _WORST[name] = (w, out, cid, big) if w > cur[0] else (cur[0], cur[1], cur[2], big)


def _bits_equal(a, b):
    it = torch.int16 if a.dtype == am.BF else torch.int32
    return torch.equal(a.view(it), b.view(it))


def _transpose(ar, src_ptr, ld, dst, B, H, T, D, what, want):
    """slh_transpose_heads into the NaN-prefilled buffer dst; want: [B][H][T][D] - values exact, padding rows and columns exactly zero"""
    Dp, Tp = am.rup(D, 64), am.rup(T, 64)
    lib.call(lib.OP_TRANSPOSE_HEADS, lib.TransposeDesc(src=src_ptr, dst=ar.base + ar.off[dst], B=B, H=H, T=T, ld=ld, ldt=Tp, D=D), stream())
    torch.cuda.synchronize()
    t = ar.full(dst).view(B, H, Dp, Tp)
    assert torch.equal(t[:, :, :D, :T], want.permute(0, 1, 3, 2)), f"{what}: slh_transpose_heads values"
    bits = t.view(torch.int16)
    assert bool((bits[:, :, D:] == 0).all()) and bool((bits[..., T:] == 0).all()), f"{what}: slh_transpose_heads padding must be exactly zero"


def _put(ar, name, t, col0=0):
    """[B][T][H][D] -> columns [col0, col0 + H D) of the [B T][..] buffer"""
    B, T, H, D = t.shape
    ar.full(name)[:, col0:col0 + H * D] = t.reshape(B * T, H * D)


def _as_heads(t2d, B, T, H, D):
    """[B T][H D] -> [B][H][T][D]"""
    return t2d.reshape(B, T, H, D).permute(0, 2, 1, 3)


def _launch(op, d):
    lib.call(op, d, stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", am.FWD_CASES, ids=[c.id for c in am.FWD_CASES])
def test_attention_matrix_fwd(dev, case):
    c = case
    B, H, Tq, Tk, D, C = c.B, c.H, c.Tq, c.Tk, c.D, c.H * c.D
    ar = am.Arena(am.fwd_bufs(c), dev)
    L = am.make_inputs(c, dev, _seed(c))
    HV, first = H + c.vt_extra, (1 if c.vt_extra else 0)
    if c.pack == "qkv":
        _put(ar, "qkv", L["q"])
        _put(ar, "qkv", L["k"], C)
        _put(ar, "qkv", L["v"], 2 * C)
        v_ptr, ldv, v_wide = ar.base + ar.off["qkv"] + 2 * 2 * C, 3 * C, L["v"]
    else:
        _put(ar, "q", L["q"])
        _put(ar, "k", L["k"])
        g = torch.Generator(device=dev).manual_seed(5)
        v_wide = torch.randn(B, Tk, HV, D, generator=g, device=dev).to(am.BF)
        v_wide[:, :, first:first + H] = L["v"]
        _put(ar, "v", v_wide)
        v_ptr, ldv = ar.base + ar.off["v"], HV * D
    _transpose(ar, v_ptr, ldv, "vt", B, HV, Tk, D, c.id, am.heads(v_wide))
    ar.freeze()
    d = am.fwd_desc(c, ar.base, ar.off)
    name = lib.attn_fwd_kernel_name(d)
    assert name == am.fwd_name(c), f"{c.id}: the library names {name} for the real addresses, {am.fwd_name(c)} for made-up ones"
    _launch(lib.OP_ATTN_FWD, d)
    assert ar.untouched_outside_outputs(), f"{c.id}: bytes outside o and lse changed (fence, ldo padding, lse padding or an input)"
    got = {n: ar.view(n).clone() for n in ("o", "lse")}
    ar.refill_outputs()
    _launch(lib.OP_ATTN_FWD, d)
    for n in got:
        assert _bits_equal(got[n], ar.view(n)), f"{c.id}: {n} differs between two runs"
    assert lib.attn_carries_touch(d) == (name == "attn_fwd_ks_kernel"), f"{c.id}: slh_attn_fwd_carries_touch disagrees with {name}"
    if c.pf:
        ar.refill_outputs()
        _launch(lib.OP_ATTN_FWD, am.fwd_desc(c, ar.base, ar.off, pf=True))
        for n in got:
            assert _bits_equal(got[n], ar.view(n)), f"{c.id}: the weight-touch hint changed {n}"
    assert ar.untouched_outside_outputs(), f"{c.id}: a later run wrote outside o and lse"
    q, k, v = (am.heads(L[n]) for n in "qkv")
    o_ref, o_bound, l_ref, l_bound = am.forward_reference(q, k, v, D ** -0.5)
    go = _as_heads(got["o"], B, Tq, H, D)
    if Tk == 1:
        assert torch.equal(go, v.expand(B, H, Tq, D)), f"{c.id}: one key, softmax = 1: o must equal v exactly"
    w, _, b = check_elementwise(f"{c.id} [o]", go, o_ref, o_bound, statistic=True)
    wl, _, _ = check_elementwise(f"{c.id} [lse]", got["lse"].view(B, H, Tq), l_ref, l_bound, statistic=False)
    _note(name, w, "o", c.id, b)
    _note(name, wl, "lse", c.id, None)
    bs = "n/a" if b is None else f"{b:+.4f}"
    print(f"[parity] attn matrix {c.id}: {name}; worst |got - ref| / bound = {w:.3f} (o), {wl:.3f} (lse); rounding statistic b = {bs}")


def _forward_kernel(c, L, dev):
    """the forward kernel's own o [B T][C] and lse [B H Tq + 64] (plain tensors) for a chained case"""
    B, H, Tq, Tk, D, C = c.B, c.H, c.Tq, c.Tk, c.D, c.H * c.D
    Dp, Tkp = am.rup(D, 64), am.rup(Tk, 64)
    q, k, v = (L[n].reshape(-1, C).contiguous() for n in "qkv")
    vt = torch.full((B, H, Dp, Tkp), float("nan"), device=dev, dtype=am.BF)
    _launch(lib.OP_TRANSPOSE_HEADS, lib.TransposeDesc(src=v.data_ptr(), dst=vt.data_ptr(), B=B, H=H, T=Tk, ld=C, ldt=Tkp, D=D))
    o = torch.full((B * Tq, C), float("nan"), device=dev, dtype=am.BF)
    lse = torch.full((B * H * Tq + 64,), float("nan"), device=dev)
    _launch(lib.OP_ATTN_FWD, lib.AttnDesc(q=q.data_ptr(), k=k.data_ptr(), vt=vt.data_ptr(), o=o.data_ptr(), lse=lse.data_ptr(), B=B, H=H, Tq=Tq,
                                          Tk=Tk, ldq=C, ldk=C, ldvt=Tkp, ldo=C, scale=D ** -0.5, D=D))
    return o, lse


@pytest.mark.parametrize("case", am.BWD_CASES, ids=[c.id for c in am.BWD_CASES])
def test_attention_matrix_bwd(dev, case):
    c = case
    B, H, Tq, Tk, D, C = c.B, c.H, c.Tq, c.Tk, c.D, c.H * c.D
    n = B * H * Tq
    ar = am.Arena(am.bwd_bufs(c), dev)
    L = am.make_inputs(c, dev, _seed(c))
    q, k, v, do = (am.heads(L[x]) for x in ("q", "k", "v", "do"))
    if c.chained:
        o2d, lse_flat = _forward_kernel(c, L, dev)
        o, lse = _as_heads(o2d, B, Tq, H, D), lse_flat[:n].view(B, H, Tq)
    else:
        o, lse = am.forward_for_backward(q, k, v, D ** -0.5)
    if c.pack == "qkv":
        for i, x in enumerate("qkv"):
            _put(ar, "qkv", L[x], i * C)
        ptr = lambda i: ar.base + ar.off["qkv"] + 2 * i * C
        ld = 3 * C
    else:
        for x in "qkv":
            _put(ar, x, L[x])
        ptr = lambda i: ar.base + ar.off["qkv"[i]]
        ld = C
    ar.full("o")[:] = am.rows(o)
    _put(ar, "do", L["do"])
    ar.nan_fill("lse")                                  # the 64 floats of padding keep the NaN pattern
    ar.full("lse")[:n, 0] = lse.reshape(-1)
    _transpose(ar, ptr(1), ld, "kt", B, H, Tk, D, c.id + " kt", k)
    if c.need_dkv:
        _transpose(ar, ptr(0), ld, "qt", B, H, Tq, D, c.id + " qt", q)
        _transpose(ar, ar.base + ar.off["do"], C, "dot", B, H, Tq, D, c.id + " dot", do)
    ar.freeze()
    d = am.bwd_desc(c, ar.base, ar.off)
    names = lib.attn_bwd_kernel_names(d)
    assert names == am.bwd_names(c)
    outs = ["delta"] + (["dqkv"] if c.pack == "qkv" else ["dq"] + (["dk", "dv"] if c.need_dkv else []))
    _launch(lib.OP_ATTN_BWD, d)
    assert ar.untouched_outside_outputs(), f"{c.id}: bytes outside delta, dq, dk, dv changed (fence, the lse / delta padding or an input)"
    raw = {x: ar.view(x).clone() for x in outs}
    ar.refill_outputs()
    _launch(lib.OP_ATTN_BWD, d)
    for x in outs:
        assert _bits_equal(raw[x], ar.view(x)), f"{c.id}: {x} differs between two runs"
    assert ar.untouched_outside_outputs(), f"{c.id}: the second run wrote outside the outputs"
    got = {"delta": raw["delta"].view(B, H, Tq)}
    if c.pack == "qkv":
        got.update(dq=_as_heads(raw["dqkv"][:, :C], B, Tq, H, D), dk=_as_heads(raw["dqkv"][:, C:2 * C], B, Tk, H, D),
                   dv=_as_heads(raw["dqkv"][:, 2 * C:], B, Tk, H, D))
    else:
        got["dq"] = _as_heads(raw["dq"], B, Tq, H, D)
        if c.need_dkv:
            got.update(dk=_as_heads(raw["dk"], B, Tk, H, D), dv=_as_heads(raw["dv"], B, Tk, H, D))
    if c.chained:
        o64, _, l64, _ = am.forward_reference(q, k, v, D ** -0.5)
        ref = am.backward_reference(q, k, v, o64, do, l64, D ** -0.5, bool(c.need_dkv))
        for x in ("dq", "dk", "dv"):
            report(f"attn matrix {c.id} {x} ({names[0] if x == 'dq' else names[1]})", got[x], ref[x][0], 1.5e-2)
        return
    ref = am.backward_reference(q, k, v, o, do, lse, D ** -0.5, bool(c.need_dkv))
    stat = am.bwd_takes_statistic(c)
    line = []
    for x, (r, bound) in ref.items():
        w, _, b = check_elementwise(f"{c.id} [{x}]", got[x], r, bound, statistic=stat and x != "delta")
        _note(names[1] if x in ("dk", "dv") else (names[0] if x == "dq" else "attn_delta_kernel"), w, x, c.id, b)
        line.append(f"{x} {w:.3f}" + ("" if b is None else f" (b = {b:+.4f})"))
    print(f"[parity] attn matrix {c.id}: {names[0]}{', ' + names[1] if names[1] else ''}; worst |got - ref| / bound: " + ", ".join(line))


def test_attention_matrix_every_form_ran():
    """the sweep above reached every instantiation the library can name, each with a worst ratio <= 1 and - but for the delta kernel -
    an applied rounding statistic.  Counts in this process: it needs the whole module run in one process."""
    for name in am.FWD_NAMES + am.BWD_DQ_NAMES + am.BWD_DKV_NAMES + ["attn_delta_kernel"]:
        assert name in _WORST, f"{name} never ran (run the whole module in one process)"
        w, out, cid, b = _WORST[name]
        bs = "n/a" if b is None else f"{b:+.4f}"
        print(f"[parity] attn matrix form {name}: worst |got - ref| / bound = {w:.3f} ({out}; {cid}); largest |b| = {bs}")
        assert w <= 1.0
        assert b is not None or name == "attn_delta_kernel", f"{name}: no case applied the rounding statistic"
