"""The tape of a training forward plan: typed records, complete when they are appended, one backward handler per type.
CPU only: the dry-run plans of tests/plan_digest.py (virtual arenas, no device)."""
import functools
from dataclasses import dataclass

import pytest
import torch

from sliders_amd import lib
from sliders_amd.arena import Arena
from sliders_amd.backward import BackwardPlan
from sliders_amd.config import CONFIGS
from sliders_amd.lora_store import LoraStore
from sliders_amd.planner import AttnRec, Conv3, ConvOutRec, GegluRec, GemmRec, GnRec, LnRec, UNetPlan
from tests import plan_digest as pd

RECORDS = (GemmRec, GnRec, LnRec, AttnRec, GegluRec, ConvOutRec)
CASES = [("tiny_sdxl", 16, "noxattn"), ("tiny_sd1", 16, "full"), ("tiny_sdxl", 16, "full")]


@functools.lru_cache(maxsize=None)
def _train(name, hw, method):
    """(forward plan, backward plan) of one training dry run; shared, read only"""
    p, bw, _, _ = pd.plan(name, hw, method, "train")
    return p, bw


@pytest.mark.parametrize("name,hw,method", CASES)
def test_every_record_is_typed_and_has_a_backward_handler(name, hw, method):
    p, bw = _train(name, hw, method)
    assert p.tape and all(type(r) in RECORDS for r in p.tape)
    assert {type(r) for r in p.tape} == set(RECORDS), "a tiny training plan reaches every record kind"
    assert set(BackwardPlan.HANDLERS) == set(RECORDS)
    assert isinstance(p.tape[-1], ConvOutRec) and bw.prog.n_ops > p.prog.n_ops
    # complete when appended: every product's record names its output (and T wherever it carries an adapter)
    gemms = [r for r in p.tape if isinstance(r, GemmRec)]
    assert all(r.out is not None and (r.T is not None) == (r.grp is not None) for r in gemms)
    assert all(r.N > 0 and r.K > 0 and r.K % 64 == 0 for r in gemms)
    # no-grad plans record nothing
    assert pd.plan(name, hw, method, "on")[0].tape == []


def test_a_record_kind_without_a_handler_is_an_error_that_names_it():
    @dataclass
    class MadeUpRec:
        name: str

    p, _, _, _ = pd.plan("tiny_sdxl", 16, "noxattn", "train")
    n = len(p.tape)
    p.tape.append(MadeUpRec("made_up"))
    with pytest.raises(TypeError, match="MadeUpRec"):
        BackwardPlan(p, *pd.GRAD_SAMPLE, pd.ONE_PTR)
    del p.tape[n:]
    assert BackwardPlan(p, *pd.GRAD_SAMPLE, pd.ONE_PTR).prog.n_ops > 0


@pytest.mark.parametrize("name,hw,method", [c for c in CASES if c[2] == "full"])
def test_conv1_of_every_resnet_carries_its_temb_path_and_nothing_else_does(name, hw, method):
    p, bw = _train(name, hw, method)
    assert p.lora.temb_entries, "train method full adapts time_emb_proj"
    gemms = [r for r in p.tape if isinstance(r, GemmRec)]
    conv1 = [r for r in gemms if r.name.endswith(".conv1")]
    assert [r.temb_path for r in conv1] == [r.name[:-len(".conv1")] for r in conv1]
    assert sorted(r.temb_path for r in conv1) == sorted(p.w.resnet_paths)
    assert all(r.temb_path is None for r in gemms if not r.name.endswith(".conv1"))
    assert not any(hasattr(r, "temb_path") for r in p.tape if not isinstance(r, GemmRec))
    # the backward reads it: one time_emb_proj adapter gradient per resnet and sample that carries a gradient
    n = sum(1 for nm in bw.prog.op_names if nm.endswith(".conv1.temb_lora"))
    assert n == len(p.w.resnet_paths) * bw.nb


def test_training_fold_keeps_the_layernorm_record_around_a_stand_in():
    """On SD-1.x at a 32 x 32 latent, the smallest dry run whose training plan accepts a fold (10 of its 48 LayerNorms; the tiny
    configurations' plans accept none: no tile that takes a fold runs their products)."""
    p, _ = _train("sd1", 32, "noxattn")
    by_name = {nm: d for o, d, nm in p.ops if o == lib.OP_GEMM}
    folds = [(r, p.tape[i + 1]) for i, r in enumerate(p.tape) if isinstance(r, LnRec) and r.out.name.endswith(".unwritten")]
    assert len(folds) >= 4, "this training plan accepts LayerNorm folds"
    for ln, prod in folds:
        assert isinstance(prod, GemmRec) and prod.x is ln.out and prod.x is not ln.x
        d = by_name[prod.name]
        assert d.ln_in and d.ln_mr_out == ln.mr.ptr and d.a0 == ln.x.ptr, "the launch reads the un-normalised tensor"
        assert not any(nm == ln.name for _, _, nm in p.ops), "no LayerNorm launch"
    # a LayerNorm that was launched wrote its output: the product behind it reads that buffer
    for i, r in enumerate(p.tape):
        if isinstance(r, LnRec) and not r.out.name.endswith(".unwritten"):
            assert by_name[p.tape[i + 1].name].a0 == r.out.ptr and not by_name[p.tape[i + 1].name].ln_in


@pytest.mark.parametrize("mode", ["off", "train"])
def test_a_plain_3x3_product_plans_as_a_convolution(mode):
    """stride 1, no source transform: the value every field of which is its default is still a convolution"""
    assert Conv3() == Conv3(stride=1, xform=0) and Conv3() is not None
    p = pd.plan("tiny_sdxl", 16, "noxattn", mode)[0]
    plain = [(d, nm) for o, d, nm in p.ops if o == lib.OP_GEMM and nm.endswith((".conv1", ".conv2"))]
    assert len(plain) == 2 * len(p.w.resnet_paths)
    for d, nm in plain:
        assert d.mode == 1 and d.stride == 1 and d.src_xform == 0, nm
        assert d.K == 9 * (d.ca0 + d.ca1) and (d.ho, d.wo) == (d.hs, d.ws) and d.M == d.batch * d.ho * d.wo, nm
    down = [d for o, d, nm in p.ops if o == lib.OP_GEMM and nm.endswith(".downsamplers.0.conv")]
    up = [d for o, d, nm in p.ops if o == lib.OP_GEMM and nm.endswith(".upsamplers.0.conv")]
    assert down and all(d.mode == 1 and d.stride == 2 and d.src_xform == 0 and 2 * d.ho == d.hs for d in down)
    assert up and all(d.mode == 1 and d.stride == 1 and d.src_xform == 1 and d.ho == 2 * d.hs for d in up)
    assert all(d.mode == 0 for o, d, nm in p.ops if o == lib.OP_GEMM and nm.endswith((".proj_in", ".ff2", ".conv_shortcut")))
    if mode == "train":
        recs = {r.name: r for r in p.tape if isinstance(r, GemmRec)}
        assert all(recs[nm].conv == Conv3() for _, nm in plain)
        assert all(r.conv is None for r in recs.values() if r.name.endswith((".proj_in", ".ff2", ".conv_shortcut")))
    # the final convolution (slh_skinny) too
    last = [d for o, d, nm in p.ops if nm == "conv_out"]
    assert len(last) == 1 and last[0].mode == 1 and last[0].stride == 1 and last[0].src_xform == 0


def test_planning_leaves_the_lora_store_as_it_was():
    cfg = CONFIGS["tiny_sd1"]()
    store = LoraStore(cfg, train_method="full", init="none")
    before = set(vars(store))
    w = pd.Weights(cfg)
    for mode in ("on", "train"):
        va, vz = Arena(1 << 50, None), Arena(1 << 40, None)
        p = UNetPlan(cfg, w, va, vz, pd.B, 16, 16, pd.CTX, store, mode, pd.SCALE_PTR)
        if mode == "train":
            BackwardPlan(p, *pd.GRAD_SAMPLE, pd.ONE_PTR)
    assert set(vars(store)) == before and "temb_tcol" not in vars(store)
    # the store's own table, built on the first request: column -> the first T column of its resnet's adapter
    tcol = store.temb_tcol_table(w)
    assert tcol is store.temb_tcol_table(w) and tcol.dtype == torch.int32 and tcol.numel() == w.temb_total
    for i, path in enumerate(w.resnet_paths):
        o, n = w.temb_offsets[path], store.temb_entries[i].target.out_dim
        assert bool((tcol[o:o + n] == 4 * i).all())
    gemv = [d for o, d, nm in p.ops if nm == "time_emb_proj_all"]
    assert len(gemv) == 1 and gemv[0].lora_tcol == tcol.data_ptr()
