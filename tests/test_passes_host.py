"""The driver of one UNet pass (sliders_amd/passes.py) and the slider session of the samplers (SliderSampler.slider_session) on the
host: stand-in plans whose io entries hold CPU tensors and whose two programs only record that they ran."""
import itertools
from types import SimpleNamespace

import pytest
import torch

from sliders_amd.edit import SliderEditor
from sliders_amd.passes import Pass, default_time_ids
from sliders_amd.sampler import SliderSampler

BF = torch.bfloat16
POOLED, ADD_IN = 5, 9


class _Prog:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def run(self, stream):
        self.log.append((self.name, stream))


def _plan(rows, h=8, w=12, cached=True, ctx_dim=6):
    log = []
    buf = lambda *shape, dtype=BF: SimpleNamespace(tensor=torch.full(shape, float("nan"), dtype=dtype))
    io = {"sample": buf(rows, 4, h, w), "ctx": buf(rows, 77, ctx_dim), "t": buf(rows, 1, dtype=torch.float32),
          "time_ids": buf(rows, 6, dtype=torch.float32), "add_in": buf(rows, ADD_IN)}
    return SimpleNamespace(B=rows, H=h, W=w, io=io, log=log, prog=_Prog("full", log), prog_text_cached=_Prog("cached", log) if cached else None)


def _engine(is_xl=True):
    return SimpleNamespace(cfg=SimpleNamespace(is_xl=is_xl, pooled_dim=POOLED), device=torch.device("cpu"))


@pytest.mark.parametrize("first,cached", itertools.product((True, False), (True, False)))
def test_program_rule(first, cached):
    p = _plan(2, cached=cached)
    drv = Pass(_engine(), p)
    want = "cached" if cached and not first else "full"
    assert drv.program(first).name == want
    drv.run(500, first, 17)
    assert p.log == [(want, 17)] and bool((p.io["t"].tensor == 500.0).all())


@pytest.mark.parametrize("rows", [2, 4, 6])
def test_load_latents_writes_every_block_and_nothing_else(rows):
    p = _plan(rows)
    x = torch.randn(2, 4, 8, 12, generator=torch.Generator().manual_seed(rows))
    Pass(_engine(), p).load_latents(x)
    smp = p.io["sample"].tensor
    assert smp.shape[0] == rows and not bool(torch.isnan(smp).any())
    for r in range(0, rows, 2):
        assert torch.equal(smp[r:r + 2], x.to(BF))
    assert all(bool(b.tensor.isnan().all()) for k, b in p.io.items() if k != "sample"), "no other input is written"
    assert p.log == []


def test_load_cond_defaults_and_reshapes_time_ids():
    h, w, rows = 8, 12, 2
    assert torch.equal(default_time_ids(h, w, rows), torch.tensor([[64.0, 96.0, 0.0, 0.0, 64.0, 96.0]] * 2))
    g = torch.Generator().manual_seed(0)
    ctx, pooled = torch.randn(rows, 77, 6, generator=g), torch.randn(rows, POOLED, generator=g)
    p = _plan(rows, h, w)
    Pass(_engine(), p).load_cond(ctx, pooled)
    assert torch.equal(p.io["ctx"].tensor, ctx.to(BF))
    assert torch.equal(p.io["time_ids"].tensor, torch.tensor([[64.0, 96.0, 0.0, 0.0, 64.0, 96.0]] * 2))
    add_in = p.io["add_in"].tensor
    assert torch.equal(add_in[:, :POOLED], pooled.to(BF)) and bool(add_in[:, POOLED:].isnan().all()), "columns past pooled_dim are untouched"
    given = torch.arange(12, dtype=torch.float64)            # any layout of rows * 6 numbers: reshaped, not replaced
    Pass(_engine(), p).load_cond(ctx, pooled, given)
    assert torch.equal(p.io["time_ids"].tensor, given.to(torch.float32).reshape(2, 6))
    assert bool(p.io["sample"].tensor.isnan().all()) and bool(p.io["t"].tensor.isnan().all()) and p.log == []


def test_load_cond_without_added_conditions_touches_neither_time_ids_nor_add_in():
    p = _plan(2)
    ctx = torch.randn(2, 77, 6, generator=torch.Generator().manual_seed(1))
    Pass(_engine(is_xl=False), p).load_cond(ctx)
    assert torch.equal(p.io["ctx"].tensor, ctx.to(BF))
    assert bool(p.io["time_ids"].tensor.isnan().all()) and bool(p.io["add_in"].tensor.isnan().all())


# ---- the slider session ----------------------------------------------------------------------------------------------------------
class _Merger:
    """WeightMerger's surface: one swept slider (scale None) and, with held=, one at a fixed scale"""

    def __init__(self, held=None):
        self.merged, self.events = False, []
        self.sliders = SimpleNamespace(scales=lambda swept=0.0: [float(swept)] + ([held] if held is not None else []))

    def merge(self, scales):
        self.merged = True
        self.events.append(("merge", list(scales)))

    def restore(self):
        self.merged = False
        self.events.append(("restore",))


def _sampler(cls=SliderSampler, store=None, merger=None):
    s = cls.__new__(cls)                 # the constructor builds a scheduler and a WeightMerger on a real engine
    lora = []
    s.eng = SimpleNamespace(set_lora=lambda active, multiplier=1.0: lora.append((active, multiplier)))
    s.store, s.merger, s.lora = store, merger, lora
    return s


def _walk(s, grid, drv, **kw):
    with s.slider_session(**kw) as gate:
        for i, t in enumerate(grid):
            drv.run(t, gate(t, i == 0), 0)


GRID = [750, 500, 250, 0]


def test_merge_on_crossing_start_noise_forces_the_full_program_on_that_step_only():
    m, p = _Merger(), _plan(2)
    s = _sampler(merger=m)
    _walk(s, GRID, Pass(_engine(), p), scale=1.5, start_noise=600)
    assert [n for n, _ in p.log] == ["full", "full", "cached", "cached"]
    assert m.events == [("merge", [1.5]), ("restore",)] and not m.merged and s.lora == [], "no store: the adapter is never touched"


def test_all_zero_scales_do_not_merge_and_a_held_slider_does():
    m, p = _Merger(), _plan(2)
    _walk(_sampler(merger=m), GRID, Pass(_engine(), p), scale=0.0, start_noise=600)
    assert [n for n, _ in p.log] == ["full", "cached", "cached", "cached"] and m.events == []
    m, p = _Merger(held=-1.0), _plan(2)
    _walk(_sampler(merger=m), GRID, Pass(_engine(), p), scale=0.0, start_noise=600)
    assert [n for n, _ in p.log] == ["full", "full", "cached", "cached"] and m.events == [("merge", [0.0, -1.0]), ("restore",)]


def test_the_editors_multiplier_zero_never_merges_even_with_a_held_slider():
    m, p = _Merger(held=-1.0), _plan(2)
    s = _sampler(SliderEditor, merger=m)
    _walk(s, GRID, Pass(_engine(), p), scale=0.0, start_noise=600, zero_merges=False)
    assert [n for n, _ in p.log] == ["full", "cached", "cached", "cached"] and m.events == []
    # per-pass multipliers (the footprint): 0 merges nothing, the first non-zero one merges and is a first pass again
    p = _plan(2)
    with s.slider_session(1.5, 600, zero_merges=False) as gate:
        for n, mult in enumerate((0.0, 0.0, 1.5, 1.5)):
            Pass(_engine(), p).run(500, gate(500, n == 0, mult), 0)
    assert [n for n, _ in p.log] == ["full", "cached", "full", "cached"] and m.events == [("merge", [1.5, -1.0]), ("restore",)]


def test_store_gate_sets_the_multiplier_per_step_and_switches_off_on_exit():
    s = _sampler(store=object())
    _walk(s, GRID, Pass(_engine(), _plan(2)), scale=2.0, start_noise=600)
    assert s.lora == [(True, 0.0), (True, 2.0), (True, 2.0), (True, 2.0), (False, 1.0)]


@pytest.mark.parametrize("cls", [SliderSampler, SliderEditor])
def test_session_exit_restores_and_switches_the_adapter_off_when_the_body_raises(cls):
    class Boom(RuntimeError):
        pass
    m = _Merger()
    s = _sampler(cls, store=object(), merger=m)
    with pytest.raises(Boom):
        with s.slider_session(1.5, 600) as gate:
            assert gate(500, True) is True and m.merged
            raise Boom()
    assert not m.merged and m.events == [("merge", [1.5]), ("restore",)]
    assert s.lora == [(True, 1.5), (False, 1.0)], "the adapter is off after an exception, for the sampler as for the editor"
