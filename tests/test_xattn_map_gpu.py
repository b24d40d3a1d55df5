"""slh_xattn_map on the device, through every layer that uses it (tests/xattn_map_matrix.py has the cases, the float64 reference and
the derivation of the bound; docs/EDIT.md "A mask from a word" the results).

Kernel matrix: per case all buffers live in one pattern-filled allocation with 4 KiB fences; the columns of q and k the kernel has no
business reading hold NaN, `out` starts as NaN (or as a random prior with accumulate).  Every element meets its bound against the
float64 reference, the closed forms (all-ones weights, all-zero q) are met to the same bound, every byte outside `out` is unchanged,
and a second run from the same starting state gives the same bits.
Engine: a maps plan computes the ordinary plan's epsilon bit for bit where nothing fuses, and its maps agree with the fp32 oracle's
as well as a torch-bf16 run of the same oracle does (the project's 1.25x rule).  Editor and CLI: word_map / word_mask / --mask_tokens.
"""
import os
import zlib

import pytest
import torch

from sliders_amd import lib
from tests import xattn_map_matrix as xm
from tests.util import check_elementwise, stream

pytestmark = pytest.mark.gpu

_WORST = {"ratio": -1.0, "id": ""}


@pytest.mark.parametrize("case", xm.CASES, ids=[c.id for c in xm.CASES])
def test_xattn_map_matrix(dev, case):
    c = case
    L = xm.inputs(c, zlib.crc32(c.id.encode()) % (2 ** 31))
    ar = xm.Arena(c, L, dev)
    d = ar.desc(lib)
    lib.call(lib.OP_XATTN_MAP, d, stream())
    torch.cuda.synchronize()
    got = ar.out()
    assert ar.untouched_outside_out(), f"{c.id}: bytes outside out changed (a fence or an input)"
    ref, bound = xm.reference(c, L)
    w, _, _ = check_elementwise(c.id, got, ref, bound, statistic=False)
    print(f"[parity] xattn_map {c.id}: worst |got - ref| / bound = {w:.3f}")
    if w > _WORST["ratio"]:
        _WORST.update(ratio=w, id=c.id)
    cf = xm.closed_form(c, L)
    if cf is not None:
        check_elementwise(c.id + " [closed form]", got, cf, bound + 4 * 2.0 ** -53 * cf.abs(), statistic=False)
    ar.reset()
    lib.call(lib.OP_XATTN_MAP, d, stream())
    torch.cuda.synchronize()
    assert torch.equal(ar.out().view(torch.int32), got.view(torch.int32)), f"{c.id}: two runs differ"
    assert ar.untouched_outside_out(), f"{c.id}: the second run wrote outside out"


def test_xattn_map_matrix_worst(dev):
    """the figure docs/EDIT.md records (counts in this process: run the whole module)"""
    assert _WORST["ratio"] >= 0, "the matrix did not run in this process"
    print(f"[parity] xattn_map matrix: worst |got - ref| / bound over {len(xm.CASES)} cases = {_WORST['ratio']:.3f} ({_WORST['id']})")
    assert _WORST["ratio"] <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------------------
def _engine_inputs(cfg, hw, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 4, hw, hw, generator=g)
    ctx = torch.randn(2, 77, cfg.cross_attention_dim, generator=g)
    kw = None
    if cfg.is_xl:
        kw = {"text_embeds": torch.randn(2, cfg.pooled_dim, generator=g), "time_ids": torch.tensor([[hw * 8.0, hw * 8.0, 0, 0, hw * 8.0, hw * 8.0]] * 2)}
    wt = torch.zeros(1, 77)
    wt[0, 2], wt[0, 3] = 1.0, 0.5
    return x, ctx, kw, wt


def _run_maps(eng, x, ctx, kw, wt, t=500.0):
    """one pass of the maps plan -> (eps, {factor: map [1][T]}) as CPU tensors"""
    p = eng.plan(2, x.shape[2], x.shape[3], "off", attn_maps={"max_factor": 4})
    eng.load_inputs(p, x.to(eng.device), t, ctx.to(eng.device), None if kw is None else {k: v.to(eng.device) for k, v in kw.items()})
    p.io["xattn_wt"].tensor.copy_(wt)
    for k, b in p.io.items():
        if k.startswith("xattn_map."):
            b.tensor.fill_(float("nan"))
    p.prog.run(stream(), graph=False)
    torch.cuda.synchronize()
    return p.io["eps"].tensor.clone().cpu(), {int(k.split(".")[1]): b.tensor.clone().cpu() for k, b in p.io.items() if k.startswith("xattn_map.")}


def _oracle_net(name, dtype=torch.float32):
    from oracle.unet_oracle import build_unet
    net = build_unet(name, seed=0)
    for prm in net.parameters():             # bf16-valued weights: the engine, the fp32 oracle and its bf16 arm hold the same numbers
        prm.data = prm.data.to(torch.bfloat16).to(dtype)
    return net


def _engine(name, dev):
    from sliders_amd.config import CONFIGS
    from sliders_amd.unet import UNetEngine
    cfg = CONFIGS[name]()
    net = _oracle_net(name)
    return cfg, net, UNetEngine(cfg, net.state_dict(), dev)


def test_maps_plan_keeps_eps_where_nothing_fuses(dev):
    """tiny SDXL at 16 x 16 latents: HW % 128 != 0 at every level, the ordinary plan runs every cross-attention as its own launch, so
    the maps plan is the ordinary plan plus read-only map ops"""
    cfg, _, eng = _engine("tiny_sdxl", dev)
    x, ctx, kw, wt = _engine_inputs(cfg, 16)
    out = eng(x.to(dev), 500.0, ctx.to(dev), {k: v.to(dev) for k, v in kw.items()}, mode="off").sample
    ref_eps = eng.plan(2, 16, 16, "off").io["eps"].tensor.clone().cpu()
    eps, maps = _run_maps(eng, x, ctx, kw, wt)
    assert torch.equal(eps.view(torch.int16), ref_eps.view(torch.int16))
    assert sorted(maps) == [2, 4] and all(bool(torch.isfinite(m).all()) for m in maps.values())
    eps2, maps2 = _run_maps(eng, x, ctx, kw, wt)
    assert torch.equal(eps2.view(torch.int16), eps.view(torch.int16))
    assert all(torch.equal(maps[f].view(torch.int32), maps2[f].view(torch.int32)) for f in maps)
    assert out.shape == x.shape


def _oracle_maps(name, x, ctx, kw, wt, hw, factors, dtype):
    """The per-level maps from the oracle's own q and k (forward hooks on attn2.to_q / to_k), formed in float64: the mean over the
    level's layers and heads of softmax(q k^T / sqrt(D)) . wt, for the text half"""
    net = _oracle_net(name, dtype)
    cap = {}
    hooks = []
    for name, mod in net.named_modules():
        if name.endswith("attn2.to_q") or name.endswith("attn2.to_k"):
            hooks.append(mod.register_forward_hook(lambda m, i, o, name=name: cap.__setitem__(name, o.detach().to(torch.float64))))
    r = lambda a: a.to(torch.bfloat16).to(dtype)
    with torch.no_grad():
        net(r(x), torch.tensor(500.0), r(ctx), None if kw is None else {k: r(v) for k, v in kw.items()})
    for h in hooks:
        h.remove()
    sums, counts = {}, {}
    for name in sorted(n for n in cap if n.endswith("to_q")):
        q, k = cap[name][1:], cap[name[:-1] + "k"][1:]           # the text half
        T, C = q.shape[1], q.shape[2]
        f = int(round((hw * hw / T) ** 0.5))
        if f not in factors:
            continue
        heads = _heads_of(net, name)
        D = C // heads
        qh, kh = q.reshape(1, T, heads, D).transpose(1, 2), k.reshape(1, 77, heads, D).transpose(1, 2)
        P = torch.softmax(qh @ kh.transpose(-1, -2) * D ** -0.5, dim=-1)           # [1][heads][T][77]
        m = (P * wt.to(torch.float64)[:, None, None, :]).sum(-1).mean(1)             # [1][T]
        sums[f] = sums.get(f, 0) + m
        counts[f] = counts.get(f, 0) + 1
    return {f: sums[f] / counts[f] for f in sums}


def _heads_of(net, q_name):
    mod = net
    for part in q_name.split(".")[:-1]:
        mod = getattr(mod, part) if not part.isdigit() else mod[int(part)]
    return mod.heads


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("name,hw", [("tiny_sdxl", 32), ("tiny_sd1", 16)])
def test_maps_against_the_oracle(dev, name, hw):
    """The maps of the engine against the fp32 oracle's, by relative L2 per level; the tolerance is what a torch-bf16 run of the same
    oracle misses by, times 1.25 (parity).  At 32 x 32 the ordinary tiny-SDXL plan fuses the factor-2 cross-attention,
    so there the maps plan is a different program and only its maps are judged."""
    cfg, net, eng = _engine(name, dev)
    x, ctx, kw, wt = _engine_inputs(cfg, hw)
    _, maps = _run_maps(eng, x, ctx, kw, wt)
    _, again = _run_maps(eng, x, ctx, kw, wt)
    want = [1, 2, 4] if name == "tiny_sd1" else [2, 4]
    assert sorted(maps) == want
    ref = _oracle_maps(name, x, ctx, kw, wt, hw, want, torch.float32)
    arm = _oracle_maps(name, x, ctx, kw, wt, hw, want, torch.bfloat16)
    assert sorted(ref) == want
    for f in want:
        assert torch.equal(maps[f].view(torch.int32), again[f].view(torch.int32)), f"level {f}: two runs differ"
        e, b = _rel_l2(maps[f], ref[f]), _rel_l2(arm[f], ref[f])
        print(f"[parity] xattn maps {name} {hw}x{hw} level {f}: engine rel-L2 {e:.3e}, torch-bf16 arm {b:.3e}, ratio {e / b:.2f}")
        assert e <= 1.25 * b, f"{name} level {f}: engine {e:.3e} > 1.25 x bf16 arm {b:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
# editor
# ---------------------------------------------------------------------------------------------------------------------------
def _editor(dev, form):
    from sliders_amd.edit import SliderEditor
    from sliders_amd.lora_store import LoraStore
    cfg, net, eng = _engine("tiny_sdxl", dev)
    store = sliders = None
    if form != "none":
        store = LoraStore(cfg, rank=4, alpha=1.0, train_method="noxattn", device=dev)
        g = torch.Generator().manual_seed(3)
        for e in store.entries:
            store.params[e.up_off:e.up_off + e.up_numel] = (torch.randn(e.up_numel, generator=g) * 0.05).to(dev, torch.bfloat16)
        if form == "sliders":
            from sliders_amd.merge import SliderSet
            sliders = SliderSet(cfg, [({k: v.cpu() for k, v in store.state_dict().items()}, None)])
            store = None
    return cfg, eng, SliderEditor(eng, store, None, sliders=sliders)


def _invert(cfg, ed, dev, hw=16):
    g = torch.Generator().manual_seed(11)
    ctx = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).to(dev)
    pooled = torch.randn(2, cfg.pooled_dim, generator=g).to(dev)
    x0 = torch.randn(1, 4, hw, hw, generator=g).to(dev)
    return ed.invert(ctx, x0, steps=10, skip=3, guidance_scale=3.0, seed=2, pooled=pooled)


@pytest.fixture(scope="module")
def plain_map(dev):
    """word_map of the editor without a slider: what the store= and sliders= forms are compared with"""
    cfg, eng, ed = _editor(dev, "none")
    sp = _invert(cfg, ed, dev)
    return ed.word_map(sp, tokens=[2, 3], draws=3).cpu()


@pytest.mark.parametrize("form", ["store", "sliders"])
def test_word_map_on_the_editor(dev, tmp_path, form, plain_map):
    from sliders_amd.edit import NoiseSpace, footprint_draws, word_mask
    cfg, eng, ed = _editor(dev, form)
    sp = _invert(cfg, ed, dev)
    passes = []
    mode = "on" if form == "store" else "off"
    p = eng.plan(2, 16, 16, mode, attn_maps={"max_factor": 4})
    real = p.prog.run
    p.prog.run = lambda *a, **k: (passes.append(1), real(*a, **k))[1]
    if p.prog_text_cached is not None:
        real_c = p.prog_text_cached.run
        p.prog_text_cached.run = lambda *a, **k: (passes.append(1), real_c(*a, **k))[1]
    F = ed.word_map(sp, tokens=[2, 3], draws=3)
    idx = footprint_draws(sp.timesteps, sp.timesteps[0], 3, 0)
    assert len(passes) == len(idx) == 3
    assert F.shape == (1, 16, 16) and F.dtype == torch.float32 and bool(torch.isfinite(F).all()) and float(F.min()) >= 0.0
    # the engine is as it was: the scale-0 edit is still the reconstruction
    assert torch.equal(ed.edit_latents(sp, scale=0.0), sp.recon)
    F2 = ed.word_map(sp, tokens=[2, 3], draws=3)
    assert torch.equal(F, F2)
    path = os.path.join(tmp_path, "space.pt")
    sp.save(path)
    F3 = ed.word_map(NoiseSpace.load(path, dev), tokens=[2, 3], draws=3)
    assert torch.equal(F, F3)
    # the slider is off: the same program on the same inputs as the editor without a slider (store=: the adapter program at
    # multiplier 0, whose adapter terms are exact zeros added in fp32 ahead of the one bf16 rounding)
    assert torch.equal(F.cpu(), plain_map), f"{form}: word_map differs from the slider-free editor's (max {float((F.cpu() - plain_map).abs().max()):.3e})"
    # on random weights the map is nearly flat: binarise half way between its smallest and largest pixel so that both sides exist
    rel = F.cpu() / F.cpu().max()
    m = word_mask(F.cpu(), threshold=float((rel.min() + 1.0) / 2.0), dilate=0, feather=0.0)
    out = ed.edit_latents(sp, scale=2.0, mask=m)
    keep = (m == 0).reshape(1, 1, 16, 16).expand_as(out).to(dev)
    assert bool(keep.any()) and bool((m > 0).any())
    assert torch.equal(out[keep], sp.recon[keep])


def test_cli_mask_tokens(dev, tmp_path, monkeypatch):
    from PIL import Image
    import numpy as np
    import sliders_amd.model_util as mu
    from sliders_amd import edit
    from sliders_amd.config import CONFIGS
    from sliders_amd.unet import UNetEngine

    def tiny(model, device, seed):           # --synthetic on the tiny SDXL topology: the full-size random UNet is not what this is about
        cfg = CONFIGS["tiny_sdxl"]()
        return UNetEngine(cfg, mu.random_state_dict(cfg, device, seed), device)
    monkeypatch.setattr(mu, "synthetic_engine", tiny)
    img = os.path.join(tmp_path, "in.png")
    Image.fromarray((np.random.RandomState(0).rand(64, 64, 3) * 255).astype("uint8")).save(img)
    out, att, msk = os.path.join(tmp_path, "out"), os.path.join(tmp_path, "att.png"), os.path.join(tmp_path, "mask.png")
    edit.main(["--synthetic", "--model", "sdxl", "--image", img, "--res", "128", "--steps", "6", "--skip", "2", "--scales", "0,1",
               "--mask_tokens", "2,3", "--mask_word_draws", "2", "--save_attention", att, "--save_mask", msk, "--out", out])
    for f in (att, msk):
        im = Image.open(f)
        assert im.size == (16, 16) and im.mode == "L"
    assert np.asarray(Image.open(att)).max() == 255
    assert sorted(os.listdir(out)) == ["recon.png", "scale_0.png", "scale_1.png"]
