"""Sliders merged into the frozen weights (sliders_amd/merge.py), host side: the item table that maps every adapted module to each
stored copy of its weight, checked by applying a numpy restatement of slh_lora_merge to the stored tensors and comparing with a
WeightStore built from the plainly merged state dict; parsing of ranks / alphas / targets; the CLI option."""
import json
import os

import numpy as np
import pytest
import torch

from oracle.unet_oracle import build_unet
from sliders_amd import lib
from sliders_amd.config import CONFIGS
from sliders_amd.merge import SliderSet, WeightMerger, module_names
from sliders_amd.modules import lora_targets
from sliders_amd.weights import WeightStore

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CENSUS = sorted(json.load(open(os.path.join(G, "lora_census.json"))))          # "<model>/<train_method>"


def random_slider(cfg, method, rank, alpha, seed, std=0.05, dtype=torch.bfloat16):
    """A slider checkpoint in the reference's layout (lora.py:231-248) with random factors: lora_down as the reference initialises it
    in scale (~ 1 / sqrt(fan_in) is not needed here: both factors ~ std N(0, 1), rounded to `dtype` like a saved checkpoint)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for t in lora_targets(cfg, method, rank):
        k = 3 if t.kind == "conv3" else 1
        down = (t.rank, t.in_dim) if t.kind == "linear" else (t.rank, t.in_dim, k, k)
        up = (t.out_dim, t.rank) if t.kind == "linear" else (t.out_dim, t.rank, 1, 1)
        sd[f"{t.lora_name}.alpha"] = torch.tensor(float(alpha))
        sd[f"{t.lora_name}.lora_down.weight"] = (torch.randn(down, generator=g) * std).to(dtype)
        sd[f"{t.lora_name}.lora_up.weight"] = (torch.randn(up, generator=g) * std).to(dtype)
    return sd


def merged_state_dict(cfg, sd, sliders, scales, dtype=torch.float64):
    """The plain statement: weight + sum_i s_i (alpha_i / r_i) B_i A_i per adapted module, in `dtype`, on the bf16 weights the engine
    stores.  sliders: checkpoints in the reference's layout."""
    names = module_names(cfg)
    out = {k: v.to(torch.bfloat16).to(dtype) if v.is_floating_point() else v for k, v in sd.items()}
    for lsd, s in zip(sliders, scales):
        for key in lsd:
            if not key.endswith(".lora_down.weight"):
                continue
            name = key[:-len(".lora_down.weight")]
            path, _ = names[name]
            down, up = lsd[key].to(dtype), lsd[f"{name}.lora_up.weight"].to(dtype)
            r = down.shape[0]
            alpha = float(lsd[f"{name}.alpha"]) if f"{name}.alpha" in lsd else float(r)
            delta = torch.einsum("or,r...->o...", up.reshape(up.shape[0], r), down)
            w = out[path + ".weight"]
            out[path + ".weight"] = w + (s * alpha / r) * delta.reshape(w.shape)
    return out


def _bits(t):       # bf16 tensor -> its uint16 bits as a flat numpy array (a view: writes land in the tensor)
    return t.view(torch.int16).reshape(-1).numpy().view(np.uint16)


def _bf16_to_f64(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _round_bf16(x64):
    return _bits(torch.from_numpy(np.ascontiguousarray(x64)).to(torch.bfloat16))


def slot_offsets(n, K, packed, ld):
    """element offset of every (row n[i], k) of a stored matrix: slh_gemm_desc.w_layout = 1 (pack_gemm_w) or row-major"""
    k = np.arange(K)[None, :]
    n = np.asarray(n)[:, None]
    if not packed:
        return n * ld + k
    r, s, e = n & 63, (k >> 3) & 7, k & 7
    return ((((n >> 6) * (K >> 6) + (k >> 6)) * 64 + r) << 6) + ((s ^ ((r >> 1) & 7)) << 3) + e


def numpy_merge(items, tensors, pristine, coef):
    """slh_lora_merge restated (include/sliders_hip.h), in float64: for every item, the rows n0 .. n0 + rows of tensors[item.out]."""
    for it in items:
        c = coef[it.c_off:it.c_off + it.R].double().numpy()
        delta = (it.u.double().numpy() * c[None, :]) @ it.d.double().numpy()
        off = slot_offsets(it.n0 + np.arange(it.rows), it.K, it.packed, it.K)
        m = _bf16_to_f64(_bits(pristine[it.base])[off]) + delta
        if it.gamma is None:
            _bits(tensors[it.out])[off] = _round_bf16(m).reshape(off.shape)
            continue
        gamma, beta = (_bf16_to_f64(_bits(tensors[nm])) for nm in (it.gamma, it.beta))
        folded = _round_bf16(m * gamma[None, :]).reshape(off.shape)
        _bits(tensors[it.out])[off] = folded
        rows = slice(it.n0, it.n0 + it.rows)
        tensors[it.lns][rows] = torch.from_numpy(_bf16_to_f64(folded).sum(1)).float()
        tensors[it.lnb][rows] = torch.from_numpy(_bf16_to_f64(_round_bf16(m).reshape(off.shape)) @ beta).float()


@pytest.mark.parametrize("case", CENSUS)
def test_item_table_reaches_every_stored_copy(case):
    """Two sliders (ranks 4 and 8, different alpha) of one train_method on a tiny UNet of the model family: after the restated merge,
    EVERY tensor of the WeightStore equals the one a WeightStore built from the plainly merged state dict holds - the fused q|k|v and
    k|v row ranges, attn2_kv_all.w, the temb_proj.w offsets, the 3x3 K order, and nothing else moved.  The LayerNorm-folded copies
    are defined on the unrounded merge (one rounding), so they are compared with that definition instead."""
    model, method = case.split("/")
    name = "tiny_" + model
    cfg = CONFIGS[name]()
    sd = build_unet(name, seed=0).state_dict()
    sliders = [random_slider(cfg, method, 4, 1.0, seed=1), random_slider(cfg, method, 8, 4.0, seed=2)]
    scales = [1.5, -1.0]
    w = WeightStore(cfg, sd, "cpu")
    mg = WeightMerger(w, SliderSet(cfg, list(zip(sliders, scales))))
    assert mg.items, "the train_method adapts something"
    pristine = {k: v.clone() for k, v in w.t.items()}
    numpy_merge(mg.items, w.t, pristine, mg.coefficients(scales))
    msd = merged_state_dict(cfg, sd, sliders, scales)
    want = WeightStore(cfg, msd, "cpu")
    folded = {n for it in mg.items if it.gamma for n in (it.out, it.lns, it.lnb)}
    assert set(w.t) == set(want.t)
    changed = 0
    for n in w.t:
        if n in folded:
            continue
        assert torch.equal(w.t[n], want.t[n]), f"{case}: {n} differs from the plain merge"
        changed += not torch.equal(w.t[n], pristine[n])
        assert (n in mg.touched) or torch.equal(w.t[n], pristine[n])
    assert changed == len([n for n in mg.touched if n not in folded]), "every touched tensor really changed"
    # folded copies: bf16((W + delta) * gamma), row sums of the stored values, (bias +) bf16(W + delta) . beta
    for it in mg.items:
        if it.gamma is None:
            continue
        src = {".attn1.qkv.lnw": (".attn1.to_q", ".attn1.to_k", ".attn1.to_v"), ".attn2.q.lnw": (".attn2.to_q",)}
        suffix = next(s for s in src if it.out.endswith(s))
        blk = it.out[:-len(suffix)]
        wm = torch.cat([msd[blk + s + ".weight"] for s in src[suffix]], 0)                       # float64, unrounded
        gamma, beta = w.t[it.gamma].double(), w.t[it.beta].double()
        rows = slice(it.n0, it.n0 + it.rows)
        lnw = (wm * gamma[None, :]).to(torch.bfloat16)
        assert torch.equal(w.gemm_matrix(it.out)[rows], lnw[rows]), f"{case}: {it.out} rows {it.n0}.."
        assert torch.allclose(w.t[it.lns][rows].double(), lnw.double().sum(1)[rows], rtol=0, atol=1e-5)
        assert torch.allclose(w.t[it.lnb][rows].double(), (wm.to(torch.bfloat16).double() @ beta)[rows], rtol=0, atol=1e-5)
        assert not torch.equal(w.t[it.out], pristine[it.out])


def test_zero_scales_restate_the_layernorm_fold():
    """c = 0: the restated merge leaves every matrix as it was, and the folded copies are what fold_layernorm made"""
    name = "tiny_sdxl"
    cfg = CONFIGS[name]()
    w = WeightStore(cfg, build_unet(name, seed=0).state_dict(), "cpu")
    mg = WeightMerger(w, SliderSet(cfg, [(random_slider(cfg, "full", 8, 2.0, seed=3), 0.0)]))
    pristine = {k: v.clone() for k, v in w.t.items()}
    numpy_merge(mg.items, w.t, pristine, mg.coefficients([0.0]))
    for n in w.t:
        if n.endswith((".lns", ".lnb")):
            assert torch.allclose(w.t[n], pristine[n], rtol=0, atol=1e-5), n
        else:
            assert torch.equal(w.t[n], pristine[n]), n


def test_rank_alpha_and_targets_are_parsed_from_the_checkpoint():
    cfg = CONFIGS["tiny_sd1"]()
    spec = [(1, 1.0, "xattn"), (4, 2.0, "noxattn"), (8, 8.0, "full"), (16, 4.0, "selfattn")]
    sds = [random_slider(cfg, m, r, a, seed=r, dtype=torch.float32) for r, a, m in spec]
    del sds[3][[k for k in sds[3] if k.endswith(".alpha")][-1]]         # no .alpha key: alpha = rank, like the reference's LoRAModule
    ss = SliderSet(cfg, [(sds[0], 1.0), (sds[1], None), (sds[2], -0.5), (sds[3], 2.0)])
    assert [s.rank for s in ss.sliders] == [1, 4, 8, 16]
    assert ss.scales(3.0) == [1.0, 3.0, -0.5, 2.0]
    for s, (r, a, m) in zip(ss.sliders, spec):
        assert len(s.modules) == len(lora_targets(cfg, m, r))
        assert all(mod.rank == mod.down.shape[0] == mod.up.shape[1] for mod in s.modules)
        assert sorted({mod.alpha for mod in s.modules}) in ([a], sorted({a, float(r)}))
    assert 16.0 in {mod.alpha for mod in ss.sliders[3].modules}
    conv = next(mod for mod in ss.sliders[2].modules if mod.path.endswith("resnets.0.conv1"))
    key = "lora_unet_" + conv.path.replace(".", "_") + ".lora_down.weight"
    assert torch.equal(conv.down, sds[2][key].permute(0, 2, 3, 1).reshape(8, -1)), "3x3 down weights are tap-major"
    # the coefficient vector: scale * alpha / rank per adapter row, concatenated per module in slider order
    w = WeightStore(cfg, build_unet("tiny_sd1", seed=0).state_dict(), "cpu")
    mg = WeightMerger(w, ss)
    it = next(i for i in mg.items if i.path.endswith("attn1.to_q") and i.gamma is None)
    assert it.R == 4 + 8 + 16 and it.u.shape == (it.rows, 28) and it.d.shape == (28, it.K)
    c = mg.coefficients(ss.scales(3.0))[it.c_off:it.c_off + it.R]
    assert torch.equal(c, torch.tensor([3.0 * 2.0 / 4] * 4 + [-0.5 * 8.0 / 8] * 8 + [2.0 * 4.0 / 16] * 16))
    with pytest.raises(ValueError):
        mg.coefficients([1.0])


def test_unknown_and_unmergeable_keys_raise():
    cfg = CONFIGS["tiny_sd1"]()
    sd = random_slider(cfg, "xattn", 4, 1.0, seed=0)
    bad = dict(sd)
    bad["lora_unet_down_blocks_9_attentions_0_proj_in.lora_down.weight"] = torch.zeros(4, 32)
    bad["lora_unet_down_blocks_9_attentions_0_proj_in.lora_up.weight"] = torch.zeros(32, 4)
    with pytest.raises(KeyError, match="down_blocks_9_attentions_0_proj_in"):
        SliderSet(cfg, [(bad, 1.0)])
    wrong = dict(sd)
    k = next(k for k in wrong if k.endswith(".lora_up.weight"))
    wrong[k] = torch.zeros(wrong[k].shape[0] + 8, 4)
    with pytest.raises(ValueError, match="do not fit"):
        SliderSet(cfg, [(wrong, 1.0)])
    # a module of the UNet whose stored layout the merge does not write (GEGLU.proj is held row-permuted, twice)
    names = module_names(cfg)
    ff = next(n for n in names if n.endswith("ff_net_0_proj"))
    node = names[ff][1]
    geglu = {ff + ".lora_down.weight": torch.zeros(4, node.in_dim), ff + ".lora_up.weight": torch.zeros(node.out_dim, 4)}
    w = WeightStore(cfg, build_unet("tiny_sd1", seed=0).state_dict(), "cpu")
    with pytest.raises(NotImplementedError, match="ff.net.0.proj"):
        WeightMerger(w, SliderSet(cfg, [(geglu, 1.0)]))


def test_the_library_validates_merge_items():
    """slh_lora_merge_blocks runs on the host: a row range outside the matrix, a K the layout cannot hold, a fold without its outputs"""
    buf = torch.zeros(128 * 64, dtype=torch.bfloat16)
    f = torch.zeros(64 * 64, dtype=torch.float32)
    ok = dict(base=buf.data_ptr(), out=buf.data_ptr(), u=f.data_ptr(), d=f.data_ptr(), c=f.data_ptr(), n0=32, rows=96, N=128, K=64,
              R=4, ldu=4, ldd=64, ld=0, w_layout=1)
    desc, keep = lib.merge_table([lib.LoraMergeItem(**ok)], "cpu")
    assert desc.n == 1 and desc.total == 2
    for bad in (dict(n0=64), dict(K=32), dict(R=0), dict(ldu=3), dict(w_layout=0, ld=32), dict(gamma=buf.data_ptr()), dict(d=f.data_ptr() + 4)):
        with pytest.raises(lib.SlidersHipError, match="slh_lora_merge"):
            lib.merge_table([lib.LoraMergeItem(**{**ok, **bad})], "cpu")


def test_generate_parser_takes_compose_twice():
    from sliders_amd.generate import build_parser, parse_compose
    a = build_parser().parse_args(["--synthetic", "--compose", "a.pt:1", "--compose", "dir:x/b_rank8.pt:-0.5"])
    assert a.compose == ["a.pt:1", "dir:x/b_rank8.pt:-0.5"]
    assert [parse_compose(c) for c in a.compose] == [("a.pt", 1.0), ("dir:x/b_rank8.pt", -0.5)]
    assert build_parser().parse_args([]).compose == []
    with pytest.raises(SystemExit):
        parse_compose("a.pt")
