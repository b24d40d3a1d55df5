"""GPU: sliders merged into the frozen weights - slh_lora_merge element by element against float64, WeightMerger merge / restore on a
live engine (graphs included), epsilon and the slider's effect against the fp32 oracle with the same merged weights, the sampler and
the CLI.

Tolerances.  Kernel: one bf16 rounding plus fp32 accumulation slack, |got - exact| <= 2^-8 |exact| + 2^-20 (|base| + sum |c u d|), and
at most 0.1 % of the elements away from the correctly rounded float64 value (two plain fp32 evaluations in opposite summation orders
differ on <= 1.5e-4 of the elements on inputs of this kind: weights ~ 0.03 N(0, 1), factors ~ 0.05 N(0, 1)).  Engine: the project's
own criterion (tests/test_parity_r05_gpu.py) - rel_l2(engine, fp32) <= rel_l2(bf16 arm, fp32) + 3e-4 for epsilon, and for the slider's
effect eps(merged) - eps(base) the per-block ratio and floor, err(engine) <= 1.25 err(bf16 arm) + 2e-4; the bf16 arm is the oracle
cast to bfloat16 AFTER the merge.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.lora_oracle import LoRANetworkOracle
from oracle.unet_oracle import build_unet
from sliders_amd import lib
from sliders_amd.config import CONFIGS
from sliders_amd.lora_store import LoraStore
from sliders_amd.merge import SliderSet, WeightMerger, module_names
from sliders_amd.modules import lora_targets
from sliders_amd.random_init import random_state_dict
from sliders_amd.sampler import SliderSampler
from sliders_amd.unet import UNetEngine
from sliders_amd.weights import fold_layernorm, pack_gemm_w
from tests.util import rel_err, stream

pytestmark = pytest.mark.gpu

FENCE = 4096


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel, element by element
# ---------------------------------------------------------------------------------------------------------------------------------
def round_bf16_f64(x):
    """float64 array -> the nearest bf16 value (ties to even), as float64: the correctly rounded result, with no fp32 step between"""
    m, e = np.frexp(x)
    return np.ldexp(np.rint(m * 256.0), e - 8)


def case_inputs(N, K, R, seed):
    """weights ~ 0.03 N(0, 1) (bf16), factors ~ 0.05 N(0, 1) (fp32), coefficients scale * alpha / rank with scales and alphas of the
    sizes sliders are used at"""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * 0.03).to(torch.bfloat16)
    u = torch.randn(N, R, generator=g) * 0.05
    d = torch.randn(R, K, generator=g) * 0.05
    c = torch.tensor([1.5, -1.0, 0.5, 2.0])[torch.randint(0, 4, (R,), generator=g)] * torch.tensor([1.0, 0.5, 0.25])[torch.randint(0, 3, (R,), generator=g)]
    return w, u, d, c.float()


class Arena:
    """One allocation, 0xA5 everywhere, every buffer a view with >= 4 KiB of fence on each side (as tests/gemm_matrix.py)"""

    def __init__(self, dev, sizes):
        self.off, pos = {}, FENCE
        for name, nbytes in sizes.items():
            self.off[name] = pos
            pos = (pos + nbytes + FENCE + 255) // 256 * 256
        self.sizes = sizes
        self.mem = torch.empty(pos, dtype=torch.uint8, device=dev)
        self.mem.fill_(0xA5)
        assert self.mem.data_ptr() % 256 == 0

    def view(self, name, dtype):
        return self.mem[self.off[name]:self.off[name] + self.sizes[name]].view(dtype)

    def ptr(self, name):
        return self.mem.data_ptr() + self.off[name]


def slot_offsets(n, K, packed, ld, dev):
    k = torch.arange(K, device=dev)[None, :]
    n = n.to(dev)[:, None]
    if not packed:
        return n * ld + k
    r, s, e = n & 63, (k >> 3) & 7, k & 7
    return ((((n >> 6) * (K >> 6) + (k >> 6)) * 64 + r) << 6) + ((s ^ ((r >> 1) & 7)) << 3) + e


def _store(w, packed, ld):
    if packed:
        return pack_gemm_w(w)
    out = torch.zeros(w.shape[0], ld, dtype=w.dtype)
    out[:, :w.shape[1]] = w
    return out.reshape(-1)


def run_kernel_case(dev, N, K, R, ranges, packed, fold, seed, zero_c=False, n_stored=None, row_off=0):
    """One stored matrix of n_stored rows (N of them, from row_off, are the module's), `ranges` = [(n0, rows)] relative to row_off, each
    with its own factors; fold: also the LayerNorm-folded copy with a bias.  Returns the figures; asserts every check of the issue."""
    n_stored = n_stored or N
    ld = K if packed else K + 8
    g = torch.Generator().manual_seed(seed + 1)
    wfull = (torch.randn(n_stored, K, generator=g) * 0.03).to(torch.bfloat16)
    gamma = (1.0 + 0.2 * torch.randn(K, generator=g)).to(torch.bfloat16)
    beta = (0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    bias = (0.1 * torch.randn(n_stored, generator=g)).to(torch.bfloat16)
    facs = []
    for i, (n0, rows) in enumerate(ranges):
        w_, u, d, c = case_inputs(rows, K, R, seed + 10 * i)
        wfull[row_off + n0:row_off + n0 + rows] = w_
        facs.append((u, d, torch.zeros_like(c) if zero_c else c))
    stored = _store(wfull, packed, ld)
    nel = stored.numel()
    sizes = {"base": 2 * nel, "out": 2 * nel, "lnw": 2 * nel, "lns": 4 * n_stored, "lnb": 4 * n_stored, "gamma": 2 * K, "beta": 2 * K,
             "bias": 2 * n_stored}
    for i, (u, d, c) in enumerate(facs):
        sizes.update({f"u{i}": 4 * u.numel(), f"d{i}": 4 * d.numel(), f"c{i}": 4 * c.numel()})
    ar = Arena(dev, sizes)
    BF, F32 = torch.bfloat16, torch.float32
    ar.view("base", BF).copy_(stored)
    ar.view("out", BF).copy_(stored)            # the live tensor: rows outside the items (and the pad rows) must stay as they are
    ar.view("lnw", BF).copy_(_store(fold_layernorm(wfull, None, gamma, beta)[0], packed, ld) if fold else stored)
    for nm, t in (("gamma", gamma), ("beta", beta), ("bias", bias)):
        ar.view(nm, BF).copy_(t)
    items = []
    for i, ((n0, rows), (u, d, c)) in enumerate(zip(ranges, facs)):
        for nm, t in ((f"u{i}", u), (f"d{i}", d), (f"c{i}", c)):
            ar.view(nm, F32).copy_(t.reshape(-1))
        common = dict(base=ar.ptr("base"), u=ar.ptr(f"u{i}"), d=ar.ptr(f"d{i}"), c=ar.ptr(f"c{i}"), n0=row_off + n0, rows=rows, N=n_stored,
                      K=K, R=R, ldu=R, ldd=K, ld=0 if packed else ld, w_layout=1 if packed else 0)
        items.append(lib.LoraMergeItem(out=ar.ptr("out"), **common))
        if fold:
            items.append(lib.LoraMergeItem(out=ar.ptr("lnw"), gamma=ar.ptr("gamma"), beta=ar.ptr("beta"), bias=ar.ptr("bias"),
                                           lns=ar.ptr("lns"), lnb=ar.ptr("lnb"), **common))
    desc, keep = lib.merge_table(items, dev)
    before = ar.mem.clone()
    lib.call(lib.OP_LORA_MERGE, desc, stream())
    torch.cuda.synchronize()
    first = ar.mem.clone()
    ar.mem.copy_(before)
    lib.call(lib.OP_LORA_MERGE, desc, stream())
    torch.cuda.synchronize()
    assert torch.equal(ar.mem, first), "two runs differ"
    # fences, inputs, the rows outside the items and the pad rows: nothing but the items' own elements may change
    allowed = torch.zeros(ar.mem.numel(), dtype=torch.bool, device=dev)
    for n0, rows in ranges:
        off = slot_offsets(row_off + n0 + torch.arange(rows), K, packed, ld, dev).reshape(-1)
        for nm in ("out",) + (("lnw",) if fold else ()):
            allowed[ar.off[nm] + 2 * off] = True
            allowed[ar.off[nm] + 2 * off + 1] = True
        if fold:
            for nm in ("lns", "lnb"):
                a = ar.off[nm] + 4 * (row_off + n0)
                allowed[a:a + 4 * rows] = True
    stray = (ar.mem != before) & ~allowed
    assert not bool(stray.any()), f"{int(stray.sum())} bytes written outside the items' elements (first at {int(stray.nonzero()[0])})"
    out, lnw = ar.view("out", BF), ar.view("lnw", BF)
    if packed and n_stored % 64:
        npad = (n_stored + 63) // 64 * 64
        pad = slot_offsets(torch.arange(n_stored, npad), K, True, 0, dev).reshape(-1)
        assert not bool(out[pad].float().abs().any()) and not bool(lnw[pad].float().abs().any()), "pad rows must stay zero"
    fig = dict(worst=0.0, misrounded=0, n=0, worst_lns=0.0, worst_lnb=0.0)
    for (n0, rows), (u, d, c) in zip(ranges, facs):
        rs = slice(row_off + n0, row_off + n0 + rows)
        off = slot_offsets(row_off + n0 + torch.arange(rows), K, packed, ld, dev)
        base64 = wfull[rs].double().to(dev)
        cu = (c.double()[None, :] * u.double()).to(dev)
        d64 = d.double().to(dev)
        exact = base64 + cu @ d64
        sabs = base64.abs() + cu.abs() @ d64.abs()
        got = out[off].double()
        bound = 2.0 ** -8 * exact.abs() + 2.0 ** -20 * sabs
        ratio = ((got - exact).abs() / bound.clamp_min(1e-300)).max().item() if not zero_c else 0.0
        fig["worst"] = max(fig["worst"], ratio)
        assert bool(((got - exact).abs() <= bound).all()), f"merge beyond the bound: worst |got - exact| / bound = {ratio:.3g}"
        cr = torch.from_numpy(round_bf16_f64(exact.cpu().numpy())).to(dev)
        fig["misrounded"] += int((got != cr).sum())
        fig["n"] += got.numel()
        if zero_c:
            assert torch.equal(out[off], wfull[rs].to(dev)), "c = 0 must give base exactly"
        if fold:
            gm, bt = gamma.double().to(dev), beta.double().to(dev)
            lw = lnw[off].double()
            ex = exact * gm[None, :]
            bnd = 2.0 ** -8 * ex.abs() + 2.0 ** -20 * sabs * gm.abs()[None, :]
            assert bool(((lw - ex).abs() <= bnd).all()), "folded copy beyond the bound"
            lns, lnb = ar.view("lns", F32)[rs].double(), ar.view("lnb", F32)[rs].double()
            e_s = (lns - lw.sum(1)).abs() / (K * 2.0 ** -24 * lw.abs().sum(1))
            merged = got                                     # bf16(merged), as the kernel stored it in `out`
            want_b = bias.double().to(dev)[rs] + merged @ bt
            ulp = 2.0 ** (torch.floor(torch.log2(want_b.abs().clamp_min(1e-30))) - 23)
            e_b = (lnb - want_b).abs() / (K * 2.0 ** -24 * (merged.abs() @ bt.abs()) + ulp)
            fig["worst_lns"], fig["worst_lnb"] = max(fig["worst_lns"], e_s.max().item()), max(fig["worst_lnb"], e_b.max().item())
            assert e_s.max().item() <= 1.0, f"lns off by {e_s.max().item():.3g} x its bound"
            assert e_b.max().item() <= 1.0, f"lnb off by {e_b.max().item():.3g} x its bound"
            if zero_c:
                wf, s_, b_ = fold_layernorm(wfull[rs], bias[rs], gamma, beta)
                assert torch.equal(lnw[off], wf.to(dev)), "c = 0: the folded copy is fold_layernorm's"
    share = fig["misrounded"] / max(fig["n"], 1)
    print(f"[merge] N={N} K={K} R={R} packed={packed} fold={fold} ranges={ranges}: worst err / bound {fig['worst']:.3f}, not correctly rounded "
          f"{fig['misrounded']} of {fig['n']} ({share:.2e}), lns {fig['worst_lns']:.3f} lnb {fig['worst_lnb']:.3f} of their bounds")
    assert share <= 1e-3, f"{share:.3e} of the elements are not the correctly rounded value"
    return fig


def _layouts(N):
    """the stored layouts of WeightMerger's item table at this N: (ranges, packed, fold, n_stored, row_off)"""
    if N == 3840:      # fused q|k|v: three row ranges with their own factors (two begin inside the matrix), with the LayerNorm-folded copy
        return [([(0, 1280), (1280, 1280), (2560, 1280)], True, True, None, 0)]
    if N == 1280:      # attn2.to_q with its fold; k|v: the V half of a fused [2C] matrix = a range inside attn2_kv_all.w
        return [([(0, 1280)], True, True, None, 0), ([(0, 1280)], True, False, 2 * 1280 + 640, 1280)]
    if N == 320:       # a plain matrix (out / conv / proj), and rows of the concatenated row-major temb_proj.w
        return [([(0, 320)], True, False, None, 0), ([(0, 320)], False, False, 1000, 360)]
    # N = 96: pad rows 96..128; two ranges sharing a 64-row block (tiny nets: C = 32); row-major (SLIDERS_W_ROWMAJOR=1)
    return [([(0, 96)], True, False, None, 0), ([(0, 32), (32, 64)], True, True, None, 0), ([(0, 96)], False, False, None, 0)]


@pytest.mark.parametrize("R", [1, 4, 12, 28, 64])
@pytest.mark.parametrize("K", [640, 1280, 2880])
@pytest.mark.parametrize("N", [96, 320, 1280, 3840])
def test_merge_kernel_elementwise(dev, N, K, R):
    for li, (ranges, packed, fold, n_stored, row_off) in enumerate(_layouts(N)):
        run_kernel_case(dev, N, K, R, ranges, packed, fold, seed=1000 * li + N + K + R, n_stored=n_stored, row_off=row_off)


@pytest.mark.parametrize("N,K,R", [(96, 640, 4), (3840, 1280, 28), (320, 2880, 12)])
def test_merge_kernel_zero_coefficients(dev, N, K, R):
    for li, (ranges, packed, fold, n_stored, row_off) in enumerate(_layouts(N)):
        run_kernel_case(dev, N, K, R, ranges, packed, fold, seed=77 + li, zero_c=True, n_stored=n_stored, row_off=row_off)


# ---------------------------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------------------------
def drawn_slider(cfg, method, rank, alpha, seed, std=0.05):
    """Adapter values drawn the way the existing parity tests draw them (tests/test_bench_config_gpu.py _nonzero_up over the
    reference's initialisation): lora_down kaiming_uniform(a = 1), lora_up ~ std N(0, 1), both bf16."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for t in lora_targets(cfg, method, rank):
        k = 3 if t.kind == "conv3" else 1
        down = torch.empty((t.rank, t.in_dim) if t.kind == "linear" else (t.rank, t.in_dim, k, k))
        nn.init.kaiming_uniform_(down, a=1.0, generator=g)
        up = torch.randn((t.out_dim, t.rank) if t.kind == "linear" else (t.out_dim, t.rank, 1, 1), generator=g) * std
        sd[f"{t.lora_name}.alpha"] = torch.tensor(float(alpha))
        sd[f"{t.lora_name}.lora_down.weight"] = down.to(torch.bfloat16)
        sd[f"{t.lora_name}.lora_up.weight"] = up.to(torch.bfloat16)
    return sd


def merged_weights(cfg, sd, sliders, scales, dtype, dev):
    """weight + sum_i s_i (alpha_i / r_i) B_i A_i in float64 on the bf16 weights, THEN cast to dtype"""
    names = module_names(cfg)
    by_path = {}
    for lsd, s in zip(sliders, scales):
        for key in lsd:
            if key.endswith(".lora_down.weight"):
                name = key[:-len(".lora_down.weight")]
                down, up = lsd[key], lsd[f"{name}.lora_up.weight"]
                r = down.shape[0]
                alpha = float(lsd[f"{name}.alpha"]) if f"{name}.alpha" in lsd else float(r)
                by_path.setdefault(names[name][0], []).append((s * alpha / r, up.reshape(up.shape[0], r), down))
    out = {}
    for k, v in sd.items():
        v = v.to(dev)
        mods = by_path.get(k[:-len(".weight")]) if k.endswith(".weight") else None
        if mods is None:
            out[k] = v.to(torch.bfloat16).to(dtype)
            continue
        w = v.to(torch.bfloat16).double()
        for coef, up, down in mods:
            w = w + coef * torch.einsum("or,r...->o...", up.to(dev).double(), down.to(dev).double()).reshape(w.shape)
        out[k] = w.to(dtype)
    return out


def _net(name, sd):
    net = build_unet(name, device="meta")
    net.load_state_dict(sd, assign=True)
    net.requires_grad_(False)
    return net.eval()


def _eps(net, x, t, ctx, kw, dtype, dev):
    r = lambda a: a.to(torch.bfloat16).to(device=dev, dtype=dtype)
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
        return net(r(x), torch.tensor(t, device=dev), r(ctx), {k: r(v) for k, v in kw.items()} if kw else None).sample.float().cpu()


def _inputs(cfg, B, hw, seed=1234):
    from tests.test_unet_gpu import make_inputs
    return make_inputs(cfg, B, hw, seed)


def _engine_eps(eng, x, t, ctx, kw, dev, mode="off"):
    kwd = {k: v.to(dev) for k, v in kw.items()} if kw else None
    out = eng(x.to(dev), torch.tensor(t), ctx.to(dev), kwd, mode=mode).sample.float().cpu()
    torch.cuda.synchronize()
    return out


def _tiny_engine(name, dev):
    cfg = CONFIGS[name]()
    sd = build_unet(name, seed=0).state_dict()
    return cfg, sd, UNetEngine(cfg, sd, dev)


def test_restore_puts_back_every_bit_and_graphs_see_the_merge(dev):
    name, hw, t = "tiny_sdxl", 16, 500
    cfg, sd, eng = _tiny_engine(name, dev)
    sliders = [drawn_slider(cfg, "full", 8, 4.0, 1), drawn_slider(cfg, "xattn", 4, 1.0, 2)]
    mg = WeightMerger(eng.w, SliderSet(cfg, [(sliders[0], 1.0), (sliders[1], -1.0)]))
    x, ctx, kw = _inputs(cfg, 2, hw)
    snap = {k: v.clone() for k, v in eng.w.t.items()}
    p = eng.plan(2, hw, hw, "off")
    eps0 = _engine_eps(eng, x, t, ctx, kw, dev)
    assert p.prog.capture(), "the pass is long enough to be captured"
    assert torch.equal(_engine_eps(eng, x, t, ctx, kw, dev), eps0)
    mg.merge([1.0, -1.0])
    replayed = _engine_eps(eng, x, t, ctx, kw, dev)                  # the graph captured on the base weights
    p.prog.run(stream(), graph=False)
    torch.cuda.synchronize()
    fresh = p.io["eps"].tensor.clone().float().cpu()
    assert torch.equal(replayed, fresh), "a captured graph reads the merged weights through the same pointers"
    assert rel_err(fresh, eps0) > 1e-3, "the merge has a visible effect"
    assert any(not torch.equal(eng.w.t[n], snap[n]) for n in mg.touched)
    mg.merge([1.0, -1.0])                                            # always from the pristine bits: no accumulation
    assert torch.equal(_engine_eps(eng, x, t, ctx, kw, dev), fresh)
    mg.restore()
    for k, v in eng.w.t.items():
        assert torch.equal(v, snap[k]), f"{k} not restored"
    assert torch.equal(_engine_eps(eng, x, t, ctx, kw, dev), eps0)
    eng.weights._dgrad_ready = True
    with pytest.raises(RuntimeError, match="no-grad"):
        mg.merge([1.0, -1.0])
    eng.weights._dgrad_ready = False


PARITY = {}          # (config, case) -> figures, shared by the epsilon and the effect test


def _record(key, fig):
    path = os.environ.get("SLIDERS_MERGE_PARITY_JSON")
    print(f"[merge-parity] {key}: {json.dumps(fig)}")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[key] = fig
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)


def _parity(dev, name, hw, case):
    key = f"{name}@{hw}/{case}"
    if key in PARITY:
        return PARITY[key]
    cfg = CONFIGS[name]()
    tiny = name.startswith("tiny")
    sd = build_unet(name, seed=0).state_dict() if tiny else random_state_dict(cfg, dev, 0, torch.bfloat16)
    eng = UNetEngine(cfg, sd, dev)
    x, ctx, kw = _inputs(cfg, 2, hw)
    t = 781
    store = None
    if case == "a":
        from tests.test_bench_config_gpu import _nonzero_up
        store = LoraStore(cfg, rank=4, alpha=1.0, train_method="noxattn", device=dev)
        _nonzero_up(store, dev)
        sliders, scales = [store.state_dict()], [1.0]
    else:
        sliders = [drawn_slider(cfg, "noxattn", 4, 1.0, 11), drawn_slider(cfg, "full", 8, 4.0, 12), drawn_slider(cfg, "xattn", 16, 8.0, 13)]
        scales = [1.5, -1.0, 0.5]
    mg = WeightMerger(eng.w, SliderSet(cfg, list(zip(sliders, scales))))
    g_base = _engine_eps(eng, x, t, ctx, kw, dev)
    mg.merge(scales)
    g_merged = _engine_eps(eng, x, t, ctx, kw, dev)
    mg.restore()
    g_fused = None
    if store is not None:
        eng.attach_lora(store)
        eng.set_lora(True, 1.0)
        g_fused = _engine_eps(eng, x, t, ctx, kw, dev, mode="on")
        eng.set_lora(False)
    del eng, mg
    torch.cuda.empty_cache()
    arms = {}
    for dt, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        for merged in (False, True):
            net = _net(name, merged_weights(cfg, sd, sliders if merged else [], scales if merged else [], dt, dev))
            arms[tag, merged] = _eps(net, x, t, ctx, kw, dt, dev)
            if merged and dt == torch.float32 and case == "a":
                # the same truth built the reference's way: the fp32 oracle with its LoRA modules switched on
                base = _net(name, merged_weights(cfg, sd, [], [], dt, dev))
                nw = LoRANetworkOracle(base, rank=4, multiplier=1.0, alpha=1.0, train_method="noxattn")
                nw.load_state_dict(sliders[0], strict=True)
                nw.to(device=dev, dtype=dt)
                nw.set_lora_slider(1.0)
                with nw:
                    e_lora = _eps(base, x, t, ctx, kw, dt, dev)
                arms["lora"] = rel_err(arms[tag, merged], e_lora)
                del base, nw
            del net
            torch.cuda.empty_cache()
    e32, e32b, ebf, ebfb = arms["f32", True], arms["f32", False], arms["bf16", True], arms["bf16", False]
    d32 = e32 - e32b
    cos = lambda a: F.cosine_similarity(a.flatten(), d32.flatten(), dim=0).item()
    fig = dict(eps_engine=rel_err(g_merged, e32), eps_bf16_arm=rel_err(ebf, e32), effect_size=rel_err(e32, e32b),
               effect_engine=rel_err(g_merged - g_base, d32), effect_bf16_arm=rel_err(ebf - ebfb, d32),
               cos_engine=cos(g_merged - g_base), cos_bf16_arm=cos(ebf - ebfb), finite=bool(torch.isfinite(g_merged).all()))
    if g_fused is not None:
        fig.update(effect_fused=rel_err(g_fused - g_base, d32), cos_fused=cos(g_fused - g_base), eps_fused=rel_err(g_fused, e32),
                   oracle_merged_vs_lora_modules=arms["lora"])
    _record(key, fig)
    PARITY[key] = fig
    return fig


CONFIGS_PARITY = [("tiny_sd1", 16), ("tiny_sd2", 16), ("tiny_sdxl", 16), ("sdxl", 128), ("sd1", 64)]


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("name,hw", CONFIGS_PARITY)
def test_merged_epsilon_parity(dev, name, hw, case):
    """(a) one rank-4 noxattn slider, (b) three sliders of ranks 4 / 8 / 16 with alpha 1 / 4 / 8 (noxattn, full, xattn: attn2 k / v and
    attn2_kv_all are hit) at scales +1.5, -1, +0.5: epsilon on the merged weights against the fp32 oracle with the same sum added to its
    weights in float64."""
    f = _parity(dev, name, hw, case)
    assert f["finite"] and f["effect_size"] > 1e-3, "the sliders have a visible effect"
    if case == "a":
        # two fp32 statements of one function: they differ by the fp32 rounding of W + delta (2^-24 per weight), far below 1e-4
        assert f["oracle_merged_vs_lora_modules"] <= 1e-4, f
    assert f["eps_engine"] <= f["eps_bf16_arm"] + 3e-4, f"{name} {case}: engine {f['eps_engine']:.3e} vs bf16 arm {f['eps_bf16_arm']:.3e}"


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("name,hw", CONFIGS_PARITY)
def test_merged_slider_effect_parity(dev, name, hw, case):
    """The slider's effect eps(merged) - eps(base) against the fp32 oracle's: err(engine) <= 1.25 err(bf16 merged-weights arm) + 2e-4."""
    f = _parity(dev, name, hw, case)
    assert f["effect_engine"] <= 1.25 * f["effect_bf16_arm"] + 2e-4, \
        f"{name} {case}: effect error engine {f['effect_engine']:.3e} vs bf16 arm {f['effect_bf16_arm']:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------------
# sampler, CLI
# ---------------------------------------------------------------------------------------------------------------------------------
def _hand_loop(eng, smp, mg, scales, ctx, noise, pooled, start_noise, steps, gs, cached=True):
    """base steps, merge, off-plan steps, restore - written out; cached = False never uses prog_text_cached"""
    bs, _, h, w = noise.shape
    p = eng.plan(2 * bs, h, w, "off")
    io = p.io
    io["ctx"].tensor.copy_(ctx.to(torch.bfloat16))
    if eng.cfg.is_xl:
        io["time_ids"].tensor.copy_(torch.tensor([[h * 8.0, w * 8.0, 0.0, 0.0, h * 8.0, w * 8.0]] * (2 * bs)).to(eng.device))
        io["add_in"].tensor[:, : eng.cfg.pooled_dim].copy_(pooled.to(torch.bfloat16))
    s = stream()
    sch = smp.sched
    merged = False
    if sch.fused:
        lat = noise.to(eng.device, torch.bfloat16)
        io["sample"].tensor[:bs].copy_(lat)
        io["sample"].tensor[bs:].copy_(lat)
        chw = eng.cfg.out_channels * h * w
        for i, t in enumerate(sch.make_timesteps(steps)):
            full = i == 0 or not cached
            if not merged and not t > start_noise:
                mg.merge(scales)
                merged = full = True
            io["t"].tensor.fill_(float(t))
            (p.prog if full or p.prog_text_cached is None else p.prog_text_cached).run(s)
            lib.call(lib.OP_CFG_DDIM, lib.CfgDdimDesc(eps=io["eps"].ptr, x=io["sample"].ptr, out=io["sample"].ptr, out2=io["sample"].ptr + bs * chw * 2,
                                                      nb=bs, chw=chw, guidance=gs, **sch.step_fields(t, steps)), s)
        out = io["sample"].tensor[:bs].clone()
    else:
        sch.set_timesteps(steps, device=eng.device)
        lat = (noise.to(eng.device, torch.float32) * sch.init_noise_sigma).to(torch.bfloat16)
        eps = torch.empty_like(lat)
        for i, t in enumerate(sch.timesteps):
            full = i == 0 or not cached
            if not merged and not float(t) > start_noise:
                mg.merge(scales)
                merged = full = True
            xin = sch.scale_model_input(lat, t)
            io["sample"].tensor[:bs].copy_(xin)
            io["sample"].tensor[bs:].copy_(xin)
            io["t"].tensor.fill_(float(t))
            (p.prog if full or p.prog_text_cached is None else p.prog_text_cached).run(s)
            lib.call(lib.OP_CFG_DDIM, lib.CfgDdimDesc(eps=io["eps"].ptr, x=0, out=eps.data_ptr(), out2=0, nb=bs, chw=lat[0].numel(),
                                                      guidance=gs, do_step=0), s)
            lat = sch.step(eps, t, lat, generator=None).prev_sample
        out = lat
    mg.restore()
    torch.cuda.synchronize()
    return out, merged


@pytest.mark.parametrize("scheduler", ["ddim", "euler"])
def test_sampler_merges_at_start_noise_and_restores(dev, scheduler):
    name, hw, steps, gs = "tiny_sdxl", 16, 8, 5.0
    cfg, sd, eng = _tiny_engine(name, dev)
    g = torch.Generator().manual_seed(5)
    ctx = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).to(dev)
    pooled = torch.randn(2, cfg.pooled_dim, generator=g).to(dev)
    noise = torch.randn(1, 4, hw, hw, generator=g).to(dev)
    sliders = SliderSet(cfg, [(drawn_slider(cfg, "xattn", 8, 4.0, 21), None), (drawn_slider(cfg, "noxattn", 4, 1.0, 22), -1.0)])
    snap = {k: v.clone() for k, v in eng.w.t.items()}
    smp = SliderSampler(eng, scheduler=scheduler, sliders=sliders)
    plain = SliderSampler(eng, scheduler=scheduler)
    kw = dict(ddim_steps=steps, guidance_scale=gs, pooled=pooled)
    base = plain.sample_latents(ctx, noise, **kw)
    assert eng.plan(2, hw, hw, "off").prog_text_cached is not None, "the test needs the text-cached program"
    outs = {}
    for start, want_merge in ((2000, True), (500, True), (-1, False)):      # above the first timestep, inside the loop, below the last
        got = smp.sample_latents(ctx, noise, scale=1.5, start_noise=start, **kw)
        assert not smp.merger.merged and all(torch.equal(v, snap[k]) for k, v in eng.w.t.items()), "restored when the image is done"
        hand, merged = _hand_loop(eng, smp, smp.merger, [1.5, -1.0], ctx, noise, pooled, start, steps, gs)
        assert merged == want_merge
        assert torch.equal(got, hand), f"start_noise {start}: sampler and the hand-written loop differ"
        # an xattn slider changes attn2 k / v: the step after the merge must project the text again - as a run that never uses
        # prog_text_cached does
        uncached, _ = _hand_loop(eng, smp, smp.merger, [1.5, -1.0], ctx, noise, pooled, start, steps, gs, cached=False)
        assert torch.equal(got, uncached), f"start_noise {start}: stale cross-attention K/V after the merge"
        outs[start] = got
    assert torch.equal(outs[-1], base) and not torch.equal(outs[500], base) and not torch.equal(outs[2000], outs[500])
    # every scale 0: the no-slider sampler
    zero = SliderSampler(eng, scheduler=scheduler, sliders=SliderSet(cfg, [(drawn_slider(cfg, "full", 8, 4.0, 23), None),
                                                                            (drawn_slider(cfg, "xattn", 4, 1.0, 24), 0.0)]))
    assert torch.equal(zero.sample_latents(ctx, noise, scale=0.0, start_noise=500, **kw), base)

    # an exception inside the loop still restores the weights
    class Boom(RuntimeError):
        pass

    real = smp.sched.step_fields if scheduler == "ddim" else smp.sched.step
    calls = []

    def failing(*a, **k):
        calls.append(1)
        if len(calls) == steps:
            raise Boom()
        return real(*a, **k)
    setattr(smp.sched, "step_fields" if scheduler == "ddim" else "step", failing)
    with pytest.raises(Boom):
        smp.sample_latents(ctx, noise, scale=1.5, start_noise=2000, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(v, snap[k]) for k, v in eng.w.t.items())


def test_generate_composes_sliders_and_the_fused_path_refuses_other_ranks(dev, tmp_path):
    from sliders_amd import generate
    cfg = CONFIGS["sd1"]()
    a, b = str(tmp_path / "age_alpha4.0_rank8_full.pt"), str(tmp_path / "smile_alpha1.0_rank4_noxattn.pt")
    torch.save(drawn_slider(cfg, "full", 8, 4.0, 31), a)
    torch.save(drawn_slider(cfg, "noxattn", 4, 1.0, 32), b)
    out = generate.main(["--model", "sd1", "--synthetic", "--compose", a + ":1", "--compose", b + ":-1", "--scales=0", "--ddim_steps", "3",
                         "--res", "256", "--out", str(tmp_path / "composed")])
    assert os.path.getsize(os.path.join(out, "scale_0.png")) > 0
    # the swept slider is rank 8: merged as well, one image per scale, and the scale matters
    out = generate.main(["--model", "sd1", "--synthetic", "--lora_weight", a, "--scales=-1,1", "--ddim_steps", "3", "--res", "256",
                         "--out", str(tmp_path / "swept")])
    imgs = [open(os.path.join(out, f"scale_{s}.png"), "rb").read() for s in ("-1", "1")]
    assert imgs[0] and imgs[1] and imgs[0] != imgs[1]
    eng = UNetEngine(CONFIGS["tiny_sd1"](), build_unet("tiny_sd1", seed=0).state_dict(), dev)
    store = LoraStore.__new__(LoraStore)
    store.rank = 8
    with pytest.raises(NotImplementedError, match="rank 4.*merge"):
        eng.attach_lora(store)
