"""Per-token cross-attention maps without a device: the descriptor and what slh_xattn_map refuses, the per-element bound against a
plain-torch stand-in of the kernel's arithmetic and its mutants (tests/xattn_map_matrix.py), the maps plans as dry runs, and the host
functions of sliders_amd/edit.py (word_token_indices, word_mask, level_mean / word_map_reference, check_args)."""
import ctypes as C
import zlib

import pytest
import torch

from sliders_amd import edit, lib
from sliders_amd.arena import Arena
from sliders_amd.config import CONFIGS
from sliders_amd.modules import build_tree
from sliders_amd.planner import AttnMapSpec, UNetPlan
from tests import xattn_map_matrix as xm
from tests.test_host import _FakeWeights, library_ops


# ---------------------------------------------------------------------------------------------------------------------------
# descriptor and refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_opcode_entry_and_descriptor_size():
    assert lib.OP_XATTN_MAP == 42
    assert lib._ENTRY[lib.OP_XATTN_MAP] == ("slh_xattn_map", lib.XattnMapDesc)
    assert "slh_xattn_map" in lib.EXPORTS
    assert library_ops()[42] == ("slh_xattn_map", C.sizeof(lib.XattnMapDesc)), "the library's own table lists opcode 42 so"
    assert C.sizeof(lib.XattnMapDesc) == 4 * 8 + 9 * 4 + 2 * 4 + 4


def _good(**kw):
    d = dict(q=0x10000, k=0x20000, wt=0x30000, out=0x40000, B=2, b0=1, nb=1, H=2, D=64, Tq=64, Tk=77, ldq=128, ldk=384, scale=0.125,
             coef=0.5, accumulate=0)
    d.update(kw)
    return lib.XattnMapDesc(**d)


REFUSED = {
    "D = 12": dict(D=12), "D = 200": dict(D=200, ldq=400, ldk=400), "D = 0": dict(D=0), "Tk = 0": dict(Tk=0), "Tk = 129": dict(Tk=129),
    "Tq = 0": dict(Tq=0), "H = 0": dict(H=0), "b0 + nb > B": dict(b0=1, nb=2), "b0 < 0": dict(b0=-1), "nb = 0": dict(nb=0),
    "ldk < H D": dict(ldk=120), "ldq < H D": dict(ldq=64), "ldk % 8": dict(ldk=132), "ldq % 8": dict(ldq=130),
    "null wt": dict(wt=0), "null q": dict(q=0), "null k": dict(k=0), "null out": dict(out=0), "unaligned k": dict(k=0x20008),
    "accumulate = 2": dict(accumulate=2),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refused_before_launch(what):
    """every one returns before any device call (this runs without a GPU) and names the entry point"""
    with pytest.raises(lib.SlidersHipError, match="slh_xattn_map"):
        lib.call(lib.OP_XATTN_MAP, _good(**REFUSED[what]), 0)


def test_refused_through_a_program():
    prog = lib.Program()
    prog.add(lib.OP_XATTN_MAP, _good(Tk=129), "map")
    with pytest.raises(lib.SlidersHipError, match="slh_xattn_map: Tk = 129"):
        prog.run(0, graph=False)


# ---------------------------------------------------------------------------------------------------------------------------
# the bound against the stand-in and its mutants
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    """case id -> (inputs, float64 reference, bound): computed once for the tests below"""
    out = {}
    for c in xm.CASES:
        L = xm.inputs(c, zlib.crc32(c.id.encode()) % (2 ** 31))
        out[c.id] = (L,) + xm.reference(c, L)
    return out


def test_matrix_covers_the_edges():
    cs = xm.CASES
    assert 120 <= len(cs) <= 160 and len({c.id for c in cs}) == len(cs)
    for name, vals in (("Tq", (1, 63, 64, 65, 256)), ("Tk", (1, 64, 65, 77, 128)), ("D", (8, 40, 64, 160)), ("H", (1, 2, 5)),
                       ("ldk_mult", (3, 1)), ("acc", (0, 1)), ("cls", xm.CLASSES), ("wt", xm.WT_KINDS)):
        assert {getattr(c, name) for c in cs} == set(vals), name
    assert {(c.b0, c.nb) for c in cs} == {(1, 1), (0, 2)}
    assert {(c.cls, c.wt) for c in cs if c.Tk == 77 and c.D == 64} >= {(a, b) for a in ("normal", "shift", "last", "zeroq") for b in xm.WT_KINDS}


def test_standin_stays_inside_the_bound(sweep):
    worst, at = 0.0, ""
    for c in xm.CASES:
        L, ref, bound = sweep[c.id]
        assert bool(torch.isfinite(ref).all()) and bool((bound > 0).all()) and bool(torch.isfinite(bound).all()), c.id
        r = float(((xm.standin(c, L).double() - ref).abs() / bound).max())
        assert r <= 1.0, f"{c.id}: the stand-in is {r:.3f} bounds away from float64"
        if r > worst:
            worst, at = r, c.id
        cf = xm.closed_form(c, L)
        if cf is not None:          # all-ones weights: coef H; all-zero q: coef H sum(wt) / Tk - the reference itself, up to float64
            assert bool(((cf - ref).abs() <= 1e-12 * (1 + ref.abs())).all()), c.id
    print(f"worst stand-in |got - ref| / bound = {worst:.3f} ({at})")


@pytest.mark.parametrize("mutant", xm.MUTANTS)
def test_mutant_breaks_the_bound(sweep, mutant):
    caught = []
    for c in xm.CASES:
        L, ref, bound = sweep[c.id]
        if bool(((xm.standin(c, L, mutant).double() - ref).abs() > bound).any()):
            caught.append(c.id)
    assert len(caught) >= 5, f"{mutant}: caught by {caught}"


# ---------------------------------------------------------------------------------------------------------------------------
# plans, dry run
# ---------------------------------------------------------------------------------------------------------------------------
def _plan(name, hw, spec, mode="off", store=None):
    cfg = CONFIGS[name]()
    return cfg, UNetPlan(cfg, _FakeWeights(cfg), Arena(1 << 50, None), Arena(1 << 40, None), 2, hw, hw, 77, store, mode, 0x10, attn_maps=spec)


def _attn2_per_factor(cfg):
    """factor -> number of attn2 modules, from the module tree: a block's factor is 2^(its down level), the up blocks mirror the
    down blocks, the mid block sits at the last level"""
    n = len(cfg.block_out_channels)
    out = {}

    def walk(node, path):
        kids = getattr(node, "children", None)
        kids = kids.values() if isinstance(kids, dict) else (kids or [])
        for ch in kids:
            p = f"{path}.{ch.name}" if path else ch.name
            if ch.name == "attn2":
                top = p.split(".")
                level = int(top[1]) if top[0] == "down_blocks" else n - 1 - int(top[1]) if top[0] == "up_blocks" else n - 1
                out[2 ** level] = out.get(2 ** level, 0) + 1
            walk(ch, p)
    walk(build_tree(cfg), "")
    return out


@pytest.mark.parametrize("name,expect", [("tiny_sdxl", {2: 5, 4: 12}), ("tiny_sd1", None)])
def test_maps_plan_records_one_op_per_collected_attn2(name, expect):
    cfg, p0 = _plan(name, 16, None)
    _, p = _plan(name, 16, {"max_factor": 4})
    tree = _attn2_per_factor(cfg)
    want = {f: c for f, c in tree.items() if f <= 4}
    if expect is not None:
        assert want == expect
    else:
        assert set(want) == {1, 2, 4} and 8 in tree            # SD-1.x: the 8x level (the mid block) is left out
    ops = [(nm, d) for o, d, nm in p.ops if o == lib.OP_XATTN_MAP]
    assert not [1 for o, _, _ in p0.ops if o == lib.OP_XATTN_MAP]
    assert len(ops) == sum(want.values())
    per = {}
    for nm, d in ops:
        assert nm.endswith(".attn2.map")
        f = int(round((16 * 16 / d.Tq) ** 0.5))
        per.setdefault(f, []).append(d)
        # it sits right behind its own attention launch
        names = [n for _, _, n in p.ops]
        assert names[names.index(nm) - 1] == nm[:-len(".map")] + ".sdpa"
    assert {f: len(v) for f, v in per.items()} == want
    for f, ds in per.items():
        assert [d.accumulate for d in ds] == [0] + [1] * (len(ds) - 1)
        for d in ds:
            assert d.coef == pytest.approx(1.0 / (d.H * len(ds)), rel=1e-7) and d.scale == pytest.approx(d.D ** -0.5, rel=1e-7)
            assert (d.B, d.b0, d.nb, d.Tk) == (2, 1, 1, 77) and d.out == p.io[f"xattn_map.{f}"].ptr and d.wt == p.io["xattn_wt"].ptr
    assert p.io["xattn_wt"].shape == (1, 77) and all(p.io[f"xattn_map.{f}"].shape == (1, (16 // f) ** 2) for f in want)
    # everything else is the ordinary plan's, where nothing fuses at this size: the same ops in the same order
    assert [n for _, _, n in p.ops if not n.endswith(".attn2.map")] == [n for _, _, n in p0.ops]
    assert p.prog_text_cached is None or p.prog_text_cached.n_ops < p.prog.n_ops


def test_collected_layers_are_not_fused():
    """sdxl at 128 x 128 latents: the ordinary plan runs the cross-attentions of both levels (4096 and 1024 tokens, head dim 64) in the
    epilogue of attn2.to_q; the maps plan keeps q2 of a collected layer in memory and launches its attention"""
    cfg = CONFIGS["sdxl"]()
    from tests.test_host import _FakeWeightsKvAll
    mk = lambda spec: UNetPlan(cfg, _FakeWeightsKvAll(cfg), Arena(1 << 50, None), Arena(1 << 40, None), 2, 128, 128, 77, None, "off", 0x10, attn_maps=spec)
    p0, p = mk(None), mk(AttnMapSpec(4))
    fused0 = sum(1 for o, d, _ in p0.ops if o == lib.OP_GEMM and d.xa_k)
    fused = sum(1 for o, d, _ in p.ops if o == lib.OP_GEMM and d.xa_k)
    maps = sum(1 for o, _, _ in p.ops if o == lib.OP_XATTN_MAP)
    assert fused0 > 0 and fused == 0 and maps == 70
    # a smaller max_factor leaves the other level fused
    p2 = mk({"max_factor": 2})
    assert sum(1 for o, _, _ in p2.ops if o == lib.OP_XATTN_MAP) == 10 and 0 < sum(1 for o, d, _ in p2.ops if o == lib.OP_GEMM and d.xa_k) <= fused0


def test_maps_plan_refusals():
    with pytest.raises(ValueError, match="not divisible"):
        _plan("tiny_sdxl", 18, {"max_factor": 4})
    with pytest.raises(ValueError, match="max_factor"):
        _plan("tiny_sdxl", 16, {"max_factor": 0})
    from sliders_amd.lora_store import LoraStore
    cfg = CONFIGS["tiny_sdxl"]()
    store = LoraStore(cfg, rank=4, alpha=1.0, train_method="noxattn", device="cpu")
    with pytest.raises(ValueError, match="train"):
        _plan("tiny_sdxl", 16, {"max_factor": 4}, "train", store)
    _, p = _plan("tiny_sdxl", 16, {"max_factor": 4}, "on", store)
    assert sum(1 for o, _, _ in p.ops if o == lib.OP_XATTN_MAP) == 17
    assert AttnMapSpec.of(None) is None and AttnMapSpec.of(2) == AttnMapSpec(2) == AttnMapSpec.of({"max_factor": 2})


# ---------------------------------------------------------------------------------------------------------------------------
# host functions
# ---------------------------------------------------------------------------------------------------------------------------
class FakeTokenizer:
    """whitespace words, split into pieces of at most 4 letters; ids index the piece list; BOS / EOS around, truncated to max_len"""

    def __init__(self, max_len=77):
        self.pieces, self.max_len = ["<bos>", "<eos>"], max_len

    def encode(self, text):
        ids = []
        for w in text.lower().split():
            for i in range(0, len(w), 4):
                self.pieces.append(w[i:i + 4])
                ids.append(len(self.pieces) - 1)
        return [0] + ids[:self.max_len - 2] + [1]

    def decode(self, ids):
        return "".join(self.pieces[i] for i in ids)


def test_word_token_indices():
    tok = FakeTokenizer()
    prompt = "a photograph of a woman with red hair and long Hair"
    assert edit.word_token_indices(prompt, "photograph", tok) == [2, 3, 4]          # photo|grap|h
    assert edit.word_token_indices(prompt, "woman", tok) == [7, 8]                  # woma|n
    assert edit.word_token_indices(prompt, "hair", tok) == [11, 14]                 # twice, case-insensitive
    assert edit.word_token_indices(prompt, "a", tok) == [1, 6]
    with pytest.raises(ValueError, match="not a word"):
        edit.word_token_indices(prompt, "beard", tok)
    long = " ".join(["word"] * 80) + " tail"
    with pytest.raises(ValueError):
        edit.word_token_indices(long, "tail", tok)                                  # truncated away
    edge = " ".join(["word"] * 75) + " tail"                                        # "tail" is token 76: the EOS position of a 77-key context
    with pytest.raises(ValueError):
        edit.word_token_indices(edge, "tail", FakeTokenizer(max_len=100))
    assert edit.word_token_indices(" ".join(["word"] * 74) + " tail", "tail", tok) == [75]


def test_word_mask():
    F = torch.zeros(2, 6, 6)
    F[0, 2, 2], F[0, 2, 3], F[0, 4, 4] = 4.0, 1.2, 1.19
    F[1, 1, 1], F[1, 5, 5] = 0.5, 0.15
    m = edit.word_mask(F, threshold=0.3, dilate=0, feather=0.0)
    want = torch.zeros(2, 6, 6)
    want[0, 2, 2] = want[0, 2, 3] = 1.0            # 1.2f / 4.0f >= 0.3f (checked below): at the threshold, in; 1.19 / 4.0 is out
    want[1, 1, 1] = want[1, 5, 5] = 1.0            # each sample by its own maximum: 0.15 / 0.5 = 0.3, at the threshold: in
    assert torch.tensor(1.2) / torch.tensor(4.0) >= torch.tensor(0.3)
    assert torch.equal(m, want)
    assert torch.equal(edit.word_mask(F[0], threshold=0.3, dilate=0, feather=0.0), want[0])
    with pytest.raises(ValueError, match="zero everywhere"):
        edit.word_mask(torch.zeros(1, 4, 4))
    with pytest.raises(ValueError, match="zero everywhere"):
        edit.word_mask(torch.stack([F[0], torch.zeros(6, 6)]))
    with pytest.raises(ValueError):
        edit.word_mask(F, threshold=0.0)
    # the tail is footprint_mask's: the same binary image gives the same mask under the same dilate / feather
    B = (F / F.amax(dim=(1, 2), keepdim=True) >= 0.3).float()
    for dilate, feather in ((1, 1.0), (2, 0.0), (0, 1.5)):
        assert torch.equal(edit.word_mask(F, 0.3, dilate, feather), edit.footprint_mask(B, quantile=1.0, threshold=0.5, dilate=dilate, feather=feather))


def test_level_mean_and_word_map_reference():
    h = w = 4
    m1 = torch.arange(16, dtype=torch.float32).reshape(1, 16)
    m2 = torch.tensor([[1.0, 2.0, 3.0, 4.0]])
    m4 = torch.tensor([[8.0]])
    got = edit.level_mean({4: m4, 1: m1, 2: m2}, h, w)
    up2 = torch.tensor([[1.0, 1, 2, 2], [1, 1, 2, 2], [3, 3, 4, 4], [3, 3, 4, 4]])
    assert torch.equal(got[0], ((m1.reshape(4, 4) + up2) + 8.0) / 3.0)
    with pytest.raises(ValueError):
        edit.level_mean({3: m4}, h, w)

    # a toy collector over a toy space: the maps depend on the latent and the step, so the draws' order and inputs show
    ts = [900, 700, 500, 300, 100]
    x_start = torch.full((1, 4, h, w), 1.0)
    visited = torch.stack([torch.full((1, 4, h, w), float(2 + i)) for i in range(len(ts))])
    sp = edit.NoiseSpace(x0=x_start, x_start=x_start, resid=torch.zeros_like(visited), recon=visited[-1], timesteps=ts, steps=5, skip=0, eta=1.0,
                         guidance=1.0, prediction_type="epsilon", seed=0, visited=visited)
    seen = []

    def collect(xb, t):
        assert xb.dtype == torch.bfloat16
        seen.append((float(xb.float().mean()), t))
        return {1: torch.full((1, 16), float(xb.float().mean())), 2: torch.full((1, 4), t / 100.0)}
    F = edit.word_map_reference(collect, sp, draws=3)
    assert seen == [(1.0, 900), (3.0, 500), (5.0, 100)]           # steps 0, 2, 4 on x_start, visited[1], visited[3]
    assert torch.equal(F, torch.full((1, 4, 4), ((1.0 + 9.0) / 2 + (3.0 + 5.0) / 2 + (5.0 + 1.0) / 2) / 3))
    assert len(edit.footprint_draws(ts, ts[0], 8, 0)) == 5


def test_key_weights():
    w = edit.key_weights(2, 77, tokens=[2, 3])
    assert w.shape == (2, 77) and w.dtype == torch.float32 and float(w.sum()) == 4.0 and bool((w[:, 2:4] == 1).all())
    given = torch.randn(2, 77)
    assert torch.equal(edit.key_weights(2, 77, weights=given), given)
    for bad in (dict(), dict(tokens=[1], weights=given), dict(tokens=[77]), dict(tokens=[]), dict(weights=torch.zeros(2, 76))):
        with pytest.raises(ValueError):
            edit.key_weights(2, 77, **bad)


# ---------------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------------
def _args(tmp_path, extra):
    base = ["--image", str(tmp_path / "x.png"), "--model_path", "m"]
    return edit.build_parser().parse_args(base + extra)


def test_check_args_word_masks(tmp_path):
    mask = tmp_path / "m.png"
    mask.write_bytes(b"x")
    ok = _args(tmp_path, ["--mask_word", "hair", "--mask_word", "beard", "--mask_word_threshold", "0.4", "--mask_word_draws", "4",
                          "--save_attention", "a.png", "--save_mask", "m.png", "--mask_feather", "2", "--mask_invert"])
    edit.check_args(ok)
    assert ok.mask_word == ["hair", "beard"]
    tk = _args(tmp_path, ["--synthetic", "--mask_tokens", "2,3"])
    edit.check_args(tk)
    assert tk.mask_token_list == [2, 3]
    bad = [
        ["--mask_word", "hair", "--mask", str(mask)],
        ["--mask_word", "hair", "--auto_mask", "--lora_weight", "a_alpha1.0_rank4_noxattn.pt"],
        ["--mask_tokens", "2", "--mask", str(mask)],
        ["--mask_tokens", "2", "--auto_mask", "--lora_weight", "a_alpha1.0_rank4_noxattn.pt"],
        ["--mask_tokens", "2", "--mask_word", "hair"],
        ["--synthetic", "--mask_word", "hair"],
        ["--mask_tokens", "2,x"], ["--mask_tokens", "77"], ["--mask_tokens", "-1"],
        ["--mask_word_threshold", "0.4"], ["--mask_word_draws", "4"], ["--save_attention", "a.png"],
        ["--mask_tokens", "2", "--mask_word_threshold", "0"], ["--mask_tokens", "2", "--mask_word_draws", "0"],
    ]
    for extra in bad:
        with pytest.raises(SystemExit):
            edit.check_args(_args(tmp_path, extra))
