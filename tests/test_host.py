"""CPU tests of the host side: YAML schema vs the reference's parse (golden), C-ABI exports vs the header,
static planner invariants on a virtual arena (no GPU memory), checkpoint file interchange."""
import ctypes
import json
import os
import re

import pytest
import torch

from sliders_amd import lib
from sliders_amd.arena import Arena
from sliders_amd.config import CONFIGS
from sliders_amd.config_util import load_config_from_yaml
from sliders_amd.lora_store import LoraStore
from sliders_amd.modules import build_tree
from sliders_amd.planner import BackwardPlan, UNetPlan
from sliders_amd.prompt_util import PromptEmbedsPair, PromptSettings, load_prompts_from_yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def test_yaml_schema_matches_reference_parse():
    gold = json.load(open(os.path.join(G, "schema.json")))
    cfg = load_config_from_yaml(os.path.join(G, "config_sample.yaml"))
    assert json.loads(cfg.model_dump_json()) == gold["config"]
    plain = load_prompts_from_yaml(os.path.join(G, "prompts_sample.yaml"))
    assert [json.loads(p.model_dump_json()) for p in plain] == gold["prompts"]
    attr = load_prompts_from_yaml(os.path.join(G, "prompts_sample.yaml"), ["male", "female"])
    assert [json.loads(p.model_dump_json()) for p in attr] == gold["prompts_attr"]
    # unknown keys (the GPT prompt files' `guidance:`) are ignored -> guidance_scale falls back to 1.0
    assert plain[1].guidance_scale == 1.0 and plain[0].guidance_scale == 4
    with pytest.raises(Exception):
        PromptSettings(positive="x")


def test_prompt_pair_loss_formula():
    st = PromptSettings(target="a", action="enhance", guidance_scale=2.0)
    pair = PromptEmbedsPair(torch.nn.MSELoss(), None, None, None, None, st)
    t, p, u, n = [torch.randn(1, 4, 8, 8) for _ in range(4)]
    got = pair.loss(target_latents=t, positive_latents=p, unconditional_latents=u, neutral_latents=n)
    assert torch.allclose(got, ((t - (n + 2.0 * (p - u))) ** 2).mean())
    pair.action = "erase"
    got = pair.loss(target_latents=t, positive_latents=p, unconditional_latents=u, neutral_latents=n)
    assert torch.allclose(got, ((t - (n - 2.0 * (p - u))) ** 2).mean())


def test_c_abi_exports_exactly_the_declared_symbols():
    """libsliders_hip.so loads without a GPU and exports exactly the entry points include/sliders_hip.h declares."""
    hdr = open(os.path.join(ROOT, "include", "sliders_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(slh_\w+)\s*\(", hdr, flags=re.M))
    assert len(declared) >= 25
    l = lib.load()
    for sym in sorted(declared):
        assert hasattr(l, sym), f"{sym} declared in sliders_hip.h but not exported"
    assert declared == set(lib.EXPORTS)
    assert l.slh_version() >= 2, "2: slh_op_info and slh_memset exist"
    # entry names and descriptor sizes were cross-checked per opcode inside lib.load(); a bad descriptor is rejected with a message
    d = lib.GemmDesc()
    assert l.slh_gemm(ctypes.byref(d), None) != 0
    assert b"slh_gemm" in l.slh_last_error()


def library_ops():
    """opcode -> (entry point, sizeof(descriptor)) as the library's own op table has it (slh_op_info)"""
    l = lib.load()
    n = l.slh_op_info(-1, None, None, None)
    op, entry, size = ctypes.c_int32(-7), ctypes.c_char_p(), ctypes.c_int32(-7)
    assert l.slh_op_info(n, ctypes.byref(op), ctypes.byref(entry), ctypes.byref(size)) == n
    assert (op.value, entry.value, size.value) == (-7, None, -7), "an index out of range writes nothing"
    rows = {}
    for i in range(n):
        assert l.slh_op_info(i, ctypes.byref(op), ctypes.byref(entry), ctypes.byref(size)) == n
        assert op.value not in rows, f"opcode {op.value} listed twice"
        rows[op.value] = (entry.value.decode(), size.value)
    return rows


def test_library_op_table_is_the_bindings():
    rows = library_ops()
    assert len(rows) == 41 and rows == {op: (name, ctypes.sizeof(desc)) for op, (name, desc) in lib._ENTRY.items()}
    assert rows[lib.OP_MEMSET] == ("slh_memset", 24) and lib.OP_MEMSET == 20
    # slh_memset on the host: nothing to fill is a success that launches nothing, through either route; bad descriptors are refused
    lib.call(lib.OP_MEMSET, lib.MemsetDesc(ptr=0, nbytes=0, value=1), 0)
    lib.call(lib.OP_MEMSET, lib.MemsetDesc(ptr=0x1000, nbytes=-5), 0)
    prog = lib.Program()
    prog.memset(0x1000, 0)
    prog.run(0)
    with pytest.raises(lib.SlidersHipError, match="slh_memset: null ptr"):
        lib.call(lib.OP_MEMSET, lib.MemsetDesc(ptr=0, nbytes=16), 0)
    assert lib.load().slh_memset(None, None) != 0 and b"slh_memset" in lib.load().slh_last_error()
    # the executor's own refusals keep their texts and status
    prog = lib.Program()
    prog.add(lib.OP_MEMSET, lib.Gather16Desc(), "wrong descriptor")
    with pytest.raises(lib.SlidersHipError, match=r"rc=-3.*slh_memset descriptor is 32 bytes, library expects 24"):
        prog.run(0)
    prog = lib.Program()
    prog.add(37, lib.MemsetDesc(), "retired opcode")
    with pytest.raises(lib.SlidersHipError, match=r"rc=-3.*unknown opcode 37 at op 0"):
        prog.run(0)
    l, raw = lib.load(), bytes(prog.finalize())
    for cut, what in ((4, b"truncated record header at op 0"), (16, b"truncated record at op 0")):
        assert l.slh_run_program(raw[:cut], cut, None) == -3 and what in l.slh_last_error()


# ---- the binding equals the header -------------------------------------------------------------------------------------------------
_KIND = {lib.c_vp: "pointer", lib.c_i32: "int32_t", lib.c_i64: "int64_t", lib.c_f32: "float", lib.c_f64: "double"}


def _parse_header():
    """include/sliders_hip.h -> (struct -> [(field, kind)], entry point -> descriptor struct, SLH_OP_ name -> value); kind is 'pointer' or
    the scalar's C type.  A declaration this small parser does not understand raises."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sliders_hip.h")).read(), flags=re.S)
    structs = {}
    for name, body in re.findall(r"typedef struct (slh_\w+) \{(.*?)\} \1;", hdr, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"(?:const )?(\w+)(\*?) ([\w, ]+)", decl)
            assert m, f"{name}: cannot parse '{decl}'"
            ctype, star, names = m.groups()
            names = [n.strip() for n in names.split(",")]
            assert (len(names) == 1 and ctype in ("void", "float", "int32_t", "uint32_t", "uint64_t") or ctype.startswith("slh_")) if star \
                else ctype in ("int32_t", "int64_t", "float", "double"), f"{name}: '{decl}'"
            fields += [(n, "pointer" if star else ctype) for n in names]
        structs[name] = fields
    entries = dict(re.findall(r"^int (slh_\w+)\(const (slh_\w+_desc)\* d, slh_stream_t stream\);", hdr, flags=re.M))
    ops = {n: int(v) for n, v in re.findall(r"\bSLH_OP_(\w+) = (\d+)", hdr)}
    return structs, entries, ops


def _binding_ops(module=lib):
    return {n[3:]: v for n, v in vars(module).items() if n.startswith("OP_") and isinstance(v, int)}


def _abi_mismatches(header, entry_table, ops):
    """every disagreement between the parsed header and a binding's (opcode -> (entry, ctypes struct), OP_ name -> value), as text"""
    structs, entries, hdr_ops = header
    out = [f"SLH_OP_{n}: header {hdr_ops.get(n)}, binding {ops.get(n)}" for n in sorted(set(hdr_ops) | set(ops)) if hdr_ops.get(n) != ops.get(n)]
    out += [f"opcode {op} has no OP_ constant" for op in entry_table if op not in ops.values()]
    for op, (entry, desc) in sorted(entry_table.items()):
        if entry not in entries:
            out.append(f"opcode {op}: {entry} is not declared as int {entry}(const slh_*_desc* d, slh_stream_t stream)")
            continue
        out += _struct_mismatches(structs[entries[entry]], desc, f"opcode {op} {entry}: {entries[entry]} / {desc.__name__}")
    return out


def _struct_mismatches(fields, ctype, what):
    mine = [(n, _KIND[t]) for n, t in ctype._fields_]
    if mine == fields:
        return []
    at = next((i for i, (a, b) in enumerate(zip(fields, mine)) if a != b), min(len(fields), len(mine)))
    return [f"{what}: field {at}: header {fields[at] if at < len(fields) else None}, binding {mine[at] if at < len(mine) else None}"]


def test_binding_equals_header():
    """Every SLH_OP_* value, and every field of every descriptor by name, order and kind (pointer / int32_t / int64_t / float / double),
    is the same in include/sliders_hip.h and in sliders_amd/lib.py - what the load-time check (entry name and sizeof per opcode)
    cannot see: two same-sized fields swapped load cleanly and compute garbage."""
    header = _parse_header()
    structs, entries, hdr_ops = header
    assert len(structs) >= 36 and len(hdr_ops) == 41 and len(set(hdr_ops.values())) == 41
    assert set(hdr_ops.values()) == set(lib._ENTRY), "every opcode of the header has a row of lib._ENTRY and the other way round"
    assert _abi_mismatches(header, lib._ENTRY, _binding_ops()) == []
    assert {entries[e] for e, _ in lib._ENTRY.values()} | {"slh_lora_merge_item", "slh_lora_lnfold_item"} == set(structs), \
        "a struct of the header that no check above looked at"
    assert _struct_mismatches(structs["slh_lora_merge_item"], lib.LoraMergeItem, "slh_lora_merge_item") == []
    # slh_lora_lnfold_item has no ctypes struct: lib.lnfold_item writes it as int64 words
    item = structs["slh_lora_lnfold_item"]
    assert [k for _, k in item] == ["pointer"] * 6 + ["int32_t"] * 2 and [n for n, _ in item[6:]] == ["rows", "K"]
    assert 8 * lib.LORA_LNFOLD_ITEM_I64 == 6 * 8 + 2 * 4
    # the comparison can fail: two same-kind neighbours swapped in one struct, one opcode value changed
    f = list(lib.AttnDesc._fields_)
    i = [n for n, _ in f].index("ldq")
    assert f[i + 1][0] == "ldk" and f[i][1] is f[i + 1][1]
    f[i], f[i + 1] = f[i + 1], f[i]
    swapped = type("AttnDesc", (ctypes.Structure,), {"_fields_": f})
    assert ctypes.sizeof(swapped) == ctypes.sizeof(lib.AttnDesc), "the load-time check would pass this one"
    got = _abi_mismatches(header, {**lib._ENTRY, lib.OP_ATTN_FWD: ("slh_attn_fwd", swapped)}, _binding_ops())
    assert len(got) == 1 and "slh_attn_fwd" in got[0] and "('ldq', 'int32_t')" in got[0] and "('ldk', 'int32_t')" in got[0], got
    got = _abi_mismatches(header, lib._ENTRY, {**_binding_ops(), "LION": 30})
    assert got == ["SLH_OP_LION: header 31, binding 30", "opcode 31 has no OP_ constant"], got


class _FakeWeights:
    def __init__(self, cfg):
        self.temb_offsets, self.resnet_paths, off = {}, [], 0
        for n, m in build_tree(cfg).named_modules():
            if m.cls == "ResnetBlock2D":
                self.resnet_paths.append(n)
                self.temb_offsets[n] = off
                off += m.out_dim
        self.temb_total = off
        self.packed = True
        self.kv_all_offset = {}
        self.kv_all_vbase = 0
        self.gemm_shape = {}
        self.ln_fold = True
        self.geglu16 = True          # WeightStore's default: GEGLU.proj also in the 16 | 16 block order

    def ptr(self, name):
        # a distinct, 256-byte aligned fake address per tensor name (the planner's weight-touch pass matches launches by pointer)
        if not hasattr(self, "_ids"):
            self._ids = {}
        return 0x10000000 + 0x100 * self._ids.setdefault(name, len(self._ids) + 1)

    def has(self, name):
        return True


@pytest.mark.parametrize("name,hw,method", [("tiny_sdxl", 16, "noxattn"), ("tiny_sd1", 16, "full"), ("sdxl", 128, "noxattn")])
def test_planner_static_invariants(name, hw, method):
    cfg = CONFIGS[name]()
    store = LoraStore(cfg, train_method=method, init="none")
    store.temb_tcol = torch.zeros(1, dtype=torch.int32)
    counts = {}
    for mode in ("off", "on", "train"):
        va, vz = Arena(1 << 50, None), Arena(1 << 40, None)
        p = UNetPlan(cfg, _FakeWeights(cfg), va, vz, 2, hw, hw, 77, store if mode != "off" else None, mode, 0x10)
        ops = list(p.prog.ops)
        counts[mode] = len(ops)
        # every allocation is 256-byte aligned and allocations never overlap
        spans = sorted((s, e) for s, e, _ in va.allocs)
        assert all(s % 256 == 0 for s, _ in spans)
        assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))
        gemms = [d for o, d in ops if o == lib.OP_GEMM]
        assert all(d.K % 64 == 0 and d.N % 4 == 0 and d.ldc % 4 == 0 for d in gemms)
        assert all(d.w_layout == 1 for d in gemms), "frozen weights are streamed tile-packed"
        if mode == "off":
            assert not any(d.lora_t or d.lora_down for d in gemms), "adapters off must not launch any LoRA work"
            assert not any(o == lib.OP_SKINNY for o, d in ops[:-1])
        else:
            n_lora = sum(1 for d in gemms if d.lora_t or d.lora_down)
            assert n_lora > 0
        if mode == "train":
            bw = BackwardPlan(p, 1, 1, 0x20)
            assert len(bw.prog.ops) > len(ops)
            dg = [d for o, d in bw.prog.ops if o == lib.OP_GEMM]
            assert all(d.M == d_.M for d, d_ in zip(dg[:1], dg[:1]))
            assert all(d.K % 64 == 0 for d in dg)
            # the GEGLU backward rides in the backward-data product of the Linear behind it (geglu = 2) ...
            n_geglu = sum(1 for d in gemms if d.geglu == 1)
            assert n_geglu > 0 and all(d.geglu_pre for d in gemms if d.geglu == 1)
            assert sum(1 for d in dg if d.geglu == 2) == n_geglu and all(d.geglu_pre and d.ldc >= 2 * d.N for d in dg if d.geglu == 2)
            assert not any(o == lib.OP_ELEMENTWISE and d.op == lib.EW_GEGLU_BWD for o, d in bw.prog.ops)
            # ... and dO^T of a self-attention with 64-wide heads comes out of the product that makes dO (both layouts)
            n_dot = sum(1 for d in dg if d.vt_out)
            assert all(d.vt_also_c == 1 and d.vt_col0 == 0 for d in dg if d.vt_out)
            if name == "sdxl":
                n_self = sum(1 for n in p.prog.op_names if n.endswith("attn1.sdpa"))
                assert n_dot == n_self and not any(n.endswith(".dot") for n in bw.prog.op_names)
    assert counts["off"] <= counts["on"] <= counts["train"]
    if name == "sdxl":
        assert counts["off"] < 1300     # one launch per fused op: ~1.15k for the whole SDXL UNet


def test_tile_64x160_entries_and_fallback():
    """The tuned table's entries for the 64 x 160 tile (csrc/gemm5.hip): every launch of the SDXL 1024^2 plans that is given that tile is
    one the tile can run (slh_gemm5_ok, the library's own rule, also what tuning.tile_ok asks), its LayerNorm producers leave
    80-column chunks and their consumers are told so; a launch of the same SHAPE that needs more than the tile's epilogue offers
    falls back to the 128 x 128 ring tile, not to the untuned heuristic."""
    from sliders_amd.tuning import tile_ok, tuned_tile
    cfg = CONFIGS["sdxl"]()
    store = LoraStore(cfg, train_method="noxattn", init="none")
    store.temb_tcol = torch.zeros(1, dtype=torch.int32)
    seen = 0
    for mode, B in (("on", 2), ("train", 2), ("off", 3)):
        va, vz = Arena(1 << 50, None), Arena(1 << 40, None)
        p = UNetPlan(cfg, _FakeWeights(cfg), va, vz, B, 128, 128, 77, store if mode != "off" else None, mode, 0x10)
        gemms = [d for o, d in p.prog.ops if o == lib.OP_GEMM]
        g5 = [d for d in gemms if (d.tile >> 12) & 15 == 5]
        assert all(lib.gemm5_ok(d) and tile_ok(d, d.tile) for d in g5)
        assert all(d.M % 64 == 0 and d.N % 160 == 0 and not d.ln_in for d in g5)      # (round 6: one entry carries a fused adapter, which the tile supports)
        if mode == "off":
            assert not g5                      # M = 3072: 1.5 rounds of 64 x 160 tiles, measured slower - no entries
            continue
        assert len(g5) >= 120 and {d.tile for d in g5} == {0x5425, 0x5525}      # (the 8192 x 640 products moved on to the 128 x 160 four-wave tile in round 6)
        seen += len(g5)
        # chunk statistics: producers on the tile leave N / 80 chunks, and whoever folds that LayerNorm merges N / 80 chunks of it
        # (the four-wave tile of gemm7.hip whose waves own 80 columns - 0x7645 - leaves 80-column chunks as well)
        g7 = [d for d in gemms if (d.tile >> 12) & 15 == 7]
        assert all(lib.gemm7_ok(d) for d in g7)
        prod = {d.ln_out: d.N // 80 for d in g5 + [d for d in g7 if (d.tile & 15) % 5 == 0] if d.ln_out}
        cons = [d for d in gemms if d.ln_in in prod]
        assert prod and cons and all(d.ln_in_chunks == prod[d.ln_in] and d.K == 80 * d.ln_in_chunks for d in cons)
        assert all(d.ln_in_chunks * 64 == d.K for d in gemms if d.ln_in and d.ln_in not in prod)
    assert seen
    # same key, a feature the tile has no epilogue for (a per-sample row bias): the ring tile it replaced runs
    d = lib.GemmDesc(a0=0x1000, w=0x2000, c=0x3000, lda0=1280, ca0=1280, mode=0, stride=1, ldw=0, M=2048, N=1280, K=1280, ldc=1280,
                     rows_per_sample=1024, w_layout=1)
    assert tuned_tile(d) == 0x5425
    d.rowbias, d.ld_rowbias = 0x4000, 1280
    assert not lib.gemm5_ok(d) and tuned_tile(d) == 0x4412


@pytest.mark.parametrize("train_method", ["noxattn", "xattn", "xattn-strict", "selfattn", "full"])
@pytest.mark.parametrize("nb", [1, 2])
def test_every_recorded_tile_can_run_its_launch(train_method, nb):
    """Every GEMM a plan records - no-grad, training forward AND backward, every train_method of lora.py:126-147, one or two samples
    carrying a gradient (prompt batch_size 1 / 2) - names a tile the library accepts for that launch, as recorded: slh_gemm's whole
    check, workspaces included (a table entry for the 64 x 160 tile once landed on 70 attn1.out dgrads at nb = 2 that
    carried a dO^T store, which that tile has no epilogue for)."""
    from sliders_amd.tuning import tile_ok
    cfg = CONFIGS["sdxl"]()
    store = LoraStore(cfg, train_method=train_method, init="none")
    store.temb_tcol = torch.zeros(1, dtype=torch.int32)
    B = 2 * nb
    n5 = 0
    for mode in ("on", "train"):
        va, vz = Arena(1 << 50, None), Arena(1 << 40, None)
        p = UNetPlan(cfg, _FakeWeights(cfg), va, vz, B, 128, 128, 77, store, mode, 0x10)
        progs = [p.prog]
        if mode == "train":
            progs.append(BackwardPlan(p, nb, nb, 0x20).prog)
        for prog in progs:
            for (o, d), nm in zip(prog.ops, prog.op_names):
                if o != lib.OP_GEMM:
                    continue
                if (d.tile >> 12) & 15 == 5:
                    n5 += 1
                    assert lib.gemm5_ok(d), f"{nm}: tile {d.tile:#x} cannot run this launch"
                assert not d.tile or tile_ok(d, d.tile), f"{nm}: tile {d.tile:#x}"
                try:            # slh_gemm's whole check, workspaces included, on every tile family
                    lib.gemm_kernel_name(d)
                except lib.SlidersHipError as e:
                    raise AssertionError(f"{nm}: tile {d.tile:#x} cannot run this launch") from e
    assert n5 > 0


def test_geglu_backward_is_refused_on_the_narrow_ping_pong_tiles():
    """geglu = 2 (the GEGLU backward in the epilogue) is compiled out of the 128 x 64*NI ping-pong tiles: the library refuses the launch
    instead of running it without the epilogue - the query and the dispatch alike."""
    d = lib.GemmDesc(a0=0x1000, w=0x2000, c=0x3000, lda0=1280, ca0=1280, mode=0, stride=1, ldw=0, M=1024, N=5120, K=1280, ldc=10240,
                     rows_per_sample=1024, w_layout=1, geglu=2, geglu_pre=0x4000, ld_pre=10240)
    for tile in (0x4412, 0x4011, 0x8042):
        d.tile = tile
        assert lib.gemm_tile_ok(d) and lib.gemm_kernel_name(d), hex(tile)
    for tile in (0x8013, 0x8014, 0x8015):
        d.tile = tile
        assert not lib.gemm_tile_ok(d), hex(tile)
        with pytest.raises(lib.SlidersHipError, match="geglu = 2"):
            lib.gemm_kernel_name(d)


def test_tile_and_its_extras_are_chosen_together(monkeypatch):
    """A table entry for the 64 x 160 tile on a product that wants both LayerNorm chunk statistics (ln_stats) and the V^T store
    (vt_heads): the tile is settled before anything is sized from it, so the recorded launch is one the library runs and its chunk
    buffer has the chunk count of the tile that runs."""
    from sliders_amd import tuning
    cfg = CONFIGS["tiny_sdxl"]()
    p = UNetPlan(cfg, _FakeWeights(cfg), Arena(1 << 50, None), Arena(1 << 40, None), 1, 16, 16, 77, None, "off", 0x10)
    N, K = 1920, 640
    x = p.act(1, 32, 32, K, "x")
    monkeypatch.setitem(tuning.table(), f"{x.M},{N},{K},m0,s1,x0,g0,l0,no", 0x5425)
    out = p.gemm(x, "probe", N, "probe", bias=False, vt_heads=10, ln_stats=True)
    o, d, _ = p.ops[-1]                        # (recorded behind the finished plan: not part of p.prog, which was serialised once)
    assert o == lib.OP_GEMM and d.tile == 0x5425
    lib.gemm_kernel_name(d)
    assert out.ln is not None and d.ln_out == out.ln[0].ptr
    assert out.ln[1] == N // lib.gemm_ln_chunk_cols(d) == N // 80
    assert out.ln[0].shape == (N // 80, x.M, 2)


@pytest.mark.parametrize("name,hw", [("sdxl", 128), ("sd2", 64), ("sd1", 64)])
def test_planner_fusions_of_the_no_grad_pass(name, hw):
    """Launch-count invariants of the adapters-on no-grad pass (the one the denoise loop replays): with 64-wide heads
    (SDXL, SD-2.x) every self-attention reads the V third of its fused q|k|v projection head-transposed straight from that
    GEMM's epilogue (vt_out) - no transpose launch per block; SD-1.x (40/80/160-wide heads, zero-padded d-tiles) keeps the
    transpose kernel.  With the batched text K/V path the plan also carries the program the loop replays from step 2 on."""
    from sliders_amd.weights import WeightStore   # noqa: F401  (kv_all path needs the real offsets only on the GPU plan)
    cfg = CONFIGS[name]()
    store = LoraStore(cfg, train_method="noxattn", init="none")
    store.temb_tcol = torch.zeros(1, dtype=torch.int32)
    va, vz = Arena(1 << 50, None), Arena(1 << 40, None)
    p = UNetPlan(cfg, _FakeWeights(cfg), va, vz, 2, hw, hw, 77, store, "on", 0x10)
    ops = list(p.prog.ops)
    names = list(p.prog.op_names)
    # weights of the big products (GEGLU.proj, ff.net.2, q|k|v of the 1280-channel level) are touched from the idle workgroup slots of
    # an earlier 160-tile launch (slh_gemm_desc.pf_*): every touch rides AHEAD of the product that streams those bytes, at most
    # TOUCH_WINDOW ops ahead
    from sliders_amd.planner import TOUCH_WINDOW
    wpos = {}
    for i, (o, d) in enumerate(ops):
        if o == lib.OP_GEMM:
            wpos.setdefault(d.w, i)
    touches = [(i, d) for i, (o, d) in enumerate(ops) if o in (lib.OP_GEMM, lib.OP_ATTN_FWD) and d.pf_ptr]
    if name == "sdxl":
        # (round 5: attn2.to_out / proj_out / ff.net.2 of the 1280-channel level run on the 64 x 160 tile - 256 workgroups, no idle slots;
        # round 6: attn1.to_out as well, its touch rides on the key-split self-attention launch in front of it (slh_attn_desc.pf_*) - so a
        # block has two carriers, attn1.sdpa and attn2.to_q, for its three big matrices: GEGLU.proj and ff.net.2 are touched, the next
        # block's q|k|v is not; measured with this assignment)
        assert len(touches) >= 120
        assert sum(1 for i, d in touches if ops[i][0] == lib.OP_ATTN_FWD) >= 55
    assert all(d.pf_bytes >= 6 << 20 and (ops[i][0] == lib.OP_ATTN_FWD and lib.attn_carries_touch(d) or (d.tile & 0xFFFFFF) == 0x4412)
               for i, d in touches)
    for j, dj in touches:       # the bytes a launch touches are the packed weights of a product at most TOUCH_WINDOW ops LATER
        later = [d for o, d in ops[j + 1:j + 1 + TOUCH_WINDOW] if o == lib.OP_GEMM and d.w == dj.pf_ptr]
        assert later and dj.pf_bytes == (later[0].N + 63) // 64 * 64 * later[0].K * 2, (j, hex(dj.pf_ptr))
    assert len({d.pf_ptr for _, d in touches}) == len(touches), "no matrix is touched twice in a pass"
    n_self = sum(1 for n in p.prog.op_names if n.endswith("attn1.sdpa"))
    n_tr = sum(1 for o, _ in ops if o == lib.OP_TRANSPOSE_HEADS)
    n_vt = sum(1 for o, d in ops if o == lib.OP_GEMM and d.vt_out)
    assert n_self > 0
    if name in ("sdxl", "sd2"):
        assert n_vt == n_self and all(d.vt_D == 64 and d.vt_col0 == 2 * d.N // 3 for o, d in ops if o == lib.OP_GEMM and d.vt_out)
        assert n_tr <= n_self          # what is left are the cross-attention V transposes (one per block here: fake weights have no batched K/V)
    else:
        assert n_vt == 0 and n_tr >= n_self
    # train-mode plans keep V row-major for the attention backward: the transposed copy comes on top (vt_also_c), and the
    # GEGLU product keeps its pre-activation (geglu_pre) instead of a separate elementwise launch
    pt = UNetPlan(cfg, _FakeWeights(cfg), Arena(1 << 50, None), Arena(1 << 40, None), 2, hw, hw, 77, store, "train", 0x10)
    assert all(d.vt_also_c == 1 for o, d in pt.prog.ops if o == lib.OP_GEMM and d.vt_out)
    assert sum(1 for o, d in pt.prog.ops if o == lib.OP_GEMM and d.vt_out) == (n_self if name in ("sdxl", "sd2") else 0)
    assert all(d.geglu_pre for o, d in pt.prog.ops if o == lib.OP_GEMM and d.geglu)
    assert sum(1 for o, d in pt.prog.ops if o == lib.OP_GEMM and d.geglu) == n_self
    if p.prog_text_cached is not None:
        assert p.prog_text_cached.n_ops == p.prog.n_ops - 2 - sum(1 for o, _ in ops if o == lib.OP_LORA_LN_FOLD)      # (+ their touches)
    # round 4: GEGLU.proj in the 16 | 16 block order in the no-grad passes (any tile), the 32 | 32 order with geglu_pre in training
    assert all(d.geglu == 3 for o, d in ops if o == lib.OP_GEMM and d.geglu)
    assert all(d.geglu == 1 for o, d in pt.prog.ops if o == lib.OP_GEMM and d.geglu)
    n_fold = sum(1 for o, d in ops if o == lib.OP_GEMM and d.ln_in and d.lora_down)
    n_head = sum(1 for o, _ in ops if o == lib.OP_LORA_LN_FOLD)
    if name == "sdxl":
        # norm1 folded into the adapter-carrying q|k|v of the 1280-channel level (60 blocks; its tuned tile is the 128 x 256
        # ping-pong tile): one slh_lora_ln_fold launch at the head of the program rebuilds A . gamma for all of them, and only the
        # 640-channel level keeps its LayerNorm launches
        assert n_fold == 60 and n_head == 1 and ops[1][0] == lib.OP_LORA_LN_FOLD and ops[1][1].n == 60
        assert all(d.ln_lora_s and d.ln_lora_c and (d.tile >> 12) & 15 == 8 and d.vt_out for o, d in ops if o == lib.OP_GEMM and d.ln_in and d.lora_down)
        assert sum(1 for o, _ in ops if o == lib.OP_LAYERNORM) == 10           # of 210 LayerNorms: norm1 of the ten 640-channel blocks
    else:
        assert n_fold == 0 and n_head == 0
    assert not any(d.ln_in and d.lora_down for o, d in pt.prog.ops if o == lib.OP_GEMM), "training passes keep the LayerNorm launch"


def test_checkpoint_file_is_reference_loadable(tmp_path):
    """save_weights writes a torch .pt OrderedDict with the reference's keys; it strict-loads into the oracle
    restatement of the reference's LoRANetwork (the notebooks' `network.load_state_dict(torch.load(path))`)."""
    from oracle.lora_oracle import LoRANetworkOracle
    from oracle.unet_oracle import build_unet
    cfg = CONFIGS["tiny_sdxl"]()
    s = LoraStore(cfg, train_method="noxattn")
    path = tmp_path / "slider_alpha1.0_rank4_noxattn_last.pt"
    torch.save(s.state_dict(torch.bfloat16), path)
    sd = torch.load(path)
    assert all(v.dtype == torch.bfloat16 for v in sd.values())
    net = build_unet("tiny_sdxl", seed=0)
    nw = LoRANetworkOracle(net, rank=4, multiplier=1.0, alpha=1.0, train_method="noxattn")
    nw.load_state_dict(sd, strict=True)
    assert list(nw.state_dict().keys()) == list(sd.keys())


def test_gemm_weight_tile_packing_layout():
    """pack_gemm_w must produce exactly the order include/sliders_hip.h documents for w_layout = 1 (the kernel
    addresses it with plain pointer arithmetic), and unpack_gemm_w must invert it."""
    import torch
    from sliders_amd.weights import pack_gemm_w, unpack_gemm_w
    n, k = 200, 320
    w = torch.arange(n * k, dtype=torch.float32).reshape(n, k)
    flat = pack_gemm_w(w)
    npad = 256
    assert flat.numel() == npad * k
    g = torch.Generator().manual_seed(0)
    for _ in range(200):
        r = int(torch.randint(0, npad, (1,), generator=g))
        c = int(torch.randint(0, k, (1,), generator=g))
        rr, slot, e = r & 63, (c & 63) >> 3, c & 7
        off = ((r >> 6) * (k // 64) + (c >> 6)) * 4096 + rr * 64 + ((slot ^ ((rr >> 1) & 7)) << 3) + e
        assert flat[off].item() == (w[r, c].item() if r < n else 0.0)
    assert torch.equal(unpack_gemm_w(flat, n, k), w)


def test_c_abi_rejects_bad_descriptors_before_any_launch():
    """Argument validation runs before the first HIP call, so it is testable without a GPU: every unsupported shape,
    alignment or flag combination returns non-zero and names the entry point (no silent fallback, no launch)."""
    one = 0x1000          # any non-null pointer: validation never dereferences device memory

    def gemm(**kw):
        base = dict(a0=one, w=one, c=one, lda0=64, ca0=64, mode=0, stride=1, ldw=64, M=64, N=64, K=64, ldc=64,
                    rows_per_sample=64)
        base.update(kw)
        return lib.GemmDesc(**base)

    bad = {
        "K multiple of 64": gemm(K=96, ca0=96, lda0=96, ldw=96),
        "N multiple of 4": gemm(N=66),
        "dense K": gemm(ca0=128, lda0=128),                            # K != ca0 + ca1
        "a1/ca1": gemm(ca1=64, K=128),                                 # second source declared but a1 null
        "bad tile": gemm(tile=0x33),
        "8-wave": gemm(tile=0x4021),
        "bad mode": gemm(mode=2),
        "conv K": gemm(mode=1, batch=1, hs=8, ws=8, ho=8, wo=8, K=64 * 8),
        "geglu": gemm(geglu=1, residual=one, ld_res=64),
        "fused lora": gemm(lora_down=one, lora_up=one, lora_scale=one, lora_groups=1, lora_rank=8, ld_t=4),
        "w_layout": gemm(w_layout=3),
    }
    for what, d in bad.items():
        with pytest.raises(lib.SlidersHipError, match="slh_gemm"):
            lib.call(lib.OP_GEMM, d, 0)
    with pytest.raises(lib.SlidersHipError, match="slh_layernorm"):
        lib.call(lib.OP_LAYERNORM, lib.LnDesc(x=one, y=one, gamma=one, beta=one, M=4, C=2048, ldx=2048, ldy=2048), 0)
    with pytest.raises(lib.SlidersHipError, match="slh_attn"):
        lib.call(lib.OP_ATTN_FWD, lib.AttnDesc(q=one, k=one, vt=one, o=one, B=1, H=1, Tq=64, Tk=64, ldq=64, ldk=64,
                                               ldvt=64, ldo=64, scale=1.0, D=200), 0)
    # a malformed command buffer is refused as a whole
    buf = ctypes.create_string_buffer(b"\x63\x00\x00\x00\x08\x00\x00\x00" + b"\0" * 8, 16)
    assert lib.load().slh_run_program(ctypes.cast(buf, ctypes.c_void_p), 16, None) != 0
    assert b"slh_run_program" in lib.load().slh_last_error()


def test_diffusers_directory_loader_and_weight_packing(tmp_path):
    """model_util.load_unet_state reads the layout the reference loads through diffusers (model_util.py:67-72,
    169-174: <dir>/unet/config.json + diffusion_pytorch_model.safetensors), and WeightStore repacks every matrix the
    GEMM streams losslessly (the tile-packed form unpacks to the fused / permuted source rows)."""
    from safetensors.torch import save_file
    from oracle.unet_oracle import build_unet
    from sliders_amd.model_util import load_unet_state
    from sliders_amd.weights import WeightStore

    net = build_unet("tiny_sdxl", seed=3)
    sd = {k: v.contiguous() for k, v in net.state_dict().items()}
    cfg0 = CONFIGS["tiny_sdxl"]()
    unet_dir = tmp_path / "model" / "unet"
    unet_dir.mkdir(parents=True)
    raw = {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg0.__dict__.items()}
    raw.update({"_class_name": "UNet2DConditionModel", "_diffusers_version": "0.20.2", "act_fn": "silu"})   # extra keys ignored
    (unet_dir / "config.json").write_text(json.dumps(raw))
    save_file(sd, str(unet_dir / "diffusion_pytorch_model.safetensors"))
    cfg, loaded = load_unet_state(str(tmp_path / "model"))
    assert cfg == cfg0
    assert loaded.keys() == sd.keys() and all(torch.equal(loaded[k], sd[k]) for k in sd)

    ws = WeightStore(cfg, loaded, "cpu", dtype=torch.float32)
    p = "down_blocks.1.attentions.0.transformer_blocks.0"
    qkv = torch.cat([sd[f"{p}.attn1.to_{x}.weight"] for x in "qkv"], 0)
    assert torch.equal(ws.gemm_matrix(f"{p}.attn1.qkv.w"), qkv)
    conv = sd["down_blocks.0.resnets.0.conv1.weight"]
    assert torch.equal(ws.gemm_matrix("down_blocks.0.resnets.0.conv1.w"), conv.permute(0, 2, 3, 1).reshape(conv.shape[0], -1))
    # batched text K/V: [all K rows | all V rows], each block's slice at the recorded offsets
    k_off, v_off = ws.kv_all_offset[f"{p}.attn2"]
    allkv = ws.gemm_matrix("attn2_kv_all.w")
    wk, wv = sd[f"{p}.attn2.to_k.weight"], sd[f"{p}.attn2.to_v.weight"]
    assert torch.equal(allkv[k_off:k_off + wk.shape[0]], wk) and torch.equal(allkv[v_off:v_off + wv.shape[0]], wv)
    assert allkv.shape[0] == 2 * ws.kv_all_vbase
    with pytest.raises(FileNotFoundError):
        load_unet_state(str(tmp_path / "nope"))


def test_cli_keeps_the_reference_flags():
    """train_lora.py / train_lora_xl.py flags (train_lora_xl.py:419-470) parse unchanged."""
    from sliders_amd.cli import build_parser
    a = build_parser(True).parse_args(["--config_file", "c.yaml", "--prompts_file", "p.yaml", "--alpha", "1.0", "--rank", "4",
                                       "--device", "0", "--name", "ageslider", "--attributes", "male, female"])
    got = (a.config_file, a.prompts_file, a.alpha, a.rank, a.device, a.name, a.attributes)
    assert got == ("c.yaml", "p.yaml", 1.0, 4, 0, "ageslider", "male, female")


def test_encode_prompts_xl_contract_with_tiny_clip():
    """train_util.py:77-133: per prompt the penultimate hidden states of both CLIP text encoders concatenated on the
    feature axis, and the pooled (projected) output of the SECOND encoder.  Tiny random-init CLIP models and a stub
    tokenizer stand in for the checkpoints the build image does not have."""
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
    from sliders_amd.model_util import encode_prompts_xl

    class Tok:
        model_max_length = 77

        def __call__(self, prompts, padding, max_length, truncation, return_tensors):
            g = torch.Generator().manual_seed(len(prompts))
            ids = torch.randint(1, 90, (len(prompts), max_length), generator=g)
            ids[:, -1] = 99                      # eos = highest id: CLIP pools at argmax(input_ids)
            return type("Enc", (), {"input_ids": ids})()

    torch.manual_seed(0)
    c1 = CLIPTextConfig(vocab_size=100, hidden_size=32, intermediate_size=64, num_hidden_layers=3, num_attention_heads=2,
                        max_position_embeddings=77, eos_token_id=99)
    c2 = CLIPTextConfig(vocab_size=100, hidden_size=48, intermediate_size=64, num_hidden_layers=3, num_attention_heads=2,
                        max_position_embeddings=77, projection_dim=40, eos_token_id=99)
    e1, e2 = CLIPTextModel(c1).eval(), CLIPTextModelWithProjection(c2).eval()
    prompts = ["a person", "an old person"]
    text, pooled = encode_prompts_xl([Tok(), Tok()], [e1, e2], prompts, num_images_per_prompt=2)
    assert text.shape == (4, 77, 32 + 48) and pooled.shape == (4, 40)
    ids = Tok()(prompts, "max_length", 77, True, "pt").input_ids
    with torch.no_grad():
        h1 = e1(ids, output_hidden_states=True).hidden_states[-2]
        o2 = e2(ids, output_hidden_states=True)
    want = torch.cat([h1, o2.hidden_states[-2]], -1).repeat_interleave(2, dim=0)
    assert torch.allclose(text, want) and torch.allclose(pooled, o2.text_embeds.repeat_interleave(2, dim=0))


def test_build_pairs_caches_prompts_and_concatenates_like_the_reference():
    """cli.build_pairs: one encoder call per distinct prompt (PromptEmbedsCache, train_lora_xl.py:121-151) and ctx =
    cat([unconditional, X]).repeat_interleave(batch_size) (concat_embeddings, train_util.py:136-141)."""
    from sliders_amd.cli import build_pairs
    cfg = CONFIGS["tiny_sdxl"]()
    calls = []

    def encode(text):
        calls.append(text)
        g = torch.Generator().manual_seed(len(text))
        return torch.randn(1, 77, cfg.cross_attention_dim, generator=g), torch.randn(1, cfg.pooled_dim, generator=g)

    prompts = [PromptSettings(target="person", positive="old person", unconditional="young person", neutral="person",
                              action="enhance", guidance_scale=4, batch_size=2),
               PromptSettings(target="person", positive="smiling person", unconditional="", neutral="person",
                              action="erase", guidance_scale=2, batch_size=1)]
    pairs = build_pairs(cfg, prompts, encode, "cpu")
    assert sorted(calls) == sorted({"person", "old person", "young person", "smiling person", ""})
    (s0, p0), (s1, p1) = pairs
    assert p0.ctx_target.shape == (4, 77, cfg.cross_attention_dim) and p0.pooled_positive.shape == (4, cfg.pooled_dim)
    assert p1.ctx_target.shape == (2, 77, cfg.cross_attention_dim)
    unc, tgt = encode("young person")[0].bfloat16(), encode("person")[0].bfloat16()
    assert torch.equal(p0.ctx_target, torch.cat([unc, tgt]).repeat_interleave(2, dim=0))
    assert torch.equal(p0.ctx_uncond, torch.cat([unc, unc]).repeat_interleave(2, dim=0))
    assert (p0.guidance_scale, p0.action, p1.guidance_scale, p1.action) == (4, "enhance", 2, "erase")
    assert p0.ctx_target.dtype == torch.bfloat16


# ---- config surface: honoured or rejected, never silently ignored (train_lora_xl.py:92-107, 170-203, 394-410) ----
def _cfg(**train):
    from sliders_amd import config_util
    base = dict(prompts_file="p.yaml", pretrained_model=dict(name_or_path="x"), network=dict(type="c3lier", rank=8, alpha=2.0,
                                                                                           training_method="noxattn"),
                train=dict(precision="bfloat16", noise_scheduler="ddim", iterations=1000, lr=2e-4, optimizer="AdamW",
                           lr_scheduler="constant", max_denoising_steps=50),
                save=dict(name="s", path="./models", per_steps=500, precision="bfloat16"),
                logging=dict(use_wandb=False, verbose=False), other=dict(use_xformers=True))
    base["train"].update(train)
    return config_util.RootConfig(**base)


def test_cli_rank_and_alpha_override_only_when_given():
    from sliders_amd.cli import apply_cli_overrides, build_parser
    a = build_parser(True).parse_args(["--config_file", "c.yaml"])
    assert a.rank is None and a.alpha is None
    c = apply_cli_overrides(_cfg(), a)
    assert c.network.rank == 8 and c.network.alpha == 2.0                 # the YAML's values survive
    assert c.save.name == "s_alpha2.0_rank8_noxattn" and c.save.path == "./models/s_alpha2.0_rank8_noxattn"
    a = build_parser(True).parse_args(["--config_file", "c.yaml", "--rank", "4", "--alpha", "1", "--name", "age"])
    c = apply_cli_overrides(_cfg(), a)
    assert c.network.rank == 4 and c.network.alpha == 1.0 and c.save.name == "age_alpha1.0_rank4_noxattn"


def test_optimizer_options_and_rejections():
    from sliders_amd.cli import check_supported, optimizer_options
    assert optimizer_options(_cfg().train) == {"betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.01, "name": "adamw"}
    o = optimizer_options(_cfg(optimizer="adamw", optimizer_args="weight_decay=0.1 betas=(0.8,0.99) eps=1e-6").train)
    assert o == {"betas": (0.8, 0.99), "eps": 1e-6, "weight_decay": 0.1, "name": "adamw"}
    assert optimizer_options(_cfg(optimizer="adam").train)["weight_decay"] == 0.0
    # lion_pytorch.Lion defaults (requirements.txt:5) and its own argument names only
    assert optimizer_options(_cfg(optimizer="Lion").train) == {"betas": (0.9, 0.99), "weight_decay": 0.0, "eps": 0.0, "name": "lion"}
    assert optimizer_options(_cfg(optimizer="lion", optimizer_args="weight_decay=0.02 betas=(0.95,0.98)").train)["betas"] == (0.95, 0.98)
    for bad in (dict(optimizer="lion", optimizer_args="eps=1e-6"), dict(optimizer="lion", optimizer_args="use_triton=True"),
                dict(optimizer="prodigy", optimizer_args="amsgrad=True"), dict(optimizer="adam8bit"), dict(optimizer="dadaptsgd"), dict(optimizer="dadaptlion", optimizer_args="eps=1e-6"),
                dict(optimizer="adam", optimizer_args="weight_decay=0.01"), dict(optimizer_args="amsgrad=True"),
                dict(precision="fp16"), dict(precision="float32", optimizer="lion"), dict(lr_scheduler="linear")):
        with pytest.raises(NotImplementedError):
            check_supported(_cfg(**bad))
    # train.precision float32 (config_util.py:75-83 -> weight_dtype, train_lora_xl.py:60-61, 84-90): fp32 adapter state with adam / adamw
    from sliders_amd.cli import adapter_state_dtype
    check_supported(_cfg(precision="float32"))
    check_supported(_cfg(precision="fp32", optimizer="adam"))
    assert adapter_state_dtype(_cfg(precision="float32"), rank=1) == torch.float32 and adapter_state_dtype(_cfg()) == torch.bfloat16
    # prodigyopt.Prodigy's arguments and defaults (requirements.txt: prodigyopt==1.0), lr = 1 is the user's business
    o = optimizer_options(_cfg(optimizer="Prodigy", optimizer_args="weight_decay=0.01 d_coef=2.0 safeguard_warmup=True").train)
    assert o["name"] == "prodigy" and o["weight_decay"] == 0.01 and o["d_coef"] == 2.0 and o["safeguard_warmup"] is True
    assert o["d0"] == 1e-6 and o["betas"] == (0.9, 0.999) and o["decouple"] is True and o["growth_rate"] == float("inf")
    # dadaptation 3.1's two classes with their own arguments and defaults (train_util.py:339-346)
    o = optimizer_options(_cfg(optimizer="DAdaptAdam", optimizer_args="decouple=True weight_decay=0.01 growth_rate=1.02").train)
    assert o["name"] == "dadaptadam" and o["decouple"] is True and o["weight_decay"] == 0.01 and o["growth_rate"] == 1.02
    assert o["d0"] == 1e-6 and o["eps"] == 1e-8 and o["use_bias_correction"] is False
    o = optimizer_options(_cfg(optimizer="dadaptlion").train)
    assert o["name"] == "dadaptlion" and o["betas"] == (0.9, 0.999) and o["weight_decay"] == 0.0
    for name in ("ddim", "ddpm", "lms", "euler_a"):      # model_util.py:230-277: all four for text sliders
        check_supported(_cfg(noise_scheduler=name))
    check_supported(_cfg(), image_slider=True)
    check_supported(_cfg(noise_scheduler="ddpm"), image_slider=True)     # same timestep grid and add_noise as ddim, no .step()
    with pytest.raises(NotImplementedError):             # image sliders: the fused noising step is DDIM-table only
        check_supported(_cfg(noise_scheduler="euler_a"), image_slider=True)
    with pytest.raises(ValueError):
        check_supported(_cfg(lr_scheduler="nope"))
    c = _cfg()
    c.pretrained_model.v2 = c.pretrained_model.v_pred = True      # SD-2.x 768-v: implemented (sd2 config + v-prediction DDIM)
    check_supported(c)
    check_supported(_cfg(lr_scheduler="cosine", optimizer="adam"))


@pytest.mark.parametrize("name", ["constant", "cosine", "cosine_with_restarts", "step"])
def test_lr_schedule_follows_the_torch_scheduler(name):
    """The host-side schedule hands slh_adamw, at iteration i, the lr torch's scheduler would have set after i calls of
    lr_scheduler.step() (train_lora_xl.py:346-347)."""
    from sliders_amd.cli import LrSchedule
    from sliders_amd.train_util import get_lr_scheduler
    lr0, n = 2e-4, 300
    sch = LrSchedule(name, lr0, n)
    prm = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.AdamW([prm], lr=lr0)
    ref = get_lr_scheduler(name, opt, max_iterations=n, lr_min=lr0 / 100)
    seen = []
    for i in range(n):
        assert sch.current() == pytest.approx(opt.param_groups[0]["lr"], rel=1e-12)
        seen.append(sch.current())
        opt.step()
        ref.step()
        sch.step()
    if name != "constant":
        assert min(seen) < lr0
    else:
        assert all(v == lr0 for v in seen)


def test_synthetic_prompt_embeddings_are_stable_across_processes():
    """Seeded by a stable digest of the prompt text, not by Python's per-process salted hash()."""
    import subprocess
    import sys
    code = ("import sys, zlib, torch; sys.path.insert(0, %r); from sliders_amd import cli; "
            "print(zlib.crc32('a photo of a person'.encode()) & 0xFFFFFF)" % ROOT)
    outs = {subprocess.check_output([sys.executable, "-c", code], env=dict(os.environ, PYTHONHASHSEED=str(s))).strip()
            for s in (1, 2)}
    assert len(outs) == 1
    src = open(os.path.join(ROOT, "sliders_amd", "cli.py")).read()
    assert "hash(text)" not in src


def test_single_file_checkpoint_is_rejected_before_loading(tmp_path):
    from sliders_amd.cli import check_model_files
    f = tmp_path / "model.safetensors"
    f.write_bytes(b"\0")
    with pytest.raises(NotImplementedError, match="diffusers-format model directory"):
        check_model_files(str(f))
    check_model_files(str(tmp_path))      # a directory passes this gate (the loader then validates its contents)


def test_image_slider_cli_keeps_the_reference_flags():
    """trainscripts/imagesliders/train_lora-scale-xl.py:464-541: --alpha required, folder / scale lists, stylecheck."""
    from sliders_amd.cli_image import build_parser, parse_folders_scales
    ps = build_parser()
    with pytest.raises(SystemExit):
        ps.parse_args(["--config_file", "c.yaml", "--folder_main", "d/"])            # --alpha is required
    a = ps.parse_args(["--config_file", "c.yaml", "--alpha", "1", "--folder_main", "datasets/eyesize/", "--name", "eye"])
    assert (a.folders, a.scales, a.rank, a.stylecheck) == ("verylow, low, high, veryhigh", "-2, -1, 1, 2", 4, None)
    f, s = parse_folders_scales("bigsize, smallsize", "1, -1")
    assert f == ["bigsize", "smallsize"] and s == [1, -1]
    with pytest.raises(Exception):
        parse_folders_scales("a, b, c", "1, -1")
    for script in ("train_lora-scale-xl.py", "train_lora-scale.py"):
        assert os.path.isfile(os.path.join(ROOT, "trainscripts", "imagesliders", script))


def test_vae_encoder_refuses_cpu():
    from sliders_amd.vae import VaeEncoder, random_vae_state_dict
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VaeEncoder(random_vae_state_dict((128, 128, 128, 128)), "cpu")


def test_generate_parses_the_slider_file_name_like_the_notebooks():
    """XL-sliders-inference.ipynb cell 6: rank / alpha / train_method come from substrings of the checkpoint path."""
    from sliders_amd.generate import build_parser, parse_slider_name
    assert parse_slider_name("models/age_alpha1.0_rank4_noxattn/age_alpha1.0_rank4_noxattn_last.pt") == (4, 1.0, "noxattn")
    assert parse_slider_name("eyesize_alpha2_rank8_full_500steps.pt") == (8, 2.0, "full")
    assert parse_slider_name("x_alpha1.0_rank4_xattn-strict_last.pt")[2] == "xattn-strict"
    assert parse_slider_name("unnamed.pt") == (4, 1.0, "noxattn")
    a = build_parser().parse_args(["--scales=-2,0,2", "--start_noise", "800", "--synthetic"])
    assert a.start_noise == 800 and a.ddim_steps == 50 and a.guidance_scale == 7.5


def test_host_helpers_match_the_reference_run():
    """tests/golden/host_helpers.json is the output of the reference's own train_util.py under fixed seeds
    (tests/golden/make_golden.py host_helpers): the same RNG consumption, order and results here
    (train_util.py:20-57, 136-141, 298-333, 376-419)."""
    import json
    import types
    from sliders_amd import train_util as tu
    from sliders_amd.cli import LrSchedule
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "host_helpers.json")))
    for seed in (0, 1, 7):
        torch.manual_seed(seed)
        assert [list(tu.get_random_resolution_in_bucket(b)) for b in (512, 1024, 512, 768, 1024)] == gold[f"bucket/{seed}"]
        torch.manual_seed(seed)
        got = [tu.get_add_time_ids(h, w, dynamic_crops=True).tolist() for h, w in ((512, 512), (1024, 1024), (768, 512))]
        assert got == gold[f"time_ids_dynamic/{seed}"]
    assert tu.get_add_time_ids(1024, 768, dynamic_crops=False).tolist() == gold["time_ids_static"]
    assert tu.get_add_time_ids(1000, 1001, dtype=torch.bfloat16).float().tolist() == gold["time_ids_bf16"]     # quirk D.8
    lat = tu.get_initial_latents(types.SimpleNamespace(init_noise_sigma=2.5), 2, 64, 96, 3, generator=torch.Generator().manual_seed(3))
    g = gold["initial_latents"]
    assert list(lat.shape) == g["shape"] and float(lat.double().sum()) == g["sum"] and float(lat.flatten()[0]) == g["first"]
    assert torch.equal(lat[:2], lat[2:4]) == g["repeat_equal"]
    a, b = torch.arange(6.0).view(1, 2, 3), 10 + torch.arange(6.0).view(1, 2, 3)
    assert tu.concat_embeddings(a, b, 2).tolist() == gold["concat_embeddings"]
    idx = (0, 1, 9, 10, 99, 100, 101, 299, 300, 500, 699, 700, 999)
    for name in ("constant", "cosine", "cosine_with_restarts", "step"):
        s = LrSchedule(name, 2e-4, 1000)
        lrs = []
        for i in range(1000):
            lrs.append(s.current())
            s.step()
        assert [lrs[i] for i in idx] == gold[f"lr/{name}"], name


def test_vae_checkpoints_with_deprecated_attention_names_are_normalised():
    """SD-1.4 / 1.5 VAE files name the mid-block attention query / key / value / proj_attn (1x1 convs in the oldest ones);
    diffusers renames them at load time, VaeEncoder / VaeDecoder read the file directly and must do the same."""
    from sliders_amd.vae import normalize_vae_key, random_vae_state_dict
    new = random_vae_state_dict(boc=(32, 64), decoder=True)
    back = {"to_q": "query", "to_k": "key", "to_v": "value", "to_out.0": "proj_attn"}
    old = {}
    for k, v in new.items():
        ko = k
        for n, o in back.items():
            if f".attentions.0.{n}." in k:
                ko = k.replace(f".attentions.0.{n}.", f".attentions.0.{o}.")
        old[ko] = v
    assert any(".query." in k for k in old) and any(".proj_attn." in k for k in old)
    assert {normalize_vae_key(k) for k in old} == set(new)
    assert all(normalize_vae_key(k) == k for k in new)
    # names that merely contain the words elsewhere stay untouched
    assert normalize_vae_key("encoder.down_blocks.0.resnets.0.conv1.weight") == "encoder.down_blocks.0.resnets.0.conv1.weight"


def test_step_sampler_ranks_agree_on_shared_draws_including_dynamic_resolution():
    """Data parallel: k and everything drawn from the shared stream (dynamic_resolution bucket, dynamic_crops seed) must be
    identical on every rank in every step - the ranks do the same amount of work and all-reduce once - while the pair index
    differs by rank (sliders_amd/cli.py:225-240 relies on this)."""
    from sliders_amd.parallel import StepSampler
    from sliders_amd.train_util import get_random_resolution_in_bucket
    seqs = []
    for rank in range(2):
        s = StepSampler(7, rank, 2, 8, 50)
        out = []
        for _ in range(20):
            k, pi = s.next()
            st = torch.random.get_rng_state()
            torch.manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=s.shared).item()))
            hw = get_random_resolution_in_bucket(1024)
            torch.random.set_rng_state(st)
            out.append((k, pi, hw))
        seqs.append(out)
    assert [(k, hw) for k, _, hw in seqs[0]] == [(k, hw) for k, _, hw in seqs[1]]
    assert all(a[1] != b[1] for a, b in zip(*seqs))
    assert all(1 <= k <= 49 for k, _, _ in seqs[0])
    # the SD-1.x image-slider script draws k from 1 .. max-2 (train_lora-scale.py:186-188)
    s = StepSampler(1, 0, 1, 3, 49)
    assert max(s.next()[0] for _ in range(400)) == 48


def test_bench_pairs_counter_traffic_only_with_identical_kernel_sources(tmp_path):
    """bench.py attaches roofline.traffic (per-launch bytes from committed --pmc passes) only when the tree it runs from is the tree
    the passes were taken on - as a whole, or in every file the reported kernel is built from (its translation unit, the headers it
    includes, the public header, every tile table).  A changed file of ANOTHER kernel does not void the pairing; a changed file of
    this kernel, a changed tile table or a counter file without per-file hashes does."""
    import json
    import bench
    from sliders_amd import srchash
    k = "gemm_kernel<1, 2, 0, 4, false, 4, false>"
    here = srchash.file_hashes()
    assert set(srchash.kernel_files(k, here)) >= {"gemm.hip", "gemm_common.h", "common.h", "sliders_hip.h"} and \
        "attention.hip" not in srchash.kernel_files(k, here) and all(f in srchash.kernel_files(k, here) for f in here if f.endswith(".json"))
    prof = tmp_path / "profiles"
    prof.mkdir()

    def write(fh, combined):
        json.dump({"tree_head": "abc1234", "kernel_source_hash": combined, "file_hashes": fh,
                   "kernels": {k.replace(", ", "; "): {"fetch_bytes_per_launch": 100, "write_bytes_per_launch": 23, "launches": 1}}},
                  open(prof / "r09_pmc_traffic.json", "w"))
    # 1. identical tree
    write(dict(here), srchash.kernel_source_hash())
    assert bench.pmc_traffic_for(k, str(prof))[0] == 123
    # 2. another kernel's file changed since the passes: still this kernel's numbers
    other = dict(here)
    other["attention.hip"] = "0" * 16
    write(other, "f" * 16)
    t, src = bench.pmc_traffic_for(k, str(prof))
    assert t == 123 and "attention.hip" in src and "byte-identical" in src
    # 3. this kernel's own header changed / a tile table changed / no per-file hashes: no pairing
    for bad in ("gemm_common.h", next(f for f in here if f.endswith(".json"))):
        o2 = dict(here)
        o2[bad] = "0" * 16
        write(o2, "f" * 16)
        assert bench.pmc_traffic_for(k, str(prof))[0] is None
    write({}, "f" * 16)
    t, src = bench.pmc_traffic_for(k, str(prof))
    assert t is None and "re-run" in src


def test_kernel_files_lists_what_each_unit_includes():
    """srchash.kernel_files: for every kernel prefix the listed sources are exactly the translation units (the .hip files of the entry)
    plus the project headers they #include, directly or through another header, read from the source text - a header a unit gains
    or loses has to show up in the map, or bench.py would pair counter traffic with a kernel whose code has changed."""
    from sliders_amd import srchash
    csrc = os.path.join(ROOT, "sliders_amd", "csrc")

    def closure(name, seen):
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(csrc, name)).read(), re.M):
            inc = os.path.basename(inc)            # "../../include/sliders_hip.h" -> sliders_hip.h
            if inc not in seen:
                seen.add(inc)
                if os.path.exists(os.path.join(csrc, inc)):
                    closure(inc, seen)
        return seen

    here = srchash.file_hashes()
    tables = {f for f in here if f.endswith(".json")}
    assert tables and len(srchash.KERNEL_UNITS) >= 6
    for prefix, listed in srchash.KERNEL_UNITS.items():
        units = [f for f in listed if f.endswith(".hip")]
        assert units and units[0].startswith(("gemm", "attention")), prefix
        want = set(units)
        for u in units:
            want |= closure(u, set())
        assert {"common.h", "sliders_hip.h"} <= want, prefix
        got = set(srchash.kernel_files(prefix + "<1>", here))
        assert got - tables == want, (prefix, sorted(got - tables), sorted(want))
        assert got & tables == tables and got <= set(here), prefix
    assert "attention_common.h" in srchash.kernel_files("attn_fwd_ks_kernel", here)
    assert {"addressing.h", "gemm_dispatch.h"} <= set(srchash.kernel_files("gemm5_kernel<false, 4>", here))



def test_dry_run_plans_the_program_the_real_plan_runs(monkeypatch):
    """UNetEngine sizes its arena by planning against _VirtualWeights (pointer-less).  The dry run must take the same branches as
    the real plan - same launches, same tiles, same arena high-water mark - for every mode: a forgotten attribute (geglu16 in
    round 4: the dry run planned GEGLU.proj on the 32 | 32 path, the real plan on the 16 | 16 path with other tile keys) makes them
    two different programs and the sizing a guess."""
    from sliders_amd.unet import _VirtualWeights
    cfg = CONFIGS["sdxl"]()
    store = LoraStore(cfg, train_method="noxattn", init="none")
    store.temb_tcol = torch.zeros(1, dtype=torch.int32)
    real = _FakeWeights(cfg)
    for mode in ("off", "on", "train"):
        plans = []
        for w in (real, _VirtualWeights(real)):
            va, vz = Arena(1 << 50, None), Arena(1 << 40, None)
            p = UNetPlan(cfg, w, va, vz, 2, 128, 128, 77, store if mode != "off" else None, mode, 0x10)
            plans.append((p, va))
        (pr, ar), (pv, av) = plans
        assert pv.prog.op_names == pr.prog.op_names, mode
        assert [d.tile for o, d in pv.prog.ops if o == lib.OP_GEMM] == [d.tile for o, d in pr.prog.ops if o == lib.OP_GEMM], mode
        assert [d.geglu for o, d in pv.prog.ops if o == lib.OP_GEMM] == [d.geglu for o, d in pr.prog.ops if o == lib.OP_GEMM], mode
        assert av.high_water >= ar.high_water, mode


def test_refused_layernorm_fold_leaves_nothing_in_the_program(monkeypatch):
    """ln_gemm tries the folded product first and falls back to LayerNorm + product when gemm() refuses.  With SLIDERS_LORA_UNFUSED
    the refusal comes AFTER the adapter's down-projection was recorded (round-4 advisor finding): the rollback must drop that
    launch too, otherwise it writes T into arena bytes that were handed out again."""
    cfg = CONFIGS["sdxl"]()
    store = LoraStore(cfg, train_method="noxattn", init="none")
    store.temb_tcol = torch.zeros(1, dtype=torch.int32)
    monkeypatch.setenv("SLIDERS_LORA_UNFUSED", "1")
    va, vz = Arena(1 << 50, None), Arena(1 << 40, None)
    p = UNetPlan(cfg, _FakeWeights(cfg), va, vz, 2, 128, 128, 77, store, "on", 0x10)
    names = p.prog.op_names
    downs = [n for n in names if n.endswith(".lora_down")]
    assert len(downs) == len(set(downs)), "a rolled-back fold must not leave its down-projection behind"
    # every recorded skinny launch writes a buffer that no LATER allocation overlaps (the stale launch wrote into re-allocated bytes)
    spans = sorted((s, e) for s, e, _ in va.allocs)
    assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))


class _FakeWeightsKvAll(_FakeWeights):
    """_FakeWeights plus the batched text K/V layout of WeightStore (weights.py: all attn2 K / V projections concatenated)."""

    def __init__(self, cfg):
        super().__init__(cfg)
        paths = [n for n, m in build_tree(cfg).named_modules() if n.endswith(".attn2")]
        widths = {}
        for n, m in build_tree(cfg).named_modules():
            if n.endswith(".attn2.to_k"):
                widths[n[:-len(".to_k")]] = m.out_dim
        self.kv_all_vbase = sum(widths[a] for a in paths)
        row = 0
        for a in paths:
            self.kv_all_offset[a] = (row, self.kv_all_vbase + row)
            row += widths[a]
        self.gemm_shape["attn2_kv_all.w"] = (2 * self.kv_all_vbase, cfg.cross_attention_dim)


@pytest.mark.parametrize("ctx_len,fused", [(77, True), (64, False), (48, False), (96, True), (97, False)])
def test_fused_cross_attention_gate_matches_the_kernel_checks(ctx_len, fused):
    """attn2.to_q carries the cross-attention in its epilogue only where slh_gemm accepts xa_*: two 64-key V^T tiles are always
    staged, so the padded key count roundup(ctx_len, 64) must reach 128 (65..96 keys).  Shorter contexts keep the two launches
    instead of failing inside slh_gemm (round-4 advisor finding)."""
    cfg = CONFIGS["sdxl"]()
    va, vz = Arena(1 << 50, None), Arena(1 << 40, None)
    p = UNetPlan(cfg, _FakeWeightsKvAll(cfg), va, vz, 2, 128, 128, ctx_len, None, "off", 0x10)
    assert p.kv_all is not None and p.vt_all is not None
    xa = [d for o, d in p.prog.ops if o == lib.OP_GEMM and d.xa_k]
    assert bool(xa) == fused
    assert all(d.xa_ldvt >= 128 and d.xa_tk == ctx_len and d.N % 64 == 0 and (d.tile & 0xFFFFF) == 0x4412 for d in xa)
    n_cross = sum(1 for n in p.prog.op_names if n.endswith("attn2.sdpa"))
    n_blocks = sum(1 for n in p.prog.op_names if n.endswith("attn2.q"))
    assert n_cross + len(xa) == n_blocks          # every block runs its cross-attention exactly once, one way or the other


def test_fp32_adapter_state_store_layout_and_checkpoint(tmp_path):
    """train.precision float32: LoraStore keeps an fp32 master + fp32 moments next to the bf16 buffer the kernels read; the reference
    draws of the initialisation land in both; the checkpoint is written from the master in fp32 (the reference saves in train.precision,
    quirk D.7) and strict-loads back without loss; a bf16 store has no master at all."""
    cfg = CONFIGS["tiny_sdxl"]()
    torch.manual_seed(4)
    s32 = LoraStore(cfg, rank=4, alpha=1.0, train_method="noxattn", state_dtype=torch.float32)
    torch.manual_seed(4)
    s16 = LoraStore(cfg, rank=4, alpha=1.0, train_method="noxattn")
    assert s16.master is None and s16.exp_avg.dtype == torch.bfloat16
    assert s32.master.dtype == s32.exp_avg.dtype == s32.exp_avg_sq.dtype == torch.float32 and s32.params.dtype == torch.bfloat16
    assert torch.equal(s32.params, s16.params) and torch.equal(s32.master.to(torch.bfloat16), s32.params)
    assert (s32.master != s32.params.float()).any(), "the master keeps the bits bf16 drops"
    g = torch.Generator().manual_seed(1)
    s32.master.add_(torch.randn(s32.numel, generator=g) * 1e-3)
    sd = s32.state_dict(torch.float32)
    assert all(v.dtype == torch.float32 for v in sd.values())
    torch.save(sd, tmp_path / "a.pt")
    t = LoraStore(cfg, rank=4, alpha=1.0, train_method="noxattn", state_dtype=torch.float32, init="none")
    t.load_state_dict(torch.load(tmp_path / "a.pt"), strict=True)
    assert torch.equal(t.master, s32.master) and torch.equal(t.params, s32.master.to(torch.bfloat16))
    with pytest.raises(NotImplementedError):
        LoraStore(cfg, state_dtype=torch.float16)


def test_bench_gpus_flag_relaunches_or_refuses():
    """`python bench.py --gpus N` (N > 1) outside torch.distributed.run: the script re-launches itself as N ranks of one node over
    127.0.0.1 - exactly the driver's command line - and refuses, non-zero, when the node shows fewer GPUs; it never runs one rank under
    an `n_gpus: N` label (--gpus was parsed and never read)."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    argv = ["--gpus", "8", "--steps", "5", "--warmup", "2"]
    cmd = bench.multi_gpu_relaunch(8, argv, {}, 8)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    k = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[k + 1:] == argv
    # already a rank of a torch.distributed.run job, or a single-GPU run: nothing to re-launch
    assert bench.multi_gpu_relaunch(8, argv, {"WORLD_SIZE": "8"}, 8) is None
    assert bench.multi_gpu_relaunch(1, [], {}, 0) is None
    # fewer devices than ranks: loud, non-zero
    with pytest.raises(SystemExit) as ex:
        bench.multi_gpu_relaunch(8, argv, {}, 1)
    assert "--gpus 8" in str(ex.value) and "1 GPU" in str(ex.value)
    # end to end on this GPU-less container: the process exits non-zero and prints no JSON line
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300, env={**os.environ, "WORLD_SIZE": ""})
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        assert r.returncode != 0 and "n_gpus" not in r.stdout and "--gpus 2" in r.stderr


def test_bench_dump_outputs_are_float32_and_fit_64mb(tmp_path, monkeypatch):
    """`bench.py --dump-outputs DIR`: the loss and the adapter state the last timed step left, one float32 .npy each, exactly the
    values of the device buffers, within 64 MB at the benchmarked SDXL size."""
    import sys
    import types

    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    st = LoraStore(CONFIGS["sdxl"](), rank=4, alpha=1.0, train_method="noxattn", device="cpu")
    g = torch.Generator().manual_seed(0)
    for t in (st.params, st.grads, st.exp_avg):
        t.copy_(torch.randn(t.shape, generator=g))
    bench.dump_outputs(str(tmp_path), types.SimpleNamespace(loss=torch.tensor([0.125])), st, "text")
    files = {p.name: np.load(p) for p in tmp_path.iterdir()}
    assert sorted(files) == ["lora_exp_avg.npy", "lora_grads.npy", "lora_params.npy", "loss.npy"]
    assert all(a.dtype == np.float32 for a in files.values())
    assert files["loss.npy"].tolist() == [0.125]
    assert np.array_equal(files["lora_params.npy"], st.params.float().numpy())
    assert np.array_equal(files["lora_grads.npy"], st.grads.numpy())
    assert sum(a.nbytes for a in files.values()) <= 64 * 2 ** 20
    # a plain command line measures the headline only
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (3, 1)


def test_gemm_kernel_name_comes_from_the_library():
    """slh_gemm_kernel_name: the kernel a descriptor runs on, named by the dispatch code itself (no device needed) - bench.py and the
    PMC pairing use it instead of rebuilding template arguments from tile codes."""
    d = lib.GemmDesc(a0=0x1000, w=0x2000, c=0x3000, lda0=1280, ca0=1280, mode=0, stride=1, ldw=0, M=2048, N=1280, K=1280, ldc=1280,
                     rows_per_sample=1024, w_layout=1)
    for tile, want in ((0x5425, "gemm5_kernel<false, 4>"), (0x5525, "gemm5_kernel<false, 5>"), (0x4412, "gemm_kernel<1, 2, 0, 4, false, 4, false>"),
                       (0x8014, "gemm8pb_kernel<1, 4, 0, false>"), (0x8042, "gemm8p_kernel<0, false>"), (0x11, "gemm_kernel<1, 1, 0, 2, false, 2, false>"),
                       (0x4322, "gemm_kernel<2, 2, 0, 3, false, 4, false>")):
        d.tile = tile
        assert lib.gemm_kernel_name(d) == want, hex(tile)
    d.tile = 0x4422          # 256 x 128 stages (256 + 128) * 128 B = 48 KB per slot: a 4-slot ring does not fit 160 KB, the launcher runs 3
    assert lib.gemm_kernel_name(d) == "gemm_kernel<2, 2, 0, 3, false, 4, false>"
    d.tile, d.K = 0x5425, 100            # a descriptor slh_gemm refuses: the error, not a name
    with pytest.raises(lib.SlidersHipError):
        lib.gemm_kernel_name(d)


# ---------------------------------------------------------------------------------------------------------------------------
# The element-wise GEMM bound of tests/util.py has teeth (and lets a correct kernel through)
# ---------------------------------------------------------------------------------------------------------------------------
def _trunc_bf16(x32):
    """fp32 -> bf16 by dropping the low 16 bits (round towards zero): the mutant the whole-tensor norm cannot see"""
    return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


@pytest.mark.parametrize("M,N,K", [(300, 328, 192), (256, 960, 1280), (154, 256, 5760)])
def test_gemm_elementwise_bound_passes_a_standin_and_fails_four_mutants(M, N, K):
    """Stand-in kernel: torch's fp32 CPU product + bias + residual, rounded to bf16 (nearest).  It must meet the bound
    |got - ref| <= 2^-8 |ref| + n 2^-24 S at every element and |b| <= 0.05; each mutant - truncation instead of rounding, the last
    64 of K missing in one 32 x 64 block, the bias missing in the last 4 columns, a stale last row - must fail at least one of the
    two checks, and truncation must fail the rounding statistic, at every shape.  (A bound of 2^-9 |ref| + n 2^-23 S fails the
    stand-in itself, which is why this proof stays in the suite.)"""
    from tests.util import check_elementwise, elementwise_bound, rounding_statistic, STAT_LIMIT
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    bias = torch.randn(N, generator=g).bfloat16()
    res = torch.randn(M, N, generator=g).bfloat16()
    xd, wd, bd, rd = x.double(), w.double(), bias.double(), res.double()
    ref = xd @ wd.t() + bd + rd
    sabs = xd.abs() @ wd.abs().t() + bd.abs() + rd.abs()
    bound = elementwise_bound(ref, sabs, K + 2)
    acc32 = x.float() @ w.float().t() + bias.float() + res.float()
    good = acc32.bfloat16()
    worst, _, b = check_elementwise("stand-in", good, ref, bound)
    print(f"[parity] stand-in M{M} N{N} K{K}: worst |got - ref| / bound = {worst:.3f}, b = {b:+.4f}")
    assert worst <= 1.0 and b is not None and abs(b) <= STAT_LIMIT

    def fails(name, got):
        try:
            check_elementwise(name, got, ref, bound)
        except AssertionError as e:
            print(f"[parity] mutant {name} M{M} N{N} K{K}: caught - {str(e)[:160]}")
            return True
        return False

    trunc = _trunc_bf16(acc32)
    assert fails("truncation", trunc)
    bt, cnt = rounding_statistic(trunc, ref)
    assert bt is not None and abs(bt) > STAT_LIMIT, (bt, cnt)          # the statistic alone sees it, at every K
    m0, n0 = (M - 32) // 32 * 32, 64
    short = acc32.clone()
    short[m0:m0 + 32, n0:n0 + 64] -= x.float()[m0:m0 + 32, K - 64:] @ w.float()[n0:n0 + 64, K - 64:].t()
    assert fails("dropped K tile", short.bfloat16())
    nobias = acc32.clone()
    nobias[:, N - 4:] -= bias.float()[N - 4:]
    assert fails("bias quad", nobias.bfloat16())
    stale = good.clone()
    stale[M - 1] = good[M - 2]
    assert fails("stale last row", stale)


# ---------------------------------------------------------------------------------------------------------------------------
# The GEMM test matrix (tests/gemm_matrix.py) against the library's capability rule
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gemm_matrix_cases():
    from tests import gemm_matrix as gm
    return gm, gm.enumerate_cases()


def test_gemm_capability_matches_the_recorded_table(gemm_matrix_cases):
    """slh_gemm_tile_ok's answers over the whole matrix equal tests/data/gemm_capability.json (python -m tests.gemm_matrix --write):
    a change that widens or narrows the rule shows in the diff of that file."""
    gm, (acc, _) = gemm_matrix_cases
    rec = json.load(open(gm.DATA))
    table = gm.capability_table(acc)
    assert sorted(table) == sorted(rec["table"]), set(table) ^ set(rec["table"])
    diff = {k: (table[k], rec["table"][k]) for k in table if table[k] != rec["table"][k]}
    assert not diff, f"the rule and the recorded table disagree (library, file): {diff}"
    assert rec["accepted"] == len(acc)
    assert os.path.getsize(gm.DATA) < 200 * 1024


def test_gemm_dispatch_matches_the_recorded_digests(gemm_matrix_cases):
    """The launch behind every accepted case of the matrix and every product of the dry-run plans (slh_gemm_launch_query: kernel
    instantiation, grid, block size, FNV-1a of the argument struct's bytes - group_m, tile counts, split-K cut, store16, kper are in
    there) equals tests/data/gemm_dispatch.json (python -m tests.gemm_matrix --write-dispatch; --dispatch KEY prints the tuples of one
    key): a change of the dispatch that keeps every result but moves a launch shows here, on any machine."""
    gm, (acc, _) = gemm_matrix_cases
    rec = json.load(open(gm.DISPATCH))
    got = gm.dispatch_digests(acc)
    assert sorted(got) == sorted(rec) == ["matrix", "plans"]
    assert len(got["plans"]) == 12 and sorted(got["matrix"]) == sorted(gm.capability_table(acc))
    bad = [f"{sec}: {k}" for sec in got for k in sorted(set(got[sec]) | set(rec[sec])) if got[sec].get(k) != rec[sec].get(k)]
    assert not bad, f"{len(bad)} keys launch differently from the recorded dispatch (python -m tests.gemm_matrix --dispatch KEY): {bad}"
    assert os.path.getsize(gm.DISPATCH) < 200 * 1024


def test_gemm_matrix_is_not_hollow(gemm_matrix_cases):
    """Every tile code names a kernel and runs the bare recipe at the exact-multiple shape; every recipe is accepted by at least one
    tile of each family the header (include/sliders_hip.h) says takes it - Recipe.families restates the header's text, so this is
    the check that header and rule agree; at least 4000 cases are accepted; the matrix covers every tile code the tuning tables
    and the hand-written kernel tests name."""
    gm, (acc, ref) = gemm_matrix_cases
    bare_a = {c.tile & 0xFFFF for c in acc if c.recipe.name == "bare" and c.cls == "a" and (c.tile >> 16) == 0}
    assert set(gm.TILES) <= bare_a, [hex(t) for t in set(gm.TILES) - bare_a]
    for c in acc:
        if c.recipe.name == "bare" and c.cls == "a":
            off, _ = gm.layout(c)
            assert lib.gemm_kernel_name(gm.make_desc(c, gm._FAKE_BASE, off))
    took = {}
    for c in acc:
        took.setdefault(c.recipe.name, set()).add(gm.family(c.tile))
    miss = set()
    for r in gm.RECIPES:
        # (tile 0 is no family of the header: the heuristic's pick is one of the explicit tiles, and takes what that tile takes)
        want = set(r.families) - {"auto"}
        miss.update({(r.name, f) for f in want - took.get(r.name, set())})
    assert not miss, f"the header promises these (recipe, family) pairs, the rule accepts no case of them: {sorted(miss)}"
    assert len(acc) >= 4000, len(acc)
    # split-K does not drop out where it matters: a tile that takes the bare recipe with split-K at the exact-multiple shape also takes it
    # at the ragged shape (b) and at K >= 2560 (kbig), with S = 2 and with S = 3 - uneven slices, many K tiles per slice
    def sk(cls, S):
        return {c.tile & 0xFFFF for c in acc if c.recipe.name == "bare" and c.cls == cls and (c.tile >> 16) == S}
    split_a = sk("a", 2) | sk("a", 3)
    assert {gm.family(t) for t in split_a} == {"auto", "r2", "r4", "pp"}
    for cls in ("b", "kbig"):
        for S in (2, 3):
            assert split_a <= sk(cls, S), (cls, S, sorted(hex(t) for t in split_a - sk(cls, S)))
    # ... and every split-K case of the matrix really cuts K into at least two slices
    for c in acc:
        S = (c.tile >> 16) & 15
        if S > 1:
            nk = c.dims["K"] // 64
            per = -(-nk // S)
            assert -(-nk // per) >= 2, c.id
    # tile codes named elsewhere in the repository
    named = set()

    def walk(x):
        if isinstance(x, dict):
            for v in x.values():
                walk(v)
        elif isinstance(x, list):
            for v in x:
                walk(v)
        elif isinstance(x, int):
            named.add(x & 0xFFFF)
    for fn in os.listdir(os.path.join(ROOT, "sliders_amd", "tuning")):
        if fn.endswith(".json"):
            walk(json.load(open(os.path.join(ROOT, "sliders_amd", "tuning", fn))))
    for fn in ("test_kernels_gpu.py", "test_gemm7_gpu.py"):
        for line in open(os.path.join(ROOT, "tests", fn)):
            if "tile" in line and "parametrize" in line:
                named |= {int(m, 16) & 0xFFFF for m in re.findall(r"0x[0-9a-fA-F]+", line)}
    named = {t for t in named if t and (t >> 12) in (0, 4, 5, 7, 8)}
    missing = sorted(hex(t) for t in named - set(gm.TILES))
    assert not missing, f"tile codes the tuning tables / kernel tests name but the matrix does not sweep: {missing}"


def test_gemm_tile_codes_name_a_kernel_or_are_refused():
    """Every nibble of bits 0-15 of a tile code is read by the dispatch or must be zero: 0x5xxx codes other than 0x5425 / 0x5525, unknown
    wave codes and ring depths, ring-depth bits on a ping-pong code (0x8142, 0x8f15) and codes without a block tile (MI = 0: 0x0002,
    0x4000 ...; only an all-zero code, with or without S, asks for the heuristic) are refused with a message; the aliases the header allows (WM 2 = 0, stages 2 = 0) name the same kernel; vt_also_c without vt_out,
    ln_mr_out without ln_in and geglu_pre without geglu are refused by every family (the 64 x 160 tile used to take the first)."""
    from tests import gemm_matrix as gm

    def desc(tile, wl, M=256, N=320, K=256, **kw):
        c = gm.plan_case(gm.RECIPE["bare"], 0x11, 0, wl, "a")
        off, _ = gm.layout(c)
        d = gm.make_desc(c, gm._FAKE_BASE, off, tile)
        d.M, d.N, d.K, d.ca0, d.lda0, d.ldc, d.ldw, d.rows_per_sample = M, N, K, K, K, N, 0 if wl else K, M
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for tile, wl in ((0x5425, 1), (0x5525, 1), (0x7645, 1), (0x11, 0), (0x4412, 1), (0x8042, 0), (0x8015, 1), (0, 0), (0x20000, 0)):
        assert lib.gemm_tile_ok(desc(tile, wl)), hex(tile)
    for tile, wl in ((0x5000, 1), (0x5999, 1), (0x5426, 1), (0x1011, 0), (0x3011, 0), (0x6011, 0), (0x9011, 0), (0x911, 0), (0x4112, 0),
                     (0x8142, 0), (0x8942, 0), (0x8f15, 1), (0x8415, 1), (0x0002, 0), (0x4002, 0), (0x8002, 0), (0x4000, 0), (0x2000, 0),
                     (0x0400, 0), (0x20002, 0)):
        d = desc(tile, wl)
        assert not lib.gemm_tile_ok(d), hex(tile)
        with pytest.raises(lib.SlidersHipError, match="tile"):
            lib.gemm_kernel_name(d)
    assert lib.gemm_kernel_name(desc(0x2011, 0)) == lib.gemm_kernel_name(desc(0x11, 0))
    assert lib.gemm_kernel_name(desc(0x211, 0)) == lib.gemm_kernel_name(desc(0x11, 0))
    for tile in (0x5425, 0x7645, 0x4412):
        for kw in (dict(vt_also_c=1), dict(ln_mr_out=gm._FAKE_BASE), dict(geglu_pre=gm._FAKE_BASE, ld_pre=320)):
            d = desc(tile, 1, **kw)
            assert not lib.gemm_tile_ok(d), (hex(tile), kw)
            with pytest.raises(lib.SlidersHipError, match="slh_gemm"):
                lib.gemm_kernel_name(d)


def test_gemm_tile_decoder_and_rule_agree_on_every_code():
    """All 65 536 values of tile bits 0-15, on a bare packed-weight product every family takes at whole-tile shape (512 x 1280 x 320: 64 |
    128 | 256 rows, 64 | 128 | 160 | 256 | 320 columns): slh_gemm_tile_ok accepts exactly the 30 codes the matrix sweeps, code 0 and
    the header's two aliases of them (family 2 = 0, ring slots 2 = 0); tuning.tile_fields - the Python decoder - gives each accepted
    code the family and block size of tests/gemm_matrix.py's own restatement."""
    from sliders_amd.tuning import tile_fields
    from tests import gemm_matrix as gm
    M, N, K = 512, 1280, 320
    d = lib.GemmDesc(a0=gm._FAKE_BASE, w=gm._FAKE_BASE + (1 << 24), c=gm._FAKE_BASE + (2 << 24), lda0=K, ca0=K, mode=0, stride=1, ldw=0,
                     M=M, N=N, K=K, ldc=N, rows_per_sample=M, w_layout=1)

    def canonical(code):          # the header's aliases folded: 4-wave family 2 -> 0; ring slots 2 -> 0 (double buffer) on the ring families
        fam, st = (code >> 12) & 15, (code >> 8) & 15
        fam = 0 if fam == 2 else fam
        st = 0 if fam in (0, 4) and st == 2 else st
        return fam << 12 | st << 8 | (code & 0xFF)
    swept = set(gm.TILES)
    assert len(swept) == 31 and 0 in swept
    want = {0} | {code for code in range(1 << 16) if canonical(code) in swept - {0}}      # (0x2000, 0x0200: aliases of no code)
    got = set()
    for code in range(1 << 16):
        d.tile = code
        if lib.gemm_tile_ok(d):
            got.add(code)
    assert got == want, (sorted(hex(t) for t in got - want)[:20], sorted(hex(t) for t in want - got)[:20])
    assert len(got) == 31 + 12 + 7 + 4         # + family 2 of the twelve 4-wave codes, + slots 2 of the seven double-buffer ring codes, + both
    names = {0: "r2", 4: "r4", 8: "pp", 5: "g5", 7: "g7"}
    for code in sorted(got):
        f = tile_fields(code)
        if code == 0:
            assert gm.family(code) == "auto" and (f.bm, f.bn) == (0, 0)
            continue
        c = canonical(code)
        assert names[f.family] == gm.family(c) and (f.bm, f.bn) == gm.block(c), hex(code)
        assert (f.splitk, f.slots, f.mi, f.ni) == (0, (code >> 8) & 15, (code >> 4) & 15, code & 15), hex(code)
    assert tile_fields(0x35425).splitk == 3 and tile_fields(0x20000) == (2, 0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("name,hw,method", [("tiny_sdxl", 16, "noxattn"), ("tiny_sd1", 16, "full"), ("sdxl", 128, "noxattn"), ("sdxl", 64, "noxattn")])
def test_every_gemm_of_the_dry_run_plans_passes_the_capability_rule(name, hw, method):
    """Every slh_gemm descriptor of every dry-run plan (adapters off / on / training forward + backward) is one the capability rule
    accepts, names a kernel, and - where it writes vt_out - has no padding columns: a change that narrows the rule cannot strand a
    plan without this test saying which product."""
    cfg = CONFIGS[name]()
    store = LoraStore(cfg, train_method=method, init="none")
    store.temb_tcol = torch.zeros(1, dtype=torch.int32)
    n = 0
    for mode in ("off", "on", "train"):
        va, vz = Arena(1 << 50, None), Arena(1 << 40, None)
        p = UNetPlan(cfg, _FakeWeights(cfg), va, vz, 2, hw, hw, 77, store if mode != "off" else None, mode, 0x10)
        progs = [p.prog] + ([BackwardPlan(p, 1, 1, 0x20).prog] if mode == "train" else [])
        for pr in progs:
            for o, d in pr.ops:
                if o != lib.OP_GEMM:
                    continue
                n += 1
                assert lib.gemm_tile_ok(d), f"{name} {mode}: M{d.M} N{d.N} K{d.K} tile 0x{d.tile:x}: {lib.last_error()}"
                assert lib.gemm_kernel_name(d)
                assert not d.vt_out or d.vt_ld == d.vt_tokens
    assert n > 100


# ---------------------------------------------------------------------------------------------------------------------------
# The attention test matrix (tests/attention_matrix.py): the library names its kernels, the bounds admit an honest implementation and
# reject mutants of it, and the matrix reaches every form
# ---------------------------------------------------------------------------------------------------------------------------
def test_attention_kernel_names_come_from_the_library():
    """slh_attn_fwd_kernel_name / slh_attn_bwd_kernel_names: answered by the dispatch code (attn_fwd_choose, launch_bwd_dq / _dkv), no
    device needed; the SLH_ATTN_NW2 / SLH_ATTN_KS knobs are part of the answer; a refused descriptor gives the error, not a name."""
    import subprocess
    import sys
    from tests import attention_matrix as am
    F = am.FwdCase
    for c, want in ((F(4, 16, 1024, 77, 64, "a"), "attn_fwd_kernel<4, 1, true>"), (F(4, 16, 1024, 192, 160, "a"), "attn_fwd_kernel<4, 3, false>"),
                    (F(1, 3, 192, 192, 80, "a"), "attn_fwd_kernel<2, 2, false>"), (F(2, 10, 1024, 1024, 64, "a"), "attn_fwd_ks_kernel"),
                    (F(1, 128, 64, 256, 64, "a"), "attn_fwd_kernel<2, 1, false>"), (F(1, 129, 64, 256, 64, "a"), "attn_fwd_ks_kernel"),
                    (F(6, 64, 128, 256, 64, "a"), "attn_fwd_ks_kernel"), (F(1, 769, 64, 256, 64, "a"), "attn_fwd_kernel<4, 1, false>"),
                    (F(2, 10, 1024, 1024, 80, "a"), "attn_fwd_kernel<2, 2, false>"), (F(2, 10, 1024, 320, 64, "a"), "attn_fwd_kernel<2, 1, false>")):
        d = am.fwd_desc(c)
        assert lib.attn_fwd_kernel_name(d) == want, c.id
        assert lib.attn_carries_touch(d) == (want == "attn_fwd_ks_kernel"), c.id
    Bc = am.BwdCase
    assert am.bwd_names(Bc(2, 2, 100, 100, 40, "a")) == ("attn_bwd_dq_kernel<1>", "attn_bwd_dkv_kernel<1, 2>")
    assert am.bwd_names(Bc(2, 2, 100, 100, 80, "a")) == ("attn_bwd_dq_kernel<2>", "attn_bwd_dkv_kernel<2, 2>")
    assert am.bwd_names(Bc(2, 2, 100, 100, 160, "a")) == ("attn_bwd_dq_kernel<3>", "attn_bwd_dkv_kernel<3, 1>")
    assert am.bwd_names(Bc(2, 2, 100, 77, 160, "a", need_dkv=0)) == ("attn_bwd_dq_kernel<3>", "")
    d = am.fwd_desc(F(1, 3, 192, 192, 64, "a"))
    d.D = 44
    with pytest.raises(lib.SlidersHipError, match="head_dim"):
        lib.attn_fwd_kernel_name(d)
    d = am.bwd_desc(Bc(2, 2, 100, 100, 64, "a"))
    d.qt = 0
    with pytest.raises(lib.SlidersHipError, match="dK/dV need"):
        lib.attn_bwd_kernel_names(d)
    # the knobs are read once per process
    code = ("from tests import attention_matrix as am; F = am.FwdCase; "
            "print(am.fwd_name(F(4, 16, 1024, 77, 64, 'a')), '|', am.fwd_name(F(2, 10, 1024, 1024, 64, 'a')), '|', am.fwd_name(F(4, 16, 1024, 256, 64, 'a')))")
    for env, want in (({"SLH_ATTN_NW2": "1"}, "attn_fwd_kernel<2, 1, true> | attn_fwd_ks_kernel | attn_fwd_kernel<2, 1, false>"),
                      ({"SLH_ATTN_KS": "0"}, "attn_fwd_kernel<4, 1, true> | attn_fwd_kernel<2, 1, false> | attn_fwd_kernel<4, 1, false>"),
                      ({"SLH_ATTN_KS": "2"}, "attn_fwd_kernel<4, 1, true> | attn_fwd_ks_kernel | attn_fwd_ks_kernel")):
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env={**os.environ, **env}, capture_output=True, text=True, check=True).stdout
        assert out.strip() == want, (env, out)


def _attn_fwd_check(am, c, key_split=False, mutant=None, seed=1):
    """stand-in (or a mutant of it) against the forward bounds: {output: (worst ratio, b)} or {output: the AssertionError's text}"""
    from tests.util import check_elementwise
    L = am.make_inputs(c, "cpu", seed)
    q, k, v = (am.heads(L[n]) for n in "qkv")
    o, bo, l, bl = am.forward_reference(q, k, v, c.D ** -0.5)
    go, gl = am.standin_forward(q, k, v, c.D ** -0.5, key_split, mutant)
    res = {}
    for nm, g, r, b in (("o", go, o, bo), ("lse", gl, l, bl)):
        try:
            w, _, bb = check_elementwise(f"{c.id} {mutant or 'stand-in'} [{nm}]", g, r, b, statistic=nm == "o")
            res[nm] = (w, bb)
        except AssertionError as e:
            res[nm] = str(e)
    return res


def _attn_bwd_check(am, c, mutant=None, pad=float("nan"), seed=1):
    from tests.util import check_elementwise
    L = am.make_inputs(c, "cpu", seed)
    q, k, v, do = (am.heads(L[n]) for n in ("q", "k", "v", "do"))
    sc = c.D ** -0.5
    o, lse = am.forward_for_backward(q, k, v, sc)
    ref = am.backward_reference(q, k, v, o, do, lse, sc, bool(c.need_dkv))
    padding = torch.full((64,), pad)
    got = am.standin_backward(q, k, v, o, do, torch.cat([lse.reshape(-1), padding]), padding, sc, bool(c.need_dkv), mutant)
    res = {}
    for nm, (r, b) in ref.items():
        try:
            w, _, bb = check_elementwise(f"{c.id} {mutant or 'stand-in'} [{nm}]", got[nm], r, b, statistic=am.bwd_takes_statistic(c) and nm != "delta")
            res[nm] = (w, bb)
        except AssertionError as e:
            res[nm] = str(e)
    return res, got


_ATTN_FWD_SMALL = [("a", 2, 4, 256, 192, 64), ("ac", 2, 4, 256, 192, 64), ("bc", 2, 4, 256, 77, 64), ("dc", 2, 4, 256, 256, 64), ("ec", 1, 8, 320, 384, 64),
                   ("fc", 2, 4, 256, 256, 160), ("g", 2, 4, 200, 65, 64), ("gc", 2, 4, 256, 333, 80), ("b", 2, 2, 129, 5, 40), ("a", 2, 2, 33, 1, 64)]


@pytest.mark.parametrize("cls,B,H,Tq,Tk,D", _ATTN_FWD_SMALL, ids=[f"{s[0]}-Tq{s[3]}-Tk{s[4]}-D{s[5]}" for s in _ATTN_FWD_SMALL])
def test_attention_forward_bounds_admit_the_standin(cls, B, H, Tq, Tk, D):
    """every input class, at small shapes: the stand-in of attn_fwd_kernel - and of the key-split kernel where Tk allows - meets the o and
    lse bounds at every element, and the rounding statistic wherever it applies (class c with >= 10000 elements above 0.1: it must)"""
    from tests import attention_matrix as am
    from tests.util import STAT_LIMIT
    c = am.FwdCase(B, H, Tq, Tk, D, cls)
    for ks in ((False, True) if Tk % 128 == 0 and Tk >= 256 else (False,)):
        res = _attn_fwd_check(am, c, key_split=ks)
        assert all(isinstance(r, tuple) for r in res.values()), res
        (w, b), (wl, _) = res["o"], res["lse"]
        print(f"[parity] attention stand-in {c.id} key_split={ks}: worst |got - ref| / bound = {w:.3f} (o), {wl:.3f} (lse), b = {b}")
        assert w <= 1.0 and wl <= 1.0
        if "c" in cls:
            assert b is not None and abs(b) <= STAT_LIMIT
    if "g" in cls:       # the class does what it says: the last key leads by more than 30 in the exponent
        L = am.make_inputs(c, "cpu", 1)
        s = (am.heads(L["q"]).double() @ am.heads(L["k"]).double().transpose(-1, -2)) * D ** -0.5
        assert float((s[..., -1] - s[..., :-1].amax(-1)).min()) > 30.0
    if "e" in cls or "f" in cls:   # the row maximum rises (falls) from tile to tile for nearly every row
        L = am.make_inputs(c, "cpu", 1)
        s = (am.heads(L["q"]).double() @ am.heads(L["k"]).double().transpose(-1, -2)) * D ** -0.5
        tm = torch.stack([s[..., t:t + 64].amax(-1) for t in range(0, Tk, 64)], -1)
        step = tm[..., 1:] - tm[..., :-1]
        assert float(((step > 0) if "e" in cls else (step < 0)).double().mean()) > 0.99
    if Tk == 1:
        L = am.make_inputs(c, "cpu", 1)
        go, _ = am.standin_forward(*(am.heads(L[n]) for n in "qkv"), D ** -0.5)
        assert torch.equal(go, am.heads(L["v"]).expand(B, H, Tq, D))


def test_attention_forward_bounds_reject_the_mutants():
    """Each forward mutant of the stand-in fails a check.  The two truncations are caught by the rounding statistic (class c, >= 10000
    elements above 0.1 - which is why the matrix pairs class c with every form); the denominator summed from the rounded P is caught by
    the lse bound, o alone lets it pass; the missing tail mask needs class g (the clamped row Tk - 1 counted again in the denominator)."""
    from tests import attention_matrix as am
    from tests.util import STAT_LIMIT, rounding_statistic
    F = am.FwdCase
    ac, g, dc = F(2, 4, 256, 192, 64, "ac"), F(2, 4, 200, 65, 64, "g"), F(2, 4, 256, 256, 64, "dc")
    for c, ks, mutant, where in ((ac, False, "p_trunc", "o"), (ac, False, "o_trunc", "o"), (ac, False, "drop_last_key", "o"), (g, False, "no_tail_mask", "o"),
                                 (ac, False, "skip_rescale", "o"), (ac, False, "l_from_rounded_p", "lse"), (dc, True, "ks_merge_without_a1", "o"),
                                 (dc, True, "p_trunc", "o"), (dc, True, "skip_rescale", "o")):
        good, bad = _attn_fwd_check(am, c, ks), _attn_fwd_check(am, c, ks, mutant)
        assert all(isinstance(r, tuple) for r in good.values()), good
        assert isinstance(bad[where], str), f"{mutant} passed the {where} check of {c.id}: {bad}"
        print(f"[parity] attention mutant {mutant} ({c.id}): caught - {bad[where][:150]}")
    assert isinstance(_attn_fwd_check(am, ac, False, "l_from_rounded_p")["o"], tuple)          # only the lse bound sees it
    for mutant in ("p_trunc", "o_trunc"):                                                       # the statistic alone sees truncation
        L = am.make_inputs(ac, "cpu", 1)
        q, k, v = (am.heads(L[n]) for n in "qkv")
        b, cnt = rounding_statistic(am.standin_forward(q, k, v, 0.125, False, mutant)[0], am.forward_reference(q, k, v, 0.125)[0])
        assert b is not None and abs(b) > STAT_LIMIT and cnt >= 10000, (mutant, b, cnt)


_ATTN_BWD_SMALL = [("a", "n", 2, 2, 100, 100, 64, 1), ("b", "n", 2, 4, 256, 256, 64, 1), ("bc", "o", 2, 2, 200, 77, 80, 1), ("d", "n", 1, 2, 256, 256, 160, 1),
                   ("g", "n", 1, 2, 129, 65, 160, 1), ("e", "o", 1, 2, 320, 448, 64, 1), ("f", "n", 1, 2, 192, 320, 80, 1), ("b", "o", 2, 2, 192, 5, 80, 0)]


@pytest.mark.parametrize("cls,do_cls,B,H,Tq,Tk,D,dkv", _ATTN_BWD_SMALL, ids=[f"{s[0]}{s[1]}-Tq{s[4]}-Tk{s[5]}-D{s[6]}" for s in _ATTN_BWD_SMALL])
def test_attention_backward_bounds_admit_the_standin(cls, do_cls, B, H, Tq, Tk, D, dkv):
    """every input class, dO with and without an offset: the stand-in of the delta, dq and dkv kernels - handed NaN in the 64 floats behind
    lse and delta - meets every bound, no non-finite value, and the rounding statistic where bwd_takes_statistic says it applies"""
    from tests import attention_matrix as am
    from tests.util import STAT_LIMIT
    c = am.BwdCase(B, H, Tq, Tk, D, cls, do_cls, need_dkv=dkv)
    res, _ = _attn_bwd_check(am, c)
    assert all(isinstance(r, tuple) for r in res.values()), res
    print(f"[parity] attention backward stand-in {c.id}: " + ", ".join(f"{n} {w:.3f} (b = {b})" for n, (w, b) in res.items()))
    assert all(w <= 1.0 and (b is None or abs(b) <= STAT_LIMIT) for w, b in res.values())
    if (cls, do_cls) == ("b", "n"):
        assert all(res[n][1] is not None for n in ("dq", "dk", "dv")), res


def test_attention_backward_bounds_reject_the_mutants():
    """Each backward mutant fails a check - but for two that compute the same function on every valid input, which is shown instead:
      * dq_no_kv_mask: the keys past Tk of the last tile are key Tk - 1 again, p is finite there, and K^T is ZERO there (slh_transpose_heads),
        so the unmasked dS columns meet zeros in the dQ MFMA: bit-identical results.
      * no_q_tail_zero / ds_multiplied_not_selected with FINITE values behind lse and delta: Q^T and dO^T are zero for the rows past Tq.
    With NaN behind lse / delta - what recycled arena memory may hold - the last two put 0 x NaN into the dK (and dV) product of the last
    (sample, head): non-finite dK.  ds_multiplied_not_selected is attn_bwd_dkv_kernel as it was before the rows past Tq were selected."""
    from tests import attention_matrix as am
    B_ = am.BwdCase
    stat, ragged = B_(2, 4, 256, 256, 64, "b", "n"), B_(2, 2, 100, 100, 64, "a", "n")
    for c, mutant, where in ((stat, "ds_trunc", ("dq", "dk")), (ragged, "no_q_tail_zero", ("dk", "dv")), (ragged, "ds_multiplied_not_selected", ("dk",)),
                             (stat, "dk_without_scale", ("dk",)), (stat, "delta_of_next_head", ("dq", "dk"))):
        good, _ = _attn_bwd_check(am, c)
        assert all(isinstance(r, tuple) for r in good.values()), good
        bad, got = _attn_bwd_check(am, c, mutant)
        for nm in where:
            assert isinstance(bad[nm], str), f"{mutant} passed the {nm} check of {c.id}: {bad}"
        print(f"[parity] attention mutant {mutant} ({c.id}): caught - {bad[where[0]][:150]}")
        if mutant == "ds_multiplied_not_selected":
            assert not bool(torch.isfinite(got["dk"][-1, -1].float()).all()) and bool(torch.isfinite(got["dk"][0, 0].float()).all())
    eq = lambda a, b: all(torch.equal(a[n].view(torch.int16) if a[n].dtype == torch.bfloat16 else a[n], b[n].view(torch.int16) if b[n].dtype == torch.bfloat16 else b[n]) for n in a)
    for c in (B_(2, 2, 200, 77, 80, "b", "o"), ragged):
        _, honest = _attn_bwd_check(am, c, None, pad=0.0)
        assert eq(honest, _attn_bwd_check(am, c, "dq_no_kv_mask", pad=0.0)[1])
        assert eq(honest, _attn_bwd_check(am, c, "no_q_tail_zero", pad=3.0)[1])
        assert eq(honest, _attn_bwd_check(am, c, "ds_multiplied_not_selected", pad=3.0)[1])


def test_attention_backward_reference_agrees_with_autograd():
    """backward_reference is the file header's formula; on the UNROUNDED float64 forward (o, lse2) it is float64 autograd through
    softmax(scale q k^T) v, and on the bf16 o / fp32 lse2 a backward case is handed it moves by no more than what those roundings put
    into delta and P: |d delta| <= sum_d |dO| |o_r - o|, |dP| <= P expm1(ln 2 |lse_r - lse|)."""
    from tests import attention_matrix as am
    c = am.BwdCase(2, 2, 100, 77, 80, "b", "o")
    L = am.make_inputs(c, "cpu", 3)
    q, k, v, do = (am.heads(L[n]) for n in ("q", "k", "v", "do"))
    sc = am.f32(c.D ** -0.5)
    qa, ka, va = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    (torch.softmax(qa @ ka.transpose(-1, -2) * sc, -1) @ va).backward(do.double())
    o64, _, l64, _ = am.forward_reference(q, k, v, c.D ** -0.5)
    exact = am.backward_reference(q, k, v, o64, do, l64, c.D ** -0.5)
    for nm, g in (("dq", qa.grad), ("dk", ka.grad), ("dv", va.grad)):
        assert float((exact[nm][0] - g).abs().max()) <= 1e-11 * float(g.abs().max()), nm
    o_r, l_r = am.forward_for_backward(q, k, v, c.D ** -0.5)
    given = am.backward_reference(q, k, v, o_r, do, l_r, c.D ** -0.5)
    p = torch.softmax(q.double() @ k.double().transpose(-1, -2) * sc, -1)
    dpf = torch.expm1(am.LN2 * (l_r.double() - l64).abs())[..., None]                       # relative change of P
    x = (do.double() @ v.double().transpose(-1, -2) - (do.double() * o64).sum(-1, keepdim=True)).abs()
    dd = (do.double().abs() * (o_r.double() - o64).abs()).sum(-1, keepdim=True)
    e_ds = p * (1 + dpf) * dd + p * dpf * x
    assert bool(((given["dq"][0] - qa.grad).abs() <= sc * (e_ds @ k.double().abs()) * (1 + 1e-9) + 1e-12).all())
    assert bool(((given["dk"][0] - ka.grad).abs() <= sc * (e_ds.transpose(-1, -2) @ q.double().abs()) * (1 + 1e-9) + 1e-12).all())
    assert bool(((given["dv"][0] - va.grad).abs() <= ((p * dpf).transpose(-1, -2) @ do.double().abs()) * (1 + 1e-9) + 1e-12).all())
    assert float((given["dq"][0] - qa.grad).abs().max()) > 0        # the roundings are there, and accounted for


def test_attention_matrix_is_not_hollow():
    """The kernel names the library returns over the matrix are exactly the 13 forward, 3 dq and 3 dkv instantiations; the sources launch
    no instantiation this list does not name; for every name some case applies the rounding statistic to each bf16 output (asked of the
    stand-in); every Tq / Tk edge class is present; nothing in the GPU file is skipped or expected to fail."""
    from tests import attention_matrix as am
    fwd = {}
    for c in am.FWD_CASES:
        fwd.setdefault(am.fwd_name(c), []).append(c)
    assert sorted(fwd) == sorted(am.FWD_NAMES) and len(am.FWD_NAMES) == 13, set(fwd) ^ set(am.FWD_NAMES)
    dq, dkv = {}, {}
    for c in am.BWD_CASES:
        a, b = am.bwd_names(c)
        dq.setdefault(a, []).append(c)
        if c.need_dkv:
            dkv.setdefault(b, []).append(c)
        else:
            assert b == ""
    assert sorted(dq) == sorted(am.BWD_DQ_NAMES) and sorted(dkv) == sorted(am.BWD_DKV_NAMES)
    # the sources: every launch site of an attention kernel goes through slh_launch, and names one of the listed instantiations
    src = open(os.path.join(ROOT, "sliders_amd", "csrc", "attention.hip")).read()
    dts = set(re.findall(r"launch_fwd<(\d)>\(", src))
    inst = {m.replace("DT", dt) for m in re.findall(r"slh_launch<(attn_fwd\w*(?:<[^>]*>)?)>", src) for dt in dts}
    assert inst == set(am.FWD_NAMES), inst ^ set(am.FWD_NAMES)
    assert not re.search(r"hipLaunchKernelGGL\(\(?attn_fwd", src)
    srcb = open(os.path.join(ROOT, "sliders_amd", "csrc", "attention_bwd.hip")).read()
    assert set(re.findall(r"slh_launch<(attn_bwd_\w+<[^>]*>)>", srcb)) == set(am.BWD_DQ_NAMES + am.BWD_DKV_NAMES)
    assert not re.search(r"hipLaunchKernelGGL\(\(?attn_bwd", srcb)
    # the statistic is applied, per name
    for name, cases in sorted(fwd.items()):
        for c in sorted((c for c in cases if "c" in c.cls and "g" not in c.cls), key=lambda c: c.B * c.H * c.Tq * c.Tk * c.D):
            r = _attn_fwd_check(am, c, key_split=name == "attn_fwd_ks_kernel")
            assert all(isinstance(x, tuple) for x in r.values()), r
            if r["o"][1] is not None:
                break
        else:
            raise AssertionError(f"{name}: no case of the matrix applies the rounding statistic to o")
    for names, outs in ((dq, ("dq",)), (dkv, ("dk", "dv"))):
        for name, cases in sorted(names.items()):
            for c in sorted((c for c in cases if am.bwd_takes_statistic(c) and not c.chained), key=lambda c: c.Tq * c.Tk * c.D):
                r, _ = _attn_bwd_check(am, c)
                assert all(isinstance(x, tuple) for x in r.values()), r
                if all(r[o][1] is not None for o in outs):
                    break
            else:
                raise AssertionError(f"{name}: no case of the matrix applies the rounding statistic to {outs}")
    # edges
    for what, pred in am.TQ_EDGES.items():
        assert any(pred(c.Tq) for c in am.FWD_CASES), f"no forward case with Tq {what}"
    for nw in ("4", "2"):
        for t in (33, 100, 129, 200):
            assert any(c.Tq % 128 == t % 128 and f"<{nw}," in am.fwd_name(c) for c in am.FWD_CASES), (nw, t)
    assert set(am.TK_EDGES) <= {c.Tk for c in am.FWD_CASES}, set(am.TK_EDGES) - {c.Tk for c in am.FWD_CASES}
    ks = fwd["attn_fwd_ks_kernel"]
    assert {256, 384, 1024} <= {c.Tk for c in ks} and {129, 768} <= {c.Tq // 64 * c.H * c.B for c in ks} and any(c.Tq % 128 == 64 for c in ks)
    assert any(c.pack == "qkv" for c in am.FWD_CASES) and any(c.ldo_pad for c in am.FWD_CASES) and any(c.vt_extra for c in am.FWD_CASES)
    assert any(c.pf for c in ks) and any("g" in c.cls and c.Tk % 64 for c in am.FWD_CASES)
    assert {ch for c in am.FWD_CASES for ch in c.cls} == set(am.INPUT_CLASSES)
    for name in am.BWD_DQ_NAMES:
        cs = [c for c in dq[name] if not c.chained]
        assert any(c.B > 1 and c.H > 1 and c.Tq >= 1024 and c.Tk >= 1024 and c.need_dkv for c in cs), name
        assert any(c.Tq % 64 and c.need_dkv for c in cs) and any(c.Tk % 64 and not c.need_dkv for c in cs), name
        assert any(c.pack == "qkv" for c in cs) and any(c.chained for c in dq[name]), name
    assert any(c.Tk % 64 and c.need_dkv for c in am.BWD_CASES) and {"n", "o"} <= {c.do_cls for c in am.BWD_CASES}
    gpu = open(os.path.join(ROOT, "tests", "test_attention_matrix_gpu.py")).read()
    assert "skip" not in gpu and "xfail" not in gpu


# ---------------------------------------------------------------------------------------------------------------------------
# The planner's programs, byte by byte (tests/plan_digest.py)
# ---------------------------------------------------------------------------------------------------------------------------
def test_planned_programs_match_the_recorded_digests():
    """Every dry-run plan of tests/plan_digest.py's matrix - seven configurations x adapters off / on / training forward + backward in
    the default environment, SDXL 64^2 with every planner switch flipped on its own - records the command buffers, parked batch
    descriptors, lnfold items, arena allocations and tape length whose SHA-256 tests/data/plan_digests.json holds.  A refactor of the
    planner leaves the file alone; a pull request that changes a plan re-records it (python -m tests.plan_digest --write) and shows
    which plans moved; `--dump DIR` on both trees and a diff name the first op that differs."""
    from tests import plan_digest as pd
    rec = json.load(open(pd.DATA))
    got = pd.digests()
    assert sorted(got) == sorted(rec), f"plans without a record, or records without a plan: {sorted(set(got) ^ set(rec))}"
    diff = {k: (got[k], rec[k]) for k in got if got[k] != rec[k]}
    assert not diff, f"planned now / recorded: {diff}"
    assert len(got) >= 93 and os.path.getsize(pd.DATA) < 64 * 1024
    # the matrix is not hollow: every switch moves at least one plan (three of them only at 128^2: plan_digest.WIDE_SWITCHES)
    for var, val in pd.switches():
        moved = [k for k in got if k.endswith(f"|{var}={val}") and got[k]["sha256"] != got[k[:k.rindex("|")]]["sha256"]]
        assert moved, f"{var}={val} changes no plan it is flipped for"


@pytest.mark.parametrize("name,hw,method", [("sdxl", 64, "noxattn"), ("sdxl", 128, "full"), ("sd1", 64, "full")])
def test_a_refused_layernorm_fold_plans_what_no_fold_plans(monkeypatch, name, hw, method):
    """A LayerNorm fold that the tile choice refuses must leave no trace: with planner.choose_tile refusing every product that folds
    one (ln_in), the plans - adapters off / on / training forward + backward - are, byte for byte, allocation for allocation and tape
    record for tape record, the plans of a weight store without folded weights (ln_fold = False), which never tries.  Reaches the
    no-adapter refusals (no-grad and training) that no configuration of the digest matrix does."""
    from sliders_amd import planner
    from tests import plan_digest as pd
    real = planner.choose_tile
    for mode in pd.MODES:
        want = pd.record(*pd.planned((name, hw, method, mode), None, ln_fold=False))
        with monkeypatch.context() as m:
            m.setattr(planner, "choose_tile", lambda d, **kw: None if d.ln_in else real(d, **kw))
            p, bw, va, vz = pd.planned((name, hw, method, mode), None)
            got = pd.record(p, bw, va, vz)
        assert not any(d.ln_in for o, d in p.prog.ops if o == lib.OP_GEMM)
        assert got == want, mode


# ---------------------------------------------------------------------------------------------------------------------------
# LoRA helper kernels element by element (tests/lora_matrix.py, tests/test_lora_matrix_gpu.py, docs/LORA_MATRIX.md)
# ---------------------------------------------------------------------------------------------------------------------------
def _lora_check(lm, c, mutant=None, **kw):
    """{output: (worst ratio, b) or the failure text} of the stand-in of case c (mutant: with one defect) against reference and bound"""
    from tests.util import check_elementwise
    K = lm.KINDS[c.kind]
    L = K["inputs"](c, torch.device("cpu"), 1)
    got = K["standin"](c, L, mutant=mutant, **kw) if (mutant or kw) else K["standin"](c, L)
    out = {}
    for n, (r, bound) in K["reference"](c, L).items():
        try:
            if bound is None:
                assert torch.equal(got[n], r), f"{c.id} [{n}]: not bit-exact"
                out[n] = (0.0, None)
            else:
                w, _, b = check_elementwise(f"{c.id} [{n}]", got[n], r, bound)
                out[n] = (w, b)
        except AssertionError as e:
            out[n] = str(e)
    return out


def test_lora_kernel_names_and_geometry_come_from_the_library():
    """slh_skinny_kernel_name runs slh_skinny's own selection (no device, fake pointers) and refuses what slh_skinny refuses;
    slh_lora_wgrad_geometry is the one geometry function: its products are what slh_lora_wgrad_blocks / _single_blocks return."""
    from tests import lora_matrix as lm
    names = {lm.form_of(c) for c in lm.CASES if c.kind == "skinny"}
    assert names == set(lm.SKINNY_FORMS), names ^ set(lm.SKINNY_FORMS)
    d = lm.skinny_descs(lm.Case("skinny", M=5, R=4, ca=(64, 0)))[0][1]
    assert lib.skinny_kernel_name(d) == "skinny<4,64>"
    d.K = 72
    with pytest.raises(lib.SlidersHipError, match="slh_skinny"):
        lib.skinny_kernel_name(d)
    l = lib.load()
    l.slh_lora_wgrad_blocks.argtypes = [ctypes.POINTER(lib.WgradDesc)]
    for c in lm.CASES:
        if c.kind != "wgrad":
            continue
        for d in lm.wgrad_descs(c):
            for kind in (0, 1, 2):
                gx, splits, taps, rpb = lib.wgrad_geometry(d, kind)
                assert gx >= 1 and splits >= 1 and taps in (1, 9) and rpb % 8 == 0 and splits * rpb >= d.M > (splits - 1) * rpb, (c.id, kind)
                if kind == 1:
                    assert gx * splits * taps == lib.wgrad_single_blocks(d)
                else:
                    d.slabs = 8 if kind == 2 else 0
                    assert gx * splits * taps == l.slh_lora_wgrad_blocks(ctypes.byref(d))
    with pytest.raises(lib.SlidersHipError, match="kind"):
        lib.wgrad_geometry(lm.wgrad_descs(lm.CASES[-1] if lm.CASES[-1].kind == "wgrad" else next(c for c in lm.CASES if c.kind == "wgrad"))[0], 3)


def test_lora_contracts_are_refused_on_the_host():
    """vgroup_cols that the kernel would mis-address, a weight-gradient batch whose table and workspace disagree about the geometry, and
    a LayerNorm-fold item with more rows than the kernel's grid: all refused before anything is launched (no device needed)."""
    one = 0x1000

    def wg(**kw):
        base = dict(z0=one, v=one, out=one, scale=one, ldz0=192, c0=192, mode=0, stride=1, M=64, R=4, ldv=12, ldo=4, vgroup_cols=64)
        base.update(kw)
        return lib.WgradDesc(**base)

    assert lib.wgrad_single_blocks(wg()) > 0
    for what, d in {"not a multiple of 8": wg(vgroup_cols=4), "does not divide C": wg(vgroup_cols=80), "R = 12": wg(R=12, ldo=12),
                    "divides C but not by 8": wg(vgroup_cols=12), "negative": wg(vgroup_cols=-8)}.items():
        with pytest.raises(lib.SlidersHipError, match="vgroup_cols"):
            lib.wgrad_single_blocks(d)
        with pytest.raises(lib.SlidersHipError, match="vgroup_cols"):
            lib.call(lib.OP_WGRAD, d, 0)
        with pytest.raises(lib.SlidersHipError, match="vgroup_cols"):
            lib.batch_table(lib.OP_WGRAD_BATCH, [d], None, arg=d.R)
    # batched: one geometry per batch, and the workspace must match it
    with pytest.raises(lib.SlidersHipError, match="all be built with slabs or all without"):
        lib.batch_table(lib.OP_WGRAD_BATCH, [wg(slabs=8, tickets=8), wg()], None, arg=4)
    bd, _ = lib.batch_table(lib.OP_WGRAD_BATCH, [wg(M=2048), wg()], None, arg=4)            # atomic geometry ...
    bd.slabs, bd.tickets = one, one                                                        # ... but a slab workspace
    with pytest.raises(lib.SlidersHipError, match="atomic geometry"):
        lib.call(lib.OP_WGRAD_BATCH, bd, 0)
    with pytest.raises(lib.SlidersHipError, match="atomic geometry"):
        lib.Program().add(lib.OP_WGRAD_BATCH, bd)
    bd, _ = lib.batch_table(lib.OP_WGRAD_BATCH, [wg(M=2048, slabs=8, tickets=8)], None, arg=4)   # slab geometry, no workspace
    with pytest.raises(lib.SlidersHipError, match="slab geometry"):
        lib.call(lib.OP_WGRAD_BATCH, bd, 0)
    with pytest.raises(lib.SlidersHipError, match="lib.batch_table"):
        lib.call(lib.OP_WGRAD_BATCH, lib.BatchDesc(table=one, prefix=one, n=1, total=1, arg=4), 0)
    # ln_fold items
    assert lib.lnfold_item(one, one, one, one, one, one, 16, 320)[-1] == 16 | (320 << 32)
    for rows, K in ((17, 320), (0, 320), (4, 324)):
        with pytest.raises(lib.SlidersHipError, match="slh_lora_ln_fold"):
            lib.lnfold_item(one, one, one, one, one, one, rows, K)


def _lora_small(lm):
    """the cases the CPU proof walks: everything but the rows-by-the-thousand skinny cases (their 16-lane order is walked on small M)"""
    return [c for c in lm.CASES if not (c.kind == "skinny" and lm._sk_geo(c)[3] > 2000)]


def test_lora_bounds_admit_the_standins():
    """Every case of the matrix (but the skinny ones with more than 2000 rows): the stand-in - fp32 accumulation in the kernel's chunk
    and lane order, the kernel's internal roundings - meets every bound.  The 16-lanes-per-row order of skinny, which only M > 16384
    selects on the device, is walked on small M for every RMAX."""
    from tests import lora_matrix as lm
    from tests.util import STAT_LIMIT
    worst = {}
    for c in _lora_small(lm):
        res = _lora_check(lm, c)
        assert all(isinstance(r, tuple) for r in res.values()), (c.id, res)
        assert all(w <= 1.0 and (b is None or abs(b) <= STAT_LIMIT) for w, b in res.values())
        f = lm.form_of(c)
        worst[f] = max(worst.get(f, 0.0), max(w for w, _ in res.values()))
    for c in lm.CASES:
        if c.kind == "skinny" and not c.kmajor and c.conv is None and lm._sk_geo(c)[3] <= 2000:
            res = _lora_check(lm, c, lpr=16, rmax=4 if c.R <= 4 else 12 if c.R <= 12 else 16)
            assert all(isinstance(r, tuple) for r in res.values()), (c.id, res)
    for f, w in sorted(worst.items()):
        print(f"[parity] lora stand-in {f}: worst |got - ref| / bound = {w:.3f}")


def test_lora_bounds_reject_the_mutants():
    """Each mutant of a stand-in leaves the bound of the case lora_matrix.mutant_cases() names for it - a case of the GPU list - and the
    honest stand-in of that same case passes.  Two remarks on reach, also in docs/LORA_MATRIX.md: a weight gradient that masks its taps
    as if the stride were 1 computes the same function at stride 2 on EVEN image sizes (no window leaves the image at the far edge),
    so only the odd sizes catch it; conv_dgrad without its oy >= ho check computes the same function at stride 2 on ODD sizes (the
    parity check already removes the row), so stride 1 and the even sizes catch it - and only with a sample behind the one that
    over-reads."""
    from tests import lora_matrix as lm
    cases = lm.mutant_cases()
    assert set(cases) == {f"{k}/{m}" for k, ms in lm.MUTANTS.items() for m in ms}
    for key, c in cases.items():
        kind, mutant = key.split("/")
        assert c.kind == kind and c in lm.CASES
        good, bad = _lora_check(lm, c), _lora_check(lm, c, mutant)
        assert all(isinstance(r, tuple) for r in good.values()), (key, good)
        caught = [r for r in bad.values() if isinstance(r, str)]
        assert caught, f"{key} passed every check of {c.id}: {bad}"
        print(f"[parity] lora mutant {key} ({c.id}): caught - {caught[0][:150]}")
    # the equivalences claimed above
    even = next(c for c in lm.CASES if c.kind == "wgrad" and len(c.probs) == 1 and c.probs[0]["conv"] == (2, 8, 6) and c.probs[0]["stride"] == 2 and c.probs[0]["xform"] == 0)
    L = lm.wgrad_inputs(even, torch.device("cpu"), 1)
    a, b = lm.wgrad_standin(even, L), lm.wgrad_standin(even, L, "taps_as_stride1")
    assert all(torch.equal(a[n], b[n]) for n in a)
    odd = next(c for c in lm.CASES if c.kind == "cdgrad" and c.stride == 2 and (c.hl, c.wl) == (7, 5) and c.B == 3)
    L = lm.cdgrad_inputs(odd, torch.device("cpu"), 1)
    assert torch.equal(lm.cdgrad_standin(odd, L)["gx"], lm.cdgrad_standin(odd, L, "no_oy_check")["gx"])


def test_lora_matrix_is_not_hollow():
    """Every form has a case; every edge the matrix claims is in the list, asked of the library where the library decides it."""
    from tests import lora_matrix as lm
    ids = [c.id for c in lm.CASES]
    assert len(ids) == len(set(ids))
    forms = {}
    for c in lm.CASES:
        forms.setdefault(lm.form_of(c), []).append(c)
    assert set(forms) == set(lm.FORMS), set(forms) ^ set(lm.FORMS)
    sk = [c for c in lm.CASES if c.kind == "skinny"]
    rows = lambda c: lm._sk_geo(c)[3]
    assert {c.R for c in sk if not c.conv and not c.kmajor} >= {1, 3, 4, 5, 8, 12, 13, 16}
    assert {lm._sk_geo(c)[1] for c in sk if not c.conv} >= {8, 64, 320, 512, 520, 136} and {rows(c) for c in sk} >= {1, 5, 333, 16384, 16385, 16391}
    # the switch between the two lane forms lies between the two neighbouring row counts of the list - wherever the library puts it
    assert lm.form_of(next(c for c in sk if rows(c) == 16384)) == "skinny<4,64>" and lm.form_of(next(c for c in sk if rows(c) == 16385)) == "skinny<4,16>"
    for f in lm.SKINNY_FORMS:                                  # every instantiation also with masked rows (R < RMAX)
        assert any(c.R < int(f[7:].split(",")[0]) for c in forms[f]), f
    assert any(c.conv and rows(c) > 16384 and c.ca == (8, 0) for c in sk) and any(c.kmajor and rows(c) > 16384 for c in sk)
    assert {(c.stride, c.xform) for c in sk if c.conv} >= {(s, x) for s in (1, 2) for x in (0, 1, 2)}
    assert {c.out_kind for c in sk if c.conv} == {0, 1} and any(c.ca[1] and c.conv for c in sk) and any(c.ca[1] and not c.conv for c in sk)
    gv = [c for c in lm.CASES if c.kind == "gemv"]
    for opt, vals in dict(nb=(1, 2, 7, 8), N=(1, 5, 37), K=(8, 320, 512, 520, 1280), in_act=(0, 1), out_f32=(0, 1), bias=(0, 1), addend=(0, 1), lora=(0, 1),
                          tcol=(0, 1)).items():
        assert {getattr(c, opt) for c in gv} >= set(vals), opt
    assert any(c.pad for c in gv)
    wgs = [c for c in lm.CASES if c.kind == "wgrad"]
    for form in ("atomic", "slab", "batch", "batch_slab"):
        sub = [c for c in wgs if c.form == form]
        dense = [(c, p, g) for c in sub for p, g in zip(c.probs, lm.wgrad_geometry(c)) if not p["conv"]]
        assert {p["M"] for _, p, _ in dense} >= {1, 7, 64, 65, 512, 513, 1024, 1025} or form != "atomic"
        assert {p["M"] for _, p, _ in dense} >= {512, 513, 1024, 1025}, form
        assert any(g[1] == 1 for _, _, g in dense) and any(g[1] > 1 for _, _, g in dense), form       # with and without an M split
        assert any(p["vg"] for c in sub for p in c.probs) and any(p["c"][1] for c in sub for p in c.probs) and any(p["conv"] for c in sub for p in c.probs), form
        assert {c.R for c in sub} == {4, 12} and {p["rmajor"] for c in sub for p in c.probs} == {0, 1}
    k2 = {p["M"]: g[1] for c in wgs if c.form == "batch_slab" for p, g in zip(c.probs, lm.wgrad_geometry(c)) if not p["conv"]}
    assert k2[512] != k2[513], "the kind-2 split edge moved away from 512 / 513: move the cases with it"
    k1 = {p["M"]: g[1] for c in wgs if c.form == "slab" for p, g in zip(c.probs, lm.wgrad_geometry(c)) if not p["conv"] and p["c"] == (264, 0)}
    assert k1[1024] != k1[1025], "the min_splits edge moved away from 1024 / 1025: move the cases with it"
    assert {p["M"] for c in wgs for p in c.probs if not p["conv"]} >= {1, 7, 64, 65}
    assert {p["c"][0] + p["c"][1] for c in wgs for p in c.probs} >= {8, 64, 264, 320, 192}
    assert {(p["stride"], p["xform"], p["conv"][1:]) for c in wgs for p in c.probs if p["conv"]} >= {(s, x, hw) for s in (1, 2) for x in (0, 1, 2) for hw in ((7, 5), (8, 6))}
    assert any(len(c.probs) > 1 and {bool(p["conv"]) for p in c.probs} == {True, False} and any(p["vg"] for p in c.probs) and any(p["c"][1] for p in c.probs) for c in wgs)
    cd = [c for c in lm.CASES if c.kind == "cdgrad"]
    assert {(c.stride, c.hl, c.wl) for c in cd} >= {(s, h, w) for s in (1, 2) for h, w in ((7, 5), (8, 6), (1, 1))}
    assert {c.cin for c in cd} >= {8, 64, 72} and {c.B for c in cd} == {1, 3} and {c.acc for c in cd} == {0, 1} and {c.ldu for c in cd} == {4, 12}
    assert any(c.ucol for c in cd) and any(c.pad for c in cd) and any((c.B * c.hl * c.wl * c.cin // 8) % 256 for c in cd)
    assert {(c.C, c.ted) for c in lm.CASES if c.kind == "temb"} == {(320, 1280), (100, 104), (8, 8)}
    ln = [c for c in lm.CASES if c.kind == "lnfold"]
    assert {c.K for c in ln} >= {8, 320, 2048, 2056} and {len(c.rows) for c in ln} >= {1, 3} and {r for c in ln for r in c.rows} >= {1, 4, 12, 16}
    ew = [c for c in lm.CASES if c.kind == "ew"]
    for op in ("copy", "add", "add_inplace"):
        assert {c.C for c in ew if c.op == op} >= {8, 72} and all((c.M * c.C // 8) % 256 for c in ew if c.op == op) and all(len(set(c.pads)) == 3 for c in ew if c.op == op)
    assert {c.geo for c in ew if c.op == "upsample"} == {(2, 3, 5), (2, 6, 10)}
    cs = [c for c in ew if c.op == "colsum"]
    assert {c.geo[1] for c in cs} >= {1, 7, 512, 513, 1030} and {c.C for c in cs} == {8, 264} and {c.geo[0] for c in cs} == {1, 3}
    assert {lm.has_atomics(c) for c in cs} == {True, False}
    for key, c in lm.mutant_cases().items():
        assert c in lm.CASES, key


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 image-path kernels element by element (tests/vae_matrix.py, tests/test_vae_matrix_gpu.py, docs/VAE_MATRIX.md)
# ---------------------------------------------------------------------------------------------------------------------------
def _vae_check(vm, c, mutant=None):
    """{label: (worst ratio, b) or the failure text} of the stand-in of case c (mutant: with one defect) against reference and bound"""
    from tests.util import check_elementwise
    K = vm.KINDS[c.kind]
    L = K["inputs"](c, torch.device("cpu"), 1)
    got = K["standin"](c, L, mutant=mutant)
    out = {}
    for label, (buf, r, bound) in K["reference"](c, L, got).items():
        try:
            if bound is None:
                assert torch.equal(got[buf], r), f"{c.id} [{label}]: not bit-exact"
                out[label] = (0.0, None)
            else:
                w, _, b = check_elementwise(f"{c.id} [{label}]", got[buf], r, bound)
                out[label] = (w, b)
        except AssertionError as e:
            out[label] = str(e)
    return out


def test_sgemm_form_comes_from_the_library_and_bad_descriptors_are_refused():
    """slh_sgemm_form runs slh_sgemm's own checks and selection (no device, fake pointers).  Refused on the host, before any launch:
    split_bf16 outside {0, 1} (the former profiling bits), upsample with stride 2 or in dense mode, and a conv output size that does not
    follow from the source, stride, pad and upsample.  The encoder's and decoder's calls pass."""
    one = 0x1000

    def conv(**kw):
        base = dict(x=one, w=one, c=one, ldx=32, ldw=288, ldc=8, M=2 * 8 * 6, N=8, K=288, mode=1, cin=32, batch=2, hs=8, ws=6, ho=8, wo=6, stride=1,
                    pad=1, alpha=1.0, split_bf16=1)
        base.update(kw)
        return lib.SgemmDesc(**base)

    def dense(**kw):
        base = dict(x=one, w=one, c=one, ldx=64, ldw=64, ldc=8, M=100, N=8, K=64, mode=0, alpha=1.0, split_bf16=1)
        base.update(kw)
        return lib.SgemmDesc(**base)

    assert lib.sgemm_form(conv()) == "split<64>" and lib.sgemm_form(dense()) == "split<64>" and lib.sgemm_form(dense(split_bf16=0)) == "exact"
    assert lib.sgemm_form(dense(M=32768)) == "split<128>"
    # what sliders_amd/vae.py records: 3 x 3 pad 1, the downsampler (stride 2, pad 0, (h - 2) // 2 + 1), the upsampler (ho = 2 hs)
    for h in (64, 33, 8):
        assert lib.sgemm_form(conv(hs=h, ws=h, ho=h, wo=h, M=2 * h * h))
        ho = (h - 2) // 2 + 1
        assert lib.sgemm_form(conv(hs=h, ws=h, ho=ho, wo=ho, M=2 * ho * ho, stride=2, pad=0))
        assert lib.sgemm_form(conv(hs=h, ws=h, ho=2 * h, wo=2 * h, M=8 * h * h, upsample=1))
    bad = {
        "split_bf16": [dense(split_bf16=3), dense(split_bf16=5), dense(split_bf16=9), dense(split_bf16=2), conv(split_bf16=-1)],
        "upsample": [conv(upsample=1, stride=2, ho=8, wo=6), conv(upsample=2, ho=16, wo=12, M=2 * 16 * 12), dense(upsample=1)],
        "does not follow": [conv(ho=7, wo=6, M=2 * 7 * 6), conv(upsample=1), conv(stride=2, pad=0, ho=8, wo=6), conv(stride=2, pad=0, ho=3, wo=3, M=18),
                            conv(pad=0), conv(hs=1, ws=1, ho=1, wo=1, M=2, pad=0), conv(batch=0, M=0)],
    }
    for what, ds in bad.items():
        for d in ds:
            with pytest.raises(lib.SlidersHipError, match="slh_sgemm"):
                lib.sgemm_form(d)
            # the pointers are made up: lib.call below is safe only because slh_sgemm refuses d before any launch, which the assertion
            # above has just established with the same checks (slh_sgemm_form runs slh_sgemm).  Keep this order.
            if d.M > 0:
                with pytest.raises(lib.SlidersHipError, match=what):
                    lib.call(lib.OP_SGEMM, d, 0)
    assert lib.sgemm_form(conv(stride=2, pad=0, ho=4, wo=3, M=24)) == "split<64>"


def test_vae_launches_too_large_for_one_grid_are_refused():
    """A launch of csrc/vae.hip that would need 2^31 workgroups or more is refused on the host, in the entry point's name, instead of
    wrapping its grid (launch_grid, csrc/common.h).  The pointers are made up and nothing is launched: every call below is refused.
    The flat entry points have no query mode, so only their refusals are asserted; slh_sgemm has one (slh_sgemm_form), and there the
    largest tile product below 2^31 with the same M is shown to pass.  slh_vae_moments (a workgroup per four pixels) and slh_vae_conv_in
    index their pixels in int, so 2^31 pixels and more are refused before the grid is sized - 2^33 pixels would not fit it either."""
    one, grid = 0x1000, "too large for one launch"
    conv = dict(x=one, w=one, bias=one, qw=one, qb=one, y=one)
    flat = [
        ("slh_vae_sample", lib.OP_VAE_SAMPLE, lib.VaeSampleDesc(moments=one, post_noise=one, noise=one, noisy_f32=one, batch=1 << 20, hw=1 << 18), grid),
        ("slh_vae_post_quant", lib.OP_VAE_POST_QUANT, lib.VaeConvDesc(**conv, batch=1 << 9, h=1 << 15, wd=1 << 15, cin=0), grid),       # 2^39 threads
        ("slh_vae_conv_in", lib.OP_VAE_CONV_IN, lib.VaeConvDesc(**conv, batch=1 << 10, h=1 << 10, wd=1 << 10, cin=3, cout=1 << 11), grid),  # 2^30 px x 2^9
        ("slh_vae_conv_in", lib.OP_VAE_CONV_IN, lib.VaeConvDesc(**conv, batch=2, h=1 << 15, wd=1 << 15, cin=3, cout=4), "pixels"),
        ("slh_vae_moments", lib.OP_VAE_MOMENTS, lib.VaeConvDesc(**conv, batch=8, h=1 << 15, wd=1 << 15, cin=4), "pixels"),              # 2^33 pixels
        ("slh_gn32_apply", lib.OP_GN32_APPLY, lib.Gn32Desc(x=one, gamma=one, beta=one, stats=one, y=one, ldx=1024, ldy=1024, C=1024, batch=1 << 10,
                                                           hw=1 << 21, groups=32), grid),                                                # 2^39 threads
    ]
    for name, op, d, what in flat:
        with pytest.raises(lib.SlidersHipError, match=f"{name}: .*{what}"):
            lib.call(op, d, 0)
    # slh_sgemm, exact form (split_bf16 = 0): 2^16 x 2^15 tiles of 128 x 128 are 2^31 workgroups; one tile column less fits
    big = dict(x=one, w=one, c=one, ldx=16, ldw=16, ldc=1 << 22, M=1 << 23, K=16, mode=0, alpha=1.0, split_bf16=0)
    with pytest.raises(lib.SlidersHipError, match=f"slh_sgemm: .*{grid}"):
        lib.sgemm_form(lib.SgemmDesc(**big, N=1 << 22))
    assert lib.sgemm_form(lib.SgemmDesc(**big, N=(1 << 22) - 128)) == "exact"
    with pytest.raises(lib.SlidersHipError, match=f"slh_sgemm: .*{grid}"):          # and in int the product of 2^24 x 2^24 tiles was 0
        lib.sgemm_form(lib.SgemmDesc(**dict(big, M=(1 << 31) - 1, N=(1 << 31) - 4, ldc=(1 << 31) - 4)))


def test_vae_bounds_admit_the_standins():
    """Every case of the matrix: the stand-in - fp32 arithmetic, for the split form the explicit bf16 halves - meets every bound; the
    evaluated dropped-product term of every split case stays below 3 * 2^-18 |alpha| sum |x||w| (the figure for operands spread over
    their binades) - the bound asks no less than that; the sample case that takes the rounding statistic has the elements for it."""
    from tests import vae_matrix as vm
    from tests.util import STAT_LIMIT, STAT_MIN_ABS, STAT_MIN_COUNT
    worst, split_ratio = {}, 0.0
    for c in vm.CASES:
        res = _vae_check(vm, c)
        assert all(isinstance(r, tuple) for r in res.values()), (c.id, res)
        assert all(w <= 1.0 and (b is None or abs(b) <= STAT_LIMIT) for w, b in res.values())
        for label, (w, _) in res.items():
            f = vm.form_of(c, label)
            worst[f] = max(worst.get(f, 0.0), w)
        if c.kind == "sgemm" and vm.sgemm_form(c) != "exact":
            extra, spread = vm.sgemm_split_terms(c, vm.sgemm_inputs(c, torch.device("cpu"), 1))
            r = float((extra / spread).max())
            assert r <= 1.0, (c.id, r)
            split_ratio = max(split_ratio, r)
    assert set(worst) == set(vm.FORMS)
    for f, w in sorted(worst.items()):
        print(f"[parity] vae stand-in {f}: worst |got - ref| / bound = {w:.3f}")
    print(f"[parity] vae split forms: dropped-product term at most {split_ratio:.3f} x 3 * 2^-18 |alpha| sum |x||w|")
    big = vm._find("sample", B=2, hw=2500)
    ref = vm.sample_reference(big, vm.sample_inputs(big, torch.device("cpu"), 1))["noisy_bf16"][1]
    assert ref.numel() == 20000 and int((ref.abs() > STAT_MIN_ABS).sum()) >= STAT_MIN_COUNT
    res = _vae_check(vm, big)
    assert res["noisy_bf16"][1] is not None and res["noisy_bf16 == bf16(noisy_f32)"] == (0.0, None)


def test_vae_bounds_reject_the_mutants():
    """Each mutant of a stand-in leaves the bound of the case vae_matrix.mutant_cases() names for it - a case of the GPU list - and the
    honest stand-in of that same case passes.  Remarks on reach, also in docs/VAE_MATRIX.md: a split kernel that skips its last K step
    when nk % 3 == 1 computes the same function at nk = 2, 3, 5 (shown); a conv that checks its taps against hs instead of hs << 1
    computes the same function without upsample (shown); a softmax that sums only its first 1024 columns is the same function up to
    cols = 1024 (shown)."""
    from tests import vae_matrix as vm
    cases = vm.mutant_cases()
    assert set(cases) == {f"{k}/{m}" for k, ms in vm.MUTANTS.items() for m in ms}
    for key, c in cases.items():
        kind, mutant = key.split("/")
        assert c.kind == kind and c in vm.CASES
        good, bad = _vae_check(vm, c), _vae_check(vm, c, mutant)
        assert all(isinstance(r, tuple) for r in good.values()), (key, good)
        caught = [r for r in bad.values() if isinstance(r, str)]
        assert caught, f"{key} passed every check of {c.id}: {bad}"
        print(f"[parity] vae mutant {key} ({c.id}): caught - {caught[0][:150]}")
    # a wrong statistic fails the statistics check, not the apply check (y is referred to the kernel's own statistics), and vice versa
    bad = _vae_check(vm, cases["gn32/first_cluster_only"], "first_cluster_only")
    assert isinstance(bad["stats"], str) and isinstance(bad["y"], tuple)
    # the equivalences claimed above
    cpu = torch.device("cpu")
    for c in vm.CASES:
        if c.kind == "sgemm" and vm.sgemm_form(c) != "exact" and (vm._sg_geo(c)[4] // 32) % 3 != 1 and vm._sg_geo(c)[2] < 2000:
            L = vm.sgemm_inputs(c, cpu, 1)
            assert torch.equal(vm.sgemm_standin(c, L)["c"], vm.sgemm_standin(c, L, "split_skips_last_step_nk_mod3_1")["c"]), c.id
    c = vm._find("sgemm", conv=(3, 7, 5), stride=1, pad=1, up=0, split=0)
    L = vm.sgemm_inputs(c, cpu, 1)
    assert torch.equal(vm.sgemm_standin(c, L)["c"], vm.sgemm_standin(c, L, "upsample_bounds_hs")["c"])
    # stride 2 / pad 0 on the odd image: no window reaches row hs (ho = 3, the last row read is 6), so the unmasked bottom tap is the same
    # function there; and with ho == hs (stride 1 / pad 1) so is the sample offset taken from ho
    c = vm._find("sgemm", conv=(3, 7, 5), stride=2, pad=0, cin=32, split=1)
    L = vm.sgemm_inputs(c, cpu, 1)
    assert torch.equal(vm.sgemm_standin(c, L)["c"], vm.sgemm_standin(c, L, "bottom_tap_unmasked_stride2")["c"])
    c = vm._find("sgemm", conv=(3, 8, 6), stride=1, pad=1, cin=32, split=1)
    L = vm.sgemm_inputs(c, cpu, 1)
    assert torch.equal(vm.sgemm_standin(c, L)["c"], vm.sgemm_standin(c, L, "sample_offset_uses_ho")["c"])
    for key in ("sgemm/sample_offset_uses_ho", "sgemm/bottom_tap_unmasked_stride2"):
        assert vm.sgemm_form(cases[key]) == "split<64>" and cases[key].conv[0] == 3
    c = vm._find("softmax", cols=1024, cls="n")
    L = vm.softmax_inputs(c, cpu, 1)
    assert torch.equal(vm.softmax_standin(c, L)["x"], vm.softmax_standin(c, L, "sum_first_1024")["x"])


def test_vae_matrix_is_not_hollow():
    """Every form has a case; every edge the matrix claims is in the list, asked of the library where the library decides it."""
    from tests import vae_matrix as vm
    ids = [c.id for c in vm.CASES]
    assert len(ids) == len(set(ids))
    forms = {}
    for c in vm.CASES:
        for label in (("stats", "y") if c.kind == "gn32" else ("",)):
            forms.setdefault(vm.form_of(c, label), []).append(c)
    assert set(forms) == set(vm.FORMS), set(forms) ^ set(vm.FORMS)
    sg = [c for c in vm.CASES if c.kind == "sgemm"]
    form, geo = vm.sgemm_form, vm._sg_geo
    dense, conv = [c for c in sg if not c.conv], [c for c in sg if c.conv]
    # dense: every M, N, K in both requests; the split form at nk = 1 .. 5 and 7; K = 16, 48 fall back - as the library says
    for split in (0, 1):
        sub = [c for c in dense if c.split == split]
        assert {c.M for c in sub} >= {1, 63, 64, 65, 127, 128, 129, 300} and {c.N for c in sub} >= {4, 124, 128, 132, 260}
        assert {c.K for c in sub} >= {16, 32, 48, 64, 96, 128, 160, 224}
    assert all(form(c) == "exact" for c in dense if c.split == 0)
    assert {c.K // 32 for c in dense if form(c) == "split<64>"} >= {1, 2, 3, 4, 5, 7}
    assert {c.K for c in dense if c.split == 1 and form(c) == "exact"} == {16, 48}, "the K % 32 edge moved: move the cases with it"
    assert all(form(c) != "exact" for c in dense if c.split == 1 and c.K % 32 == 0)
    for f in ("exact", "split<64>"):
        sub = [c for c in dense if form(c) == f]
        assert {c.alpha for c in sub} == {1.0, 0.37} and {c.bias for c in sub} == {0, 1, 2} and {c.res for c in sub} == {0, 1}, f
        assert all(any(c.pads[i] for c in sub) for i in range(4)) and any(c.res and c.pads[2] for c in sub), f
    # conv: images, stride / pad pairs, cin, Cout, batch, residual; cin = 16, 48 fall back - as the library says
    pairs = {(c.stride, c.pad) for c in conv if not c.up}
    assert pairs == {(1, 1), (2, 0), (1, 0), (2, 1)}
    for sp in pairs:
        assert {c.conv[1:] for c in conv if (c.stride, c.pad) == sp and not c.up} >= {(7, 5), (8, 6)}, sp
    assert {(c.stride, c.pad) for c in conv if c.conv[1:] == (1, 1) and not c.up} == {(1, 1), (2, 1)}
    assert {c.cin for c in conv if c.split == 1 and form(c) == "exact"} == {16, 48}, "the cin % 32 edge moved: move the cases with it"
    assert {c.cin for c in conv if form(c) == "split<64>"} >= {32, 64} and {c.cin for c in conv if c.split == 0} >= {32, 64}
    assert {c.N for c in conv} >= {4, 132}
    # batch and residual per kernel form (as the library reports it) and per stride / pad pair: a second sample behind the image is what
    # shows a tap that escapes its mask or a wrong sample offset - in the split kernel's load_x as much as in the exact kernel's
    for f in ("exact", "split<64>"):
        for sp in pairs:
            sub = [c for c in conv if form(c) == f and (c.stride, c.pad) == sp and not c.up]
            assert {c.conv[0] for c in sub} >= {1, 3} and {c.res for c in sub} == {0, 1}, (f, sp)
            assert {c.conv[1:] for c in sub if c.conv[0] == 3} >= {(7, 5), (8, 6)}, (f, sp)
    ups = [c for c in conv if c.up]
    assert {form(c) for c in ups} >= {"exact", "split<64>", "split<128>"} and {c.conv[1:] for c in ups} >= {(7, 5), (1, 1)}
    assert all(c.stride == 1 and c.pad == 1 and geo(c)[5] == 2 * c.conv[1] for c in ups) and any(c.conv[0] == 3 for c in ups)
    # the 128-row form: either side of the tile-count threshold, wherever the library puts it
    lo, hi = vm._find("sgemm", M=32640, N=4, K=32), vm._find("sgemm", M=32763, N=4, K=32)
    assert (form(lo), form(hi)) == ("split<64>", "split<128>"), "the 255 / 256 tile edge moved: move the cases with it"
    big = [c for c in sg if form(c) == "split<128>"]
    assert any(c.conv and not c.up for c in big) and any(c.up for c in big) and any(not c.conv and c.N == 132 and c.K == 96 for c in big)
    # gn32
    gn = [c for c in vm.CASES if c.kind == "gn32"]
    assert {(c.C, c.groups) for c in gn} == {(32, 8), (128, 32), (256, 32), (256, 64), (512, 32), (1024, 32)}
    for C, g in {(c.C, c.groups) for c in gn}:
        sub = [c for c in gn if (c.C, c.groups) == (C, g)]
        assert {c.hw for c in sub} >= {1, 63, 64, 65, 1024, 1025, 1093} and {c.B for c in sub} == {1, 3} and {c.act for c in sub} == {0, 1}, (C, g)
        assert {c.off for c in sub} == {0.5, 300.0} and any(c.pads[0] and c.pads[1] for c in sub), (C, g)
    clusters = lambda hw: lib.gn32_workspace(hw)[1] - 1
    assert clusters(1024) == 1 and clusters(1025) == 2, "the one / two cluster edge moved away from 1024 / 1025: move the cases with it"
    assert clusters(1093) == 2 and clusters(1) == 1
    sm = [c for c in vm.CASES if c.kind == "softmax"]
    for cls in "ns":
        assert {(c.rows, c.cols, c.ld) for c in sm if c.cls == cls} == {(1, 4, 4), (3, 1024, 1024), (3, 1028, 1040), (5, 4096, 4096)}
    ci = [c for c in vm.CASES if c.kind == "conv_in"]
    assert {(c.cin, c.cout, c.geo) for c in ci} == {(a, b, g) for a in (3, 4) for b in (4, 128) for g in ((1, 1, 1), (2, 3, 5), (3, 9, 7))}
    mo = [c for c in vm.CASES if c.kind == "moments"]
    assert {c.C for c in mo} == {4, 128, 256, 260, 512} and {c.geo for c in mo} == {(1, 1, 1), (2, 3, 5), (3, 3, 3)}
    assert len(mo) == 15 and any((c.geo[0] * c.geo[1] * c.geo[2]) % 4 for c in mo)
    sa = [c for c in vm.CASES if c.kind == "sample"]
    assert {c.hw for c in sa} == {1, 15, 300, 2500} and {c.B for c in sa} == {1, 2} and len({c.outs for c in sa}) == 7
    L = vm.sample_inputs(sa[0].__class__("sample", B=2, hw=15), torch.device("cpu"), 1)
    assert {float(v) for v in L["moments"][:, 4:].reshape(-1)[::5][:4]} == {-40.0, -30.0, 20.0, 25.0}
    pq = [c for c in vm.CASES if c.kind == "post_quant"]
    for zbf in (0, 1):
        assert {c.hw for c in pq if c.zbf == zbf} == {1, 15, 300} and {c.B for c in pq if c.zbf == zbf} == {1, 3}
    for key, c in vm.mutant_cases().items():
        assert c in vm.CASES, key
