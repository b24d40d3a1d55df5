"""Digests of the planner's dry-run programs: what sliders_amd/planner.py records is pinned byte by byte.

The planner runs on the CPU against virtual arenas, so a plan is a pure function of (configuration, shape, mode, environment) once
every pointer it is handed is a pure function of what it names.  plan() builds one plan (and, for "train", its BackwardPlan) against
such stand-ins and record() reduces it to {ops, sha256, high_water}.  The SHA-256 covers, in this order:
  * every op of plan.prog - name, opcode and the descriptor bytes of the command buffer itself,
  * plan.prog_text_cached where it exists, the BackwardPlan's program for "train",
  * the descriptors parked for the batched launches (_tr_batch / _wg_batch: a dry run does not pack them into a device table),
  * lnfold_items, the (start, end, name) allocation lists of both arenas (they carry the allocation order) and the tape length.
LoraLnFoldDesc.items is the address of a host tensor made while planning: it is zeroed, its contents are lnfold_items.

matrix() is the fixed list of cases; tests/test_host.py re-plans it and compares with tests/data/plan_digests.json
(`python -m tests.plan_digest --write` records the file - only when a change of the programs is the point of the pull request;
`--dump DIR` writes one text line per op, so that two trees are compared with a plain diff instead of two hashes).
"""
import ctypes
import dataclasses
import hashlib
import json
import os
import sys
import zlib
from typing import Dict, Iterator, List, Optional, Tuple

from sliders_amd import lib, planner
from sliders_amd.arena import Arena
from sliders_amd.config import CONFIGS
from sliders_amd.lora_store import LoraStore
from sliders_amd.modules import build_tree
from sliders_amd.planner import BackwardPlan, UNetPlan
from sliders_amd.unet import _VirtualLora

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "plan_digests.json")

B, CTX, GRAD_SAMPLE = 2, 77, (1, 1)
MODES = ("off", "on", "train")
SCALE_PTR, ONE_PTR = 0x10, 0x20


class Weights:
    """Weight stand-in whose addresses are a function of the tensor NAME (256-byte aligned): a plan that asks for one more name - the
    `.lnw` of a fold it then refuses - moves no other pointer.  Carries WeightStore's batched text K/V layout (all attn2 K / V
    projections concatenated), so that kv_all, the fused cross-attention and prog_text_cached are reached."""

    def __init__(self, cfg, ln_fold: bool = True):
        self.temb_offsets, self.resnet_paths, off = {}, [], 0
        widths = {}
        for n, m in build_tree(cfg).named_modules():
            if m.cls == "ResnetBlock2D":
                self.resnet_paths.append(n)
                self.temb_offsets[n] = off
                off += m.out_dim
            if n.endswith(".attn2.to_k"):
                widths[n[:-len(".to_k")]] = m.out_dim
        self.temb_total = off
        self.packed = True
        self.ln_fold = ln_fold
        self.geglu16 = True
        self.kv_all_vbase = sum(widths.values())
        self.kv_all_offset, row = {}, 0
        for a, wd in widths.items():
            self.kv_all_offset[a] = (row, self.kv_all_vbase + row)
            row += wd
        self.gemm_shape = {"attn2_kv_all.w": (2 * self.kv_all_vbase, cfg.cross_attention_dim)}

    def ptr(self, name):
        return 0x10000000 + 0x100 * zlib.crc32(name.encode())

    def has(self, name):
        return True


class Lora(_VirtualLora):
    """The sizing run's adapter stand-in with one address per entry instead of 0x2000 for all of them (which would hide a wrong
    entry): parameters at P + 2 * offset (bf16), gradients at G + 4 * offset (fp32)."""
    P, G = 0x400000000, 0x800000000

    def down_ptr(self, e):
        return self.P + 2 * e.down_off

    def up_ptr(self, e):
        return self.P + 2 * e.up_off

    def gdown_ptr(self, e):
        return self.G + 4 * e.down_off

    def gup_ptr(self, e):
        return self.G + 4 * e.up_off


_STORES: Dict[Tuple[str, str], LoraStore] = {}


def _store(name: str, method: str) -> LoraStore:
    key = (name, method)
    if key not in _STORES:
        _STORES[key] = LoraStore(CONFIGS[name](), train_method=method, init="none")
    return _STORES[key]


def plan(name: str, hw: int, method: str, mode: str, ln_fold: bool = True):
    """(forward plan, backward plan or None, activation arena, zero arena) of one dry run"""
    cfg = CONFIGS[name]()
    va, vz = Arena(1 << 50, None), Arena(1 << 40, None)
    lora = Lora(_store(name, method)) if mode != "off" else None
    p = UNetPlan(cfg, Weights(cfg, ln_fold), va, vz, B, hw, hw, CTX, lora, mode, SCALE_PTR)
    bw = BackwardPlan(p, *GRAD_SAMPLE, ONE_PTR) if mode == "train" else None
    return p, bw, va, vz


def _op_lines(prog) -> Iterator[str]:
    """One line per op of a Program: index, name, opcode, descriptor bytes (hex) as they stand in the command buffer"""
    assert len(prog._chunks) == len(prog.ops) == len(prog.op_names) == prog.n_ops
    for i, (chunk, (opcode, d), nm) in enumerate(zip(prog._chunks, prog.ops, prog.op_names)):
        op, n = (ctypes.c_int32 * 2).from_buffer_copy(chunk[:8])
        raw = chunk[8:8 + n]
        assert op == opcode and raw == bytes(d), f"op {i} {nm}: the command buffer and the kept descriptor differ"
        if opcode == lib.OP_LORA_LN_FOLD:
            q = type(d).from_buffer_copy(d)
            q.items = 0
            raw = bytes(q)
        yield f"{i} {nm} {opcode} {raw.hex()}"


def lines(p, bw, va, vz) -> List[str]:
    """Everything the digest covers, as text"""
    out = ["# prog"] + list(_op_lines(p.prog))
    if getattr(p, "prog_text_cached", None) is not None:
        out += ["# prog_text_cached"] + list(_op_lines(p.prog_text_cached))
    if bw is not None:
        out += ["# backward"] + list(_op_lines(bw.prog))
        out += ["# backward transposes parked for the batched launch"] + [f"{i} {bytes(d).hex()}" for i, d in enumerate(bw._tr_batch)]
        for R, descs in sorted(bw._wg_batch.items()):
            out += [f"# backward weight gradients parked for the batched launch, R = {R}"] + [f"{i} {bytes(d).hex()}" for i, d in enumerate(descs)]
    out += ["# lnfold_items"] + [" ".join(str(int(v)) for v in it) for it in p.lnfold_items]
    for title, a in (("arena", va), ("zero arena", vz)):
        out += [f"# {title} allocations"] + [f"{s} {e} {nm}" for s, e, nm in a.allocs]
    out += [f"# tape {len(p.tape)}"]
    return out


def record(p, bw, va, vz) -> dict:
    h = hashlib.sha256("\n".join(lines(p, bw, va, vz)).encode()).hexdigest()
    return {"ops": p.prog.n_ops + (bw.prog.n_ops if bw is not None else 0), "sha256": h, "high_water": va.high_water}


# the 18 switches planner.py read before it had a table of them (all off unless set; SLIDERS_GN_ONE is on unless "0")
_PLANNER_SWITCHES = ["SLIDERS_NO_WEIGHT_TOUCH", "SLIDERS_NO_ATTN_TOUCH", "SLIDERS_TOUCH_FARTHEST", "SLIDERS_LORA_UNFUSED",
                     "SLIDERS_TRAIN_NO_LN_FOLD", "SLIDERS_NO_FUSED_VT", "SLIDERS_TRAIN_NO_FUSED_VT", "SLIDERS_GN_ONE",
                     "SLIDERS_GN_TWO_LAUNCH", "SLIDERS_NO_LORA_LN_FOLD", "SLIDERS_NO_FUSED_XATTN", "SLIDERS_TRAIN_UNFUSED_GEGLU",
                     "SLIDERS_TRAIN_KV_PER_BLOCK", "SLIDERS_BWD_DOT_LAUNCH", "SLIDERS_BWD_UNFUSED_GEGLU", "SLIDERS_BWD_UNBATCHED",
                     "SLIDERS_WGRAD_ATOMIC", "SLIDERS_BWD_UNFUSED_U"]
# tuning.py keeps its own reads: the ones that change plans, by name
_TUNING_SWITCHES = ["SLIDERS_NO_TUNING", "SLIDERS_SPLITK_ALL", "SLIDERS_XATTN_ALL"]


def switches() -> List[Tuple[str, str]]:
    """(environment variable, the value that flips it): the planner's from its table of switches (planner.Switches, one dataclass
    field per switch with the variable's name in its metadata), so that a switch added there is pinned here without anyone
    remembering to; then tuning.py's."""
    table = getattr(planner, "Switches", None)
    names = [f.metadata["env"] for f in dataclasses.fields(table)] if table is not None else _PLANNER_SWITCHES
    return [(n, "0" if n == "SLIDERS_GN_ONE" else "1") for n in names + _TUNING_SWITCHES]


DEFAULT_CASES = [("tiny_sdxl", 16, "noxattn"), ("tiny_sd1", 16, "full"), ("sd1", 64, "noxattn"), ("sdxl", 32, "noxattn"),
                 ("sdxl", 64, "noxattn"), ("sdxl", 128, "noxattn"), ("sdxl", 128, "full")]
SWITCH_CASE = ("sdxl", 64, "noxattn")
# switches whose feature the 64^2 plans do not reach (no touch with two candidate carriers, no accepted adapter fold, no to_q on the ring
# tile): flipped at 128^2 as well, where they move plans
WIDE_CASE = ("sdxl", 128, "noxattn")
WIDE_SWITCHES = ("SLIDERS_TOUCH_FARTHEST", "SLIDERS_NO_LORA_LN_FOLD", "SLIDERS_NO_FUSED_XATTN")


def matrix() -> List[Tuple[str, Tuple[str, int, str, str], Optional[Tuple[str, str]]]]:
    """(key, (configuration, latent size, train method, mode), switch or None) of every pinned plan"""
    out = []
    for name, hw, method in DEFAULT_CASES:
        for mode in MODES:
            out.append((f"{name}|{hw}|{method}|{mode}", (name, hw, method, mode), None))
    for var, val in switches():
        for case in (SWITCH_CASE,) + ((WIDE_CASE,) if var in WIDE_SWITCHES else ()):
            for mode in MODES:
                out.append((f"{'|'.join(map(str, case))}|{mode}|{var}={val}", (*case, mode), (var, val)))
    return out


def planned(case, switch, ln_fold: bool = True):
    """plan(*case) with the switch set in the environment for the time of planning"""
    assert not [v for v, _ in switches() if v in os.environ], "the digests are taken with every switch at its default"
    if switch is not None:
        os.environ[switch[0]] = switch[1]
    try:
        return plan(*case, ln_fold=ln_fold)
    finally:
        if switch is not None:
            del os.environ[switch[0]]


def digests() -> Dict[str, dict]:
    return {key: record(*planned(case, switch)) for key, case, switch in matrix()}


def _main(argv):
    if "--dump" in argv:
        out = argv[argv.index("--dump") + 1]
        os.makedirs(out, exist_ok=True)
        for key, case, switch in matrix():
            with open(os.path.join(out, key.replace("|", "_") + ".txt"), "w") as fh:
                fh.write("\n".join(lines(*planned(case, switch))) + "\n")
        print(f"wrote {len(matrix())} plans to {out}")
        return
    table = digests()
    print(f"{len(table)} plans, {sum(r['ops'] for r in table.values())} ops")
    if "--write" in argv:
        os.makedirs(os.path.dirname(DATA), exist_ok=True)
        with open(DATA, "w") as fh:                   # one plan per line: a changed plan reads as a one-line diff
            fh.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in table.items()) + "\n}\n")
        print(f"wrote {DATA} ({os.path.getsize(DATA)} bytes)")
    else:
        rec = json.load(open(DATA))
        bad = sorted(set(table) ^ set(rec)) + [k for k in table if k in rec and table[k] != rec[k]]
        print("identical to the recorded file" if not bad else f"differs from the recorded file: {bad}")
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    _main(sys.argv[1:])
