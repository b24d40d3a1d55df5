"""Timing probe of the weight merge (sliders_amd/merge.py) at SDXL full size; nothing here is asserted.

1. The merge launch - `full`, three sliders of ranks 4 / 8 / 16 (total R = 28) - against a device-to-device hipMemcpyAsync of the
   same tensors (pristine copy -> live tensor), same process, alternating.  A kernel that reads base and writes out should cost about
   what the copy costs; the factor reads and R fmas per element are the only extra work.
2. Per-step time of the merged sampler next to the fused-adapter sampler, one rank-4 noxattn slider, SDXL 1024^2 (latent 128^2),
   DDIM: whole `sample_latents` calls, host clock around a device synchronise, alternating.

    python scripts/time_merge.py [--out profiles/merge_timing.txt] [--steps 20] [--reps 5] [--skip_sampler]
"""
import argparse
import ctypes
import os
import socket
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _hip():
    """the HIP runtime torch loaded (one instance per process)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip_sampler", action="store_true")
    a = ap.parse_args()
    from sliders_amd.config import CONFIGS
    from sliders_amd.lora_store import LoraStore
    from sliders_amd.merge import SliderSet, WeightMerger
    from sliders_amd.random_init import random_state_dict
    from sliders_amd.sampler import SliderSampler
    from sliders_amd.unet import UNetEngine
    from test_merge_gpu import drawn_slider

    dev = torch.device("cuda:0")
    cfg = CONFIGS["sdxl"]()
    eng = UNetEngine(cfg, random_state_dict(cfg, dev, 0, torch.bfloat16), dev)
    lines = [f"box {socket.gethostname()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}"]

    # ---- 1. merge launch vs device-to-device copy ---------------------------------------------------------------------------------
    sliders = [(drawn_slider(cfg, "full", r, float(r), 40 + r), s) for r, s in ((4, 1.5), (8, -1.0), (16, 0.5))]
    mg = WeightMerger(eng.w, SliderSet(cfg, sliders))
    scales = [s for _, s in sliders]
    mg.merge(scales)
    mg.restore()
    torch.cuda.synchronize()
    hip = _hip()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    D2D = 3
    pairs = [(eng.w.t[n].data_ptr(), mg._pristine[n].data_ptr(), eng.w.t[n].numel() * eng.w.t[n].element_size()) for n in mg.touched]
    nbytes = sum(p[2] for p in pairs)
    s = torch.cuda.current_stream().cuda_stream
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0, e1 = ev(), ev()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def copy_all():
        for dst, src, n in pairs:
            rc = hip.hipMemcpyAsync(dst, src, n, D2D, s)
            assert rc == 0, rc

    t_merge, t_copy = [], []
    for i in range(2 + a.reps):
        tm, tc = timed(lambda: mg.merge(scales)), timed(copy_all)
        if i >= 2:
            t_merge.append(tm)
            t_copy.append(tc)
    mg.restore()
    torch.cuda.synchronize()
    rows = sum(it.rows for it in mg.items)
    fma = sum(it.rows * it.K * it.R for it in mg.items)
    m, c = statistics.median(t_merge), statistics.median(t_copy)
    lines += [
        f"merge: sdxl, train_method full, sliders of rank 4 + 8 + 16 (R = 28), {len(mg.items)} items, {rows} rows, {len(mg.touched)} tensors touched",
        f"bytes: {nbytes} written ({nbytes / 2 ** 30:.2f} GiB), as many read from the pristine copies; {fma / 1e9:.1f} G fma",
        f"slh_lora_merge (one launch, incl. the coefficient upload): median {m:.2f} ms of {a.reps} (min {min(t_merge):.2f}, max {max(t_merge):.2f})"
        f" = {2 * nbytes / m / 1e6:.0f} GB/s read + written",
        f"hipMemcpyAsync device-to-device of the same tensors ({len(pairs)} calls): median {c:.2f} ms (min {min(t_copy):.2f}, max {max(t_copy):.2f})"
        f" = {2 * nbytes / c / 1e6:.0f} GB/s read + written",
        f"ratio merge / copy: {m / c:.2f}",
    ]
    print("\n".join(lines), flush=True)

    # ---- 2. per-step time: merged sampler vs fused-adapter sampler ----------------------------------------------------------------
    if not a.skip_sampler:
        del mg
        torch.cuda.empty_cache()
        hw = 128
        store = LoraStore(cfg, rank=4, alpha=1.0, train_method="noxattn", device=dev)
        g = torch.Generator().manual_seed(0)
        for e in store.entries:
            store.params[e.up_off:e.up_off + e.up_numel] = (torch.randn(e.up_numel, generator=g) * 0.05).to(dev, torch.bfloat16)
        merged = SliderSampler(eng, scheduler="ddim", sliders=SliderSet(cfg, [(store.state_dict(), None)]))
        ctx = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).to(dev)
        pooled = torch.randn(2, cfg.pooled_dim, generator=g).to(dev)
        noise = torch.randn(1, 4, hw, hw, generator=g).to(dev)
        kw = dict(scale=1.0, start_noise=750, ddim_steps=a.steps, guidance_scale=7.5, pooled=pooled)

        def run(smp):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            smp.sample_latents(ctx, noise, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(3):          # warm-up: code objects, graph capture of the adapter-free program
            run(merged)
        tm = [run(merged) for _ in range(a.reps)]
        fused = SliderSampler(eng, store, scheduler="ddim")         # attaches the store: the `on` plans are built from here on
        for _ in range(3):
            run(fused)
        tf = [run(fused) for _ in range(a.reps)]
        tm2 = [run(merged) for _ in range(a.reps)]                  # and the merged path once more, after the fused one
        md, fd, md2 = statistics.median(tm), statistics.median(tf), statistics.median(tm2)
        # the pieces: one replay of each program, and the merge / restore of this slider alone
        def replay(prog):
            for _ in range(3):
                prog.run(s)
            return statistics.median(timed(lambda: prog.run(s)) for _ in range(a.reps))
        p_off, p_on = eng.plan(2, hw, hw, "off"), eng.plan(2, hw, hw, "on")
        eng.set_lora(True, 1.0)
        pieces = [("adapter-free pass", replay(p_off.prog)), ("adapter-free pass, text K/V cached", replay(p_off.prog_text_cached)),
                  ("fused-adapter pass", replay(p_on.prog)), ("fused-adapter pass, text K/V cached", replay(p_on.prog_text_cached))]
        eng.set_lora(False)
        mg1 = merged.merger
        tmm, trr = [], []
        for _ in range(a.reps):
            tmm.append(timed(lambda: mg1.merge([1.0])))
            trr.append(timed(mg1.restore))
        pieces += [("merge of this slider", statistics.median(tmm)), ("restore", statistics.median(trr))]
        lines += [
            f"sampler: sdxl 1024x1024 (latent {hw}), CFG pair, DDIM {a.steps} steps, one rank-4 noxattn slider, start_noise 750, whole sample_latents calls",
            f"merged weights (merge + restore inside every call): median {md:.1f} ms = {md / a.steps:.2f} ms / step (second block {md2 / a.steps:.2f})",
            f"fused adapters: median {fd:.1f} ms = {fd / a.steps:.2f} ms / step",
            "pieces (device events, median): " + "; ".join(f"{k} {v:.2f} ms" for k, v in pieces),
        ]
        print("\n".join(lines[-4:]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
