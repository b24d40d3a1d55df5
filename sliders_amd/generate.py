"""Batch inference with a trained slider at several scales (eval-scripts/generate_images_sd1.py:43-215,
trainscripts/textsliders/generate_images_xl.py:405-512), on the MI355X engine:

    python -m sliders_amd.generate --model sdxl --lora_weight models/age_alpha1.0_rank4_noxattn/age_alpha1.0_rank4_noxattn_last.pt \
        --prompt "image of a person" --scales=-2,-1,0,1,2 --start_noise 750 --seed 0 --out images/ [--model_path DIR | --synthetic]

Like the reference's consumers it reads rank / alpha / train_method from the checkpoint's FILE NAME
(XL-sliders-inference.ipynb cell 6: 'rank4', 'alpha1', 'noxattn' / 'full' substrings), builds the network, strict-loads
the .pt, and for every scale runs the 50-step DDIM loop with the slider switched on below `start_noise`.

Without a slider, `--direction "POSITIVE|NEGATIVE[:ETA]"` / `--direction_file prompts.yaml` steer with the prompt pair a slider would be
trained on, `--scales` sweeping its strength (sliders_amd/directions.py; docs/SAMPLING.md, "Prompt-direction sampling").
"""
from __future__ import annotations

import argparse
import os
import re
from typing import Tuple

import torch


def parse_slider_name(path: str) -> Tuple[int, float, str]:
    """(rank, alpha, train_method) from a slider file name, with the reference notebooks' defaults (4, 1.0, 'noxattn')."""
    name = os.path.basename(path)
    rank, alpha, method = 4, 1.0, "noxattn"
    m = re.search(r"rank(\d+)", name)
    if m:
        rank = int(m.group(1))
    m = re.search(r"alpha(\d+(?:\.\d+)?)", name)
    if m:
        alpha = float(m.group(1))
    for cand in ("noxattn-hspace-last", "noxattn-hspace", "xattn-strict", "innoxattn", "selfattn", "noxattn", "xattn", "full"):
        if cand in name:
            method = cand
            break
    return rank, alpha, method


def build_parser(defaults: bool = True) -> argparse.ArgumentParser:
    """defaults=False: no argument has a default, so the parsed namespace holds exactly what the command line gives (explicit_args)"""
    p = argparse.ArgumentParser()

    def add(*names, **kw):
        if not defaults:
            kw["default"] = argparse.SUPPRESS
        p.add_argument(*names, **kw)

    add("--model", default="sdxl", choices=["sdxl", "sd1"])
    add("--model_path", default=None, help="diffusers-format model directory (unet/, vae/, text encoders)")
    add("--synthetic", action="store_true", help="random-init weights and embeddings (no model files)")
    add("--lora_weight", default=None, help="slider checkpoint (.pt) written by the trainers")
    add("--compose", action="append", default=[], metavar="PATH:SCALE",
                   help="one more slider (.pt, any rank) held at a fixed scale in every image; repeatable.  With --compose, or when "
                        "--lora_weight is not rank 4, the sliders are merged into the weights (sliders_amd/merge.py)")
    add("--prompt", default="image of a person")
    add("--negative_prompt", default=None, help="the unconditional row of the CFG pair is this prompt's encoding instead of the empty prompt's")
    add("--scales", default="-2,-1,0,1,2")
    add("--start_noise", type=int, default=750)
    add("--ddim_steps", type=int, default=50, help="sampling steps (default 50; 4 with --turbo)")
    add("--guidance_scale", type=float, default=7.5)
    add("--scheduler", default="ddim", choices=["ddim", "lms", "euler", "euler_a", "ddpm", "dpmpp_2m"],
                   help="ddim (default): fused HIP step; lms: what eval-scripts/generate_images_sd1.py:51 constructs; euler: the SDXL "
                        "checkpoints' scheduler_config (generate_images_xl.py); euler_a: what --turbo samples with; dpmpp_2m: "
                        "DPM-Solver++ 2M on fp32 latents (docs/SAMPLING.md)")
    add("--timestep_spacing", default=None, choices=["leading", "linspace", "trailing"],
                   help="timestep grid of euler / euler_a / dpmpp_2m (default: each scheduler's own); trailing (euler_a, dpmpp_2m) "
                        "starts at t = 999: the few-step grid")
    add("--fp32_latents", action="store_true",
                   help="lms / euler / euler_a / ddpm: keep an fp32 master latent and step it with one fused launch per pass instead of "
                        "the tensor-op scheduler on a bf16 latent (dpmpp_2m always does)")
    add("--no_cfg", dest="no_cfg", action="store_true",
                   help="no classifier-free guidance: only the text prompt is encoded, one UNet row per image.  Implied by "
                        "--guidance_scale <= 1 together with --timestep_spacing")
    add("--cfg", dest="no_cfg", action="store_false", help="keep the unconditional / text pair: only meaningful where --no_cfg would otherwise hold, that is under --turbo or "
                        "with --guidance_scale <= 1 next to --timestep_spacing")
    add("--turbo", action="store_true",
                   help="few-step sampling as demo_SDXL_Turbo.ipynb: --scheduler euler_a --timestep_spacing trailing "
                        "--no_cfg --ddim_steps 4 --res 512; each part can be overridden by giving it explicitly")
    add("--res", type=int, default=None)
    add("--seed", type=int, default=0)
    add("--device", type=int, default=0)
    add("--out", default="images")
    add("--prompts_path", default=None,
                   help="csv with prompt / evaluation_seed / case_number columns (eval-scripts/generate_images_sd1.py:104-107): images go to "
                        "<out>/<slider name>/<scale>/<case_number>_<sample>.png - the layout eval-scripts/clip_score.py and "
                        "sliders_amd.clip_score read")
    add("--num_samples", type=int, default=1)
    add("--from_case", type=int, default=0)
    add("--till_case", type=int, default=1000000)
    # localised sampling (docs/SAMPLING.md): the options of sliders_amd.edit, with the scale-0 image of the seed in place of a photograph
    add("--mask", default=None, help="localise the slider: an image file, white = the slider acts, black = keep the scale-0 image bit for bit")
    add("--mask_invert", action="store_true", help="with --mask: black = the slider acts")
    add("--mask_feather", type=float, default=None, metavar="SIGMA",
        help="Gaussian feathering of the mask in latent pixels (default 0 with --mask, 1 with --auto_mask)")
    add("--auto_mask", action="store_true", help="localise the slider to its own footprint on the scale-0 image")
    add("--auto_mask_scale", type=float, default=None, help="slider scale the footprint is measured at (default: the largest |scale| of --scales)")
    add("--auto_mask_draws", type=int, default=None, help="noise levels the footprint averages over (default 8)")
    add("--auto_mask_threshold", type=float, default=None, help="binarisation threshold of the footprint (default 0.5)")
    add("--auto_mask_dilate", type=int, default=None, help="latent pixels the binary footprint is grown by (default 1)")
    add("--mask_word", action="append", default=[], metavar="WORD",
        help="localise the slider to where this word of the prompt lives in the cross-attention; repeatable (needs the model's tokenizer)")
    add("--mask_tokens", default=None, metavar="I,J,...", help="the same from key positions of the prompt (BOS = 0)")
    add("--mask_word_threshold", type=float, default=None, help="binarisation threshold of the word map / its maximum (default 0.3)")
    add("--mask_word_draws", type=int, default=None, help="steps of the grid the word map averages over (default 8)")
    add("--save_attention", default=None, help="write the word map / its maximum here (8-bit PNG at latent resolution)")
    add("--save_mask", default=None, help="write the latent-resolution mask here (8-bit PNG)")
    # prompt-direction sampling (docs/SAMPLING.md): a slider's training target as guidance, --scales sweeps its strength
    add("--direction", action="append", default=[], metavar="POSITIVE|NEGATIVE[:ETA]",
        help="steer with eps(POSITIVE) - eps(NEGATIVE), times ETA (default 1) times the scale; repeatable, at most 3")
    add("--direction_file", default=None, help="the same from a prompts.yaml of the trainers: positive, unconditional, guidance_scale (ETA) "
                                               "and action (erase: the opposite sign) of its entries")
    add("--direction_entries", default=None, metavar="I,J,...", help="entries of --direction_file to take (default: all, at most 3)")
    add("--direction_quantile", type=float, default=None, metavar="Q",
        help="keep only the largest 1 - Q of each latent channel's differences (default 0: all of them)")
    add("--direction_momentum", default=None, metavar="S_M[:BETA]",
        help="SEGA's momentum on the direction: strength S_M, decay BETA (default 0.4); 0: none")
    return p


def direction_specs(a) -> list:
    """[(positive, negative, eta, sign)] of --direction / --direction_file; every error of these options is raised here"""
    import math
    from .directions import MAX_DIRECTIONS
    if a.direction and a.direction_file:
        raise SystemExit("--direction and --direction_file: give one of them")
    if a.direction_entries is not None and not a.direction_file:
        raise SystemExit("--direction_entries needs --direction_file")
    specs = []
    for spec in a.direction:
        pos, sep, neg = spec.partition("|")
        eta = 1.0
        if ":" in neg:
            neg, _, tail = neg.rpartition(":")
            try:
                eta = float(tail)
            except ValueError:
                sep = ""
        if not sep or not pos.strip():
            raise SystemExit(f"--direction {spec!r}: expected POSITIVE|NEGATIVE[:ETA]")
        if not math.isfinite(eta):
            raise SystemExit(f"--direction {spec!r}: expected a finite ETA")
        specs.append((pos, neg, eta, 1.0))
    if a.direction_file:
        if not os.path.isfile(a.direction_file):
            raise SystemExit(f"--direction_file {a.direction_file}: no such file")
        from .prompt_util import load_prompts_from_yaml
        entries = load_prompts_from_yaml(a.direction_file)
        picked = list(range(len(entries)))
        if a.direction_entries is not None:
            try:
                picked = [int(v) for v in a.direction_entries.split(",")]
            except ValueError:
                raise SystemExit(f"--direction_entries {a.direction_entries!r}: expected comma-separated entry numbers")
            if not picked or any(not 0 <= i < len(entries) for i in picked):
                raise SystemExit(f"--direction_entries {a.direction_entries!r}: {a.direction_file} has the entries 0 .. {len(entries) - 1}")
        specs = [(entries[i].positive, entries[i].unconditional, float(entries[i].guidance_scale), 1.0 if entries[i].action == "enhance" else -1.0)
                 for i in picked]
    if len(specs) > MAX_DIRECTIONS:
        raise SystemExit(f"{len(specs)} directions: at most {MAX_DIRECTIONS} (one UNet pass carries at most 8 row blocks); choose with "
                         "--direction_entries")
    return specs


DEFAULT_MOMENTUM_BETA = 0.4


def direction_momentum(a):
    """--direction_momentum S_M[:BETA] -> (s_m, beta), or None where the option is not given; every error of the option is raised here"""
    from .directions import check_momentum
    if a.direction_momentum is None:
        return None
    head, sep, tail = a.direction_momentum.partition(":")
    try:
        pair = (float(head), float(tail) if sep else DEFAULT_MOMENTUM_BETA)
    except ValueError:
        raise SystemExit(f"--direction_momentum {a.direction_momentum!r}: expected S_M[:BETA]")
    try:
        check_momentum(pair)
    except ValueError as e:
        raise SystemExit(f"--direction_momentum {a.direction_momentum!r}: {e}")
    return pair


def check_direction_args(a, no_cfg=None, guidance_scale=None, guidance_option: str = "--guidance_scale") -> list:
    """every argument error of the direction options (shared with sliders_amd.edit, which has no --no_cfg and may name another
    guidance option: the arguments in their place)"""
    from .directions import DirectionSet
    no_cfg = a.no_cfg if no_cfg is None else no_cfg
    guidance_scale = a.guidance_scale if guidance_scale is None else guidance_scale
    specs = direction_specs(a)
    momentum = direction_momentum(a)
    if not specs:
        if a.direction_quantile is not None:
            raise SystemExit("--direction_quantile needs --direction or --direction_file")
        if momentum is not None:
            raise SystemExit("--direction_momentum needs --direction or --direction_file")
        return specs
    try:
        DirectionSet.n_keep(1, a.direction_quantile or 0.0)
    except ValueError as e:
        raise SystemExit(f"--direction_quantile: {e}")
    if a.lora_weight:
        raise SystemExit("--direction / --direction_file: --scales sweeps the direction's strength, not with --lora_weight (sliders held at a "
                         "fixed scale go next to it with --compose)")
    if not no_cfg and guidance_scale == 0:
        raise SystemExit(f"--direction with {guidance_option} 0: the direction enters through the text row of the CFG pair, which a guidance "
                         "of 0 does not read" + (" (or sample with --no_cfg)" if hasattr(a, "no_cfg") else ""))
    return specs


def direction_set(a, specs, encode, cfg, xl: bool) -> dict:
    """The directions= / direction_quantile= / direction_momentum= of a run, from direction_specs' pairs ({}: there are none).
    encode(text) -> (ctx (1, 77, D), pooled (1, P) or None).  --synthetic: the direction rows are draws of their own (seed + 1), so
    the prompt rows' draws are what they are without the options."""
    if not specs:
        return {}
    from .directions import Direction, DirectionSet
    if a.synthetic:
        gd = torch.Generator().manual_seed(a.seed + 1)

        def encode(text):
            return (torch.randn(1, 77, cfg.cross_attention_dim, generator=gd), torch.randn(1, cfg.pooled_dim, generator=gd) if xl else None)
    pairs = [(encode(pos), encode(neg), eta, sign) for pos, neg, eta, sign in specs]
    steer = dict(directions=DirectionSet([Direction(cp, cn, pp, pn, eta=eta, sign=sign) for (cp, pp), (cn, pn), eta, sign in pairs]),
                 direction_quantile=a.direction_quantile or 0.0)
    momentum = direction_momentum(a)
    if momentum is not None:
        steer["direction_momentum"] = momentum
    return steer


def sampling_grid(a) -> list:
    """the timesteps the run visits, from the scheduler SliderSampler will build (host tables only)"""
    from . import schedulers
    from .ddim import DDIMSchedule
    if a.scheduler == "ddim":
        return DDIMSchedule().make_timesteps(a.ddim_steps)
    spacing = {} if a.timestep_spacing is None else {"timestep_spacing": a.timestep_spacing}
    if a.scheduler == "euler":
        sch = schedulers.EulerDiscreteScheduler(**spacing)
    elif a.scheduler == "dpmpp_2m":
        sch = schedulers.DPMSolverPP2MScheduler(**spacing)
    else:
        sch = schedulers.EulerAncestralDiscreteScheduler(**spacing) if spacing else schedulers.create(a.scheduler)
    sch.set_timesteps(a.ddim_steps)
    return sch.timesteps.tolist()


def masked(a) -> bool:
    return bool(a.mask or a.auto_mask or a.mask_word or a.mask_tokens is not None)


def check_args(a):
    """the scales, and every argument error of the mask options, before any model is built"""
    from .edit import check_mask_args
    scales = [float(v) for v in a.scales.split(",")]
    check_direction_args(a)
    if a.negative_prompt is not None and (a.no_cfg or a.synthetic):
        raise SystemExit("--negative_prompt is the unconditional row's prompt: not with --no_cfg (there is no such row) and not with "
                         "--synthetic (its rows are random draws)")
    check_mask_args(a, scales, lambda: sampling_grid(a))
    if masked(a):
        if a.scheduler not in ("ddim", "dpmpp_2m") and not a.fp32_latents:
            raise SystemExit(f"--mask / --auto_mask / --mask_word / --mask_tokens with --scheduler {a.scheduler}: the bf16 tensor-op path keeps no "
                             "trace of the scale-0 chain; add --fp32_latents (or sample with ddim)")
        if a.no_cfg and (a.mask_word or a.mask_tokens is not None):
            raise SystemExit("--mask_word / --mask_tokens read the cross-attention of the text half of the CFG pair: not with --no_cfg")
    return scales


def shares_prefix(a, scales) -> bool:
    """An unmasked sweep that contains scale 0 and another scale, on a loop without noise draws or multistep history: the scale-0 run
    is kept as a trace and the other scales start where the slider starts to act - the same images, bit for bit (asserted by
    tests/test_masked_sampling_gpu.py), without the replays of the steps every scale shares"""
    return 0.0 in scales and len(scales) > 1 and (a.scheduler == "ddim" or (a.scheduler == "euler" and a.fp32_latents))


def traced_sweep(a, smp, scales, ctx, pooled, noise, prompt, tokenizer, suffix="", **steer):
    """One seed over its scale-0 trace: with mask options the mask is derived from the trace once and every scale is blended against
    it; scale 0 is the trace's own image.  steer: directions= / direction_quantile= / direction_momentum= of the other scales.  Yields (scale, uint8 image
    [H][W][3] on the host)."""
    from .edit import mask_from_args
    from .vae import VaeDecoder
    trace = smp.base_trace(ctx, noise, a.ddim_steps, a.guidance_scale, pooled, None, a.start_noise)
    foot = {k: v for k, v in steer.items() if k != "direction_momentum"}          # --auto_mask: the directions' footprint
    mask = mask_from_args(a, smp, trace, a.res, prompt, tokenizer, suffix, **foot) if masked(a) else None
    for s in scales:
        lat = trace.final if s == 0.0 else smp.sample_latents(ctx, noise, scale=s, start_noise=a.start_noise, ddim_steps=a.ddim_steps,
                                                              guidance_scale=a.guidance_scale, pooled=pooled, mask=mask, trace=trace, **steer)
        yield s, VaeDecoder.to_uint8(smp.decoder.decode(lat))[0].cpu().numpy()


def parse_compose(spec: str) -> Tuple[str, float]:
    """'PATH:SCALE' -> (path, scale); the scale follows the LAST colon"""
    path, sep, scale = spec.rpartition(":")
    if not sep or not path:
        raise SystemExit(f"--compose {spec!r}: expected PATH:SCALE")
    try:
        return path, float(scale)
    except ValueError:
        raise SystemExit(f"--compose {spec!r}: {scale!r} is not a number")


def slider_rank(sd) -> int:
    """rank of a slider checkpoint, from its lora_down weights (the file name is only a convention)"""
    return max(int(v.shape[0]) for k, v in sd.items() if k.endswith(".lora_down.weight"))


def scale_folder(scale: float) -> str:
    """folder name of a slider scale as the reference writes it (generate_images_sd1.py:116-120: '0.5' -> 'half')"""
    return f"{scale:g}".replace("0.5", "half")


def explicit_args(argv) -> set:
    """names of the arguments this command line gives itself"""
    p = build_parser(defaults=False)
    return set(vars(p.parse_args(argv)))


def resolve_sampling(a, given: set):
    """Fill in, in place, what --turbo sets unless the command line gives it itself (`given`: explicit_args), and --no_cfg where it
    is implied.  Without --turbo, --timestep_spacing and --no_cfg every value is what it was before they existed."""
    if a.turbo:
        preset = {"scheduler": "euler_a", "timestep_spacing": "trailing", "no_cfg": True, "ddim_steps": 4, "res": 512}
        for k, v in preset.items():
            if k not in given:
                setattr(a, k, v)
    if "no_cfg" not in given and a.guidance_scale <= 1 and "timestep_spacing" in given:
        a.no_cfg = True
    if a.res is None:
        a.res = 1024 if a.model == "sdxl" else 512
    return a


def main(argv=None):
    from .cli import _encoded_pairs  # noqa: F401  (text encoders: model_util)
    from .lora_store import LoraStore
    from .model_util import load_unet_engine, synthetic_engine
    from .sampler import SliderSampler
    from .vae import VAE_SCALING, VaeDecoder, random_vae_state_dict
    a = resolve_sampling(build_parser().parse_args(argv), explicit_args(argv))
    scales = check_args(a)
    tokenizer = None
    dev = torch.device("cuda", a.device)
    xl = a.model == "sdxl"
    res = a.res
    prompts = (lambda text: [text]) if a.no_cfg else (lambda text: [a.negative_prompt or "", text])      # --no_cfg: the text prompt alone is encoded
    specs = direction_specs(a)
    if a.synthetic:
        eng = synthetic_engine(a.model, dev, a.seed)
        dec = VaeDecoder(random_vae_state_dict(device=dev, seed=a.seed, decoder=True), dev, VAE_SCALING[a.model])
        g = torch.Generator().manual_seed(a.seed)
        ctx = torch.randn(2, 77, eng.cfg.cross_attention_dim, generator=g)
        pooled = torch.randn(2, eng.cfg.pooled_dim, generator=g) if xl else None
        if a.no_cfg:         # the text row of the same draw
            ctx, pooled = ctx[1:], pooled[1:] if xl else None
        encode = None            # (direction_set draws the direction rows)
    else:
        if not a.model_path:
            raise SystemExit("--model_path (diffusers-format directory) or --synthetic is required")
        from safetensors.torch import load_file
        from . import model_util
        eng = load_unet_engine(a.model_path, dev)
        dec = VaeDecoder(load_file(os.path.join(a.model_path, "vae", "diffusion_pytorch_model.safetensors")), dev, VAE_SCALING[a.model])
        if xl:
            toks, encs = model_util.load_text_encoders_xl(a.model_path, dev, torch.bfloat16)
            tokenizer = toks[0]
            enc_xl = [model_util.encode_prompts_xl(toks, encs, [s]) for s in prompts(a.prompt)]
            ctx, pooled = torch.cat([e for e, _ in enc_xl]), torch.cat([q for _, q in enc_xl])
            encode = lambda text: model_util.encode_prompts_xl(toks, encs, [text])
        else:
            tok, enc = model_util.load_text_encoder(a.model_path, dev, torch.bfloat16)
            tokenizer = tok
            ctx, pooled = torch.cat([model_util.encode_prompts(tok, enc, [s]) for s in prompts(a.prompt)]), None
            encode = lambda text: (model_util.encode_prompts(tok, enc, [text]), None)
    steer = direction_set(a, specs, encode, eng.cfg, xl)
    store = sliders = None
    swept = torch.load(a.lora_weight, map_location="cpu") if a.lora_weight else None
    if a.compose or (swept is not None and slider_rank(swept) != 4):
        # several sliders, or a rank the fused adapter kernels are not built for: merged into the weights.  The swept slider
        # (scale None) takes each image's --scales value, the composed ones keep theirs
        from .merge import SliderSet
        held = [parse_compose(c) for c in a.compose]
        sliders = SliderSet(eng.cfg, ([(swept, None)] if swept is not None else [])
                            + [(torch.load(path, map_location="cpu"), s) for path, s in held])
    elif swept is not None:
        rank, alpha, method = parse_slider_name(a.lora_weight)
        store = LoraStore(eng.cfg, rank=rank, alpha=alpha, train_method=method, device=dev, init="none")
        store.load_state_dict(swept, strict=True)
    smp = SliderSampler(eng, store, dec, scheduler=a.scheduler, scheduler_seed=a.seed, sliders=sliders,
                        timestep_spacing=a.timestep_spacing, latents="fp32" if a.fp32_latents else None)
    os.makedirs(a.out, exist_ok=True)
    from PIL import Image
    traced = masked(a) or shares_prefix(a, scales)
    if a.prompts_path:
        # the reference's evaluation set-up: one row per case, every scale from the same seed, one folder per scale
        import pandas as pd
        df = pd.read_csv(a.prompts_path)
        name = os.path.basename(a.lora_weight).rsplit(".", 1)[0] if a.lora_weight else "no_slider"
        root = os.path.join(a.out, name)
        for s in scales:
            os.makedirs(os.path.join(root, scale_folder(s)), exist_ok=True)
        for _, row in df.iterrows():
            case = int(row.case_number)
            if not (a.from_case <= case <= a.till_case):
                continue
            if a.synthetic:
                c_row, p_row = ctx, pooled
            elif xl:
                enc_xl = [model_util.encode_prompts_xl(toks, encs, [t]) for t in prompts(str(row.prompt))]
                c_row, p_row = torch.cat([e for e, _ in enc_xl]), torch.cat([q for _, q in enc_xl])
            else:
                c_row, p_row = torch.cat([model_util.encode_prompts(tok, enc, [t]) for t in prompts(str(row.prompt))]), None
            for num in range(a.num_samples):
                if traced:
                    g = torch.Generator().manual_seed(int(row.evaluation_seed) + num)
                    noise = torch.randn(1, 4, res // 8, res // 8, generator=g)
                    for s, img in traced_sweep(a, smp, scales, c_row.to(dev), p_row.to(dev) if p_row is not None else None, noise.to(dev),
                                               str(row.prompt), tokenizer, f"_{case}_{num}", **steer):
                        Image.fromarray(img).save(os.path.join(root, scale_folder(s), f"{case}_{num}.png"))
                    continue
                for s in scales:
                    g = torch.Generator().manual_seed(int(row.evaluation_seed) + num)          # the same noise for every scale
                    noise = torch.randn(1, 4, res // 8, res // 8, generator=g)
                    img = smp.generate(c_row.to(dev), noise.to(dev), scale=s, start_noise=a.start_noise, ddim_steps=a.ddim_steps,
                                       guidance_scale=a.guidance_scale, pooled=p_row.to(dev) if p_row is not None else None, **steer)
                    Image.fromarray(img[0].cpu().numpy()).save(os.path.join(root, scale_folder(s), f"{case}_{num}.png"))
            print(f"case {case}: {a.num_samples} sample(s) x {len(scales)} scales saved under {root}")
        return root
    if traced:
        noise = torch.randn(1, 4, res // 8, res // 8, generator=torch.Generator().manual_seed(a.seed))
        for s, img in traced_sweep(a, smp, scales, ctx.to(dev), pooled.to(dev) if pooled is not None else None, noise.to(dev), a.prompt, tokenizer,
                                   **steer):
            Image.fromarray(img).save(os.path.join(a.out, f"scale_{s:g}.png"))
            print(f"scale {s:g}: saved {os.path.join(a.out, f'scale_{s:g}.png')}")
        return a.out
    for s in scales:
        noise = torch.randn(1, 4, res // 8, res // 8, generator=torch.Generator().manual_seed(a.seed))   # same seed per scale
        img = smp.generate(ctx.to(dev), noise.to(dev), scale=s, start_noise=a.start_noise, ddim_steps=a.ddim_steps,
                           guidance_scale=a.guidance_scale, pooled=pooled.to(dev) if pooled is not None else None, **steer)
        Image.fromarray(img[0].cpu().numpy()).save(os.path.join(a.out, f"scale_{s:g}.png"))
        print(f"scale {s:g}: saved {os.path.join(a.out, f'scale_{s:g}.png')}")
    return a.out


if __name__ == "__main__":
    main()
