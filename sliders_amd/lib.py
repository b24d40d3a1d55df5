"""ctypes binding of libsliders_hip.so (include/sliders_hip.h).

The product path has NO fallback: if the shared library is missing, or an opcode's entry point or descriptor
size disagrees with the library's own op table (slh_op_info), load() raises, and every op raises RuntimeError with the
library's slh_last_error() text on a non-zero status.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SLIDERS_HIP_LIB") or os.path.join(_HERE, "libsliders_hip.so")   # override: development builds

c_i32, c_i64, c_f32, c_f64, c_vp = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_void_p


def _struct(name, fields):
    return type(name, (C.Structure,), {"_fields_": fields})


def _ptrs(*names):
    return [(n, c_vp) for n in names]


def _ints(*names):
    return [(n, c_i32) for n in names]


GemmDesc = _struct("GemmDesc", _ptrs("a0", "a1", "w", "bias", "rowbias", "lora_t", "lora_up", "lora_scale",
                                     "residual", "c", "lora_down", "lora_t_out")
                   + _ints("lda0", "lda1", "ca0", "ca1", "mode", "batch", "hs", "ws", "src_xform", "stride",
                           "ho", "wo", "ldw", "M", "N", "K", "ld_rowbias", "rows_per_sample", "ld_t",
                           "lora_groups", "ld_res", "ldc", "geglu", "tile", "lora_rank", "lora_up_rmajor", "w_layout",
                           "reserved_") + _ptrs("splitk_c32", "splitk_t32", "vt_out")
                   + _ints("vt_col0", "vt_D", "vt_heads", "vt_tokens", "vt_ld", "splitk_slabs")
                   + _ptrs("ln_out", "ln_in", "ln_s", "ln_b") + _ints("ln_in_chunks") + [("ln_eps", c_f32)]
                   + _ptrs("splitk_ticket", "ln_mr_out", "geglu_pre") + _ints("ld_pre", "vt_also_c")
                   + _ptrs("xa_k", "xa_vt") + _ints("xa_tk", "xa_tq", "xa_ldk", "xa_ldvt", "xa_vt_heads") + [("xa_scale", c_f32)]
                   + _ptrs("ln_lora_s", "ln_lora_c", "pf_ptr") + [("pf_bytes", c_i64)])
SkinnyDesc = _struct("SkinnyDesc", _ptrs("a0", "a1", "w", "bias", "out")
                     + _ints("lda0", "lda1", "ca0", "ca1", "mode", "batch", "hs", "ws", "src_xform", "stride",
                             "ho", "wo", "M", "R", "K", "ldo", "out_kind", "w_kmajor"))
GemvDesc = _struct("GemvDesc", _ptrs("x", "w", "bias", "addend", "lora_t", "lora_tcol", "lora_up", "lora_scale", "y")
                   + _ints("nb", "N", "K", "ldx", "ld_add", "ld_t", "ldy", "in_act", "out_f32"))
GnDesc = _struct("GnDesc", _ptrs("x0", "x1", "gamma", "beta", "stats", "y")
                 + _ints("ldx0", "ldx1", "c0", "c1", "batch", "hw", "groups", "ldy") + [("eps", c_f32)]
                 + _ints("act") + _ptrs("partial", "ticket"))
GnBwdDesc = _struct("GnBwdDesc", _ptrs("x0", "x1", "gamma", "beta", "stats", "bstats", "dy", "dx0", "dx1")
                    + _ints("ldx0", "ldx1", "c0", "c1", "batch", "hw", "groups", "lddy", "lddx0", "lddx1")
                    + [("eps", c_f32)] + _ints("act", "accumulate0", "accumulate1") + _ptrs("bpartial", "bticket"))
LnDesc = _struct("LnDesc", _ptrs("x", "gamma", "beta", "y", "mean_rstd") + _ints("M", "C", "ldx", "ldy")
                 + [("eps", c_f32)])
LnBwdDesc = _struct("LnBwdDesc", _ptrs("x", "gamma", "dy", "mean_rstd", "dx")
                    + _ints("M", "C", "ldx", "lddy", "lddx", "accumulate"))
AttnDesc = _struct("AttnDesc", _ptrs("q", "k", "vt", "o", "lse")
                   + _ints("B", "H", "Tq", "Tk", "ldq", "ldk", "ldvt", "ldo") + [("scale", c_f32)]
                   + _ints("D", "vt_batch_heads", "reserved_") + _ptrs("pf_ptr") + [("pf_bytes", c_i64)])
TransposeDesc = _struct("TransposeDesc", _ptrs("src", "dst") + _ints("B", "H", "T", "ld", "ldt", "D"))
AttnBwdDesc = _struct("AttnBwdDesc", _ptrs("q", "k", "v", "o", "d_o", "kt", "qt", "dot", "lse", "delta", "dq", "dk", "dv")
                      + _ints("B", "H", "Tq", "Tk", "ldq", "ldk", "ldv", "ldo", "lddo", "ldkt", "ldqt", "lddq", "lddk",
                              "lddv")
                      + [("scale", c_f32)] + _ints("need_dkv", "D", "pad_"))
TembedDesc = _struct("TembedDesc", _ptrs("vals", "out") + _ints("nb", "n_vals", "dim", "ldo", "col0"))
ConvInDesc = _struct("ConvInDesc", _ptrs("x", "w", "bias", "y") + _ints("batch", "cin", "h", "wd", "cout", "ldy"))
EwDesc = _struct("EwDesc", _ptrs("a", "b", "out") + _ints("M", "C", "lda", "ldb", "ldo", "op", "iarg", "iarg2")
                 + [("alpha", c_f32)] + _ints("pad_"))
CfgDdimDesc = _struct("CfgDdimDesc", _ptrs("eps", "x", "out", "out2", "eps_text") + _ints("nb", "chw")
                      + [("guidance", c_f32), ("c_sqrt_beta_t", c_f32), ("c_inv_sqrt_alpha_t", c_f32),
                         ("c_sqrt_alpha_prev", c_f32), ("c_dir", c_f32)] + _ints("do_step", "v_prediction")
                      + [("c_sqrt_alpha_t", c_f32)] + _ints("pad_"))
DdpmEditDesc = _struct("DdpmEditDesc", _ptrs("eps", "eps_text", "x", "target", "resid", "out", "out_bf16", "out2_bf16") + _ints("nb", "chw")
                       + [(n, c_f32) for n in ("guidance", "c_sqrt_beta_t", "c_inv_sqrt_alpha_t", "c_sqrt_alpha_t", "c_sqrt_alpha_prev", "c_dir")]
                       + _ints("mode", "v_prediction"))
DdpmEditBlendDesc = _struct("DdpmEditBlendDesc", _ptrs("eps", "eps_text", "x", "resid", "keep", "mask", "out", "out_bf16", "out2_bf16")
                            + _ints("nb", "chw", "hw")
                            + [(n, c_f32) for n in ("guidance", "c_sqrt_beta_t", "c_inv_sqrt_alpha_t", "c_sqrt_alpha_t", "c_sqrt_alpha_prev", "c_dir")]
                            + _ints("v_prediction"))
EpsAbsdiffDesc = _struct("EpsAbsdiffDesc", _ptrs("eps_a", "eps_a_text", "eps_b", "eps_b_text", "out") + _ints("nb", "chw", "hw")
                         + [("guidance", c_f32)])
XattnMapDesc = _struct("XattnMapDesc", _ptrs("q", "k", "wt", "out") + _ints("B", "b0", "nb", "H", "D", "Tq", "Tk", "ldq", "ldk")
                       + [("scale", c_f32), ("coef", c_f32)] + _ints("accumulate"))
LossDesc = _struct("LossDesc", _ptrs("target", "positive", "neutral", "uncond", "loss", "dtarget", "dtarget_pix")
                   + _ints("n") + [("guidance", c_f32)] + _ints("erase", "hw", "nch"))
WgradDesc = _struct("WgradDesc", _ptrs("z0", "z1", "v", "out", "scale")
                    + _ints("ldz0", "ldz1", "c0", "c1", "mode", "batch", "hs", "ws", "src_xform", "stride", "ho",
                            "wo", "M", "R", "ldv", "ldo", "out_rmajor", "vgroup_cols") + _ptrs("slabs", "tickets"))
AdamwDesc = _struct("AdamwDesc", _ptrs("param", "exp_avg", "exp_avg_sq", "grad") + [("n", c_i64)]
                    + [(n, c_f64) for n in ("lr", "beta1", "beta2", "eps", "weight_decay")]
                    + _ints("step") + [("grad_scale", c_f32)] + _ptrs("param_lo") + _ints("f32_state", "pad_"))
LionDesc = _struct("LionDesc", _ptrs("param", "exp_avg", "grad") + [("n", c_i64)]
                   + [(n, c_f64) for n in ("lr", "beta1", "beta2", "weight_decay")] + [("grad_scale", c_f32)] + _ints("pad_"))
MemsetDesc = _struct("MemsetDesc", _ptrs("ptr") + [("nbytes", c_i64)] + _ints("value", "pad"))
LoraCdgradDesc = _struct("LoraCdgradDesc", _ptrs("u", "a_down", "scale", "gx")
                         + _ints("batch", "hl", "wl", "ho", "wo", "stride", "cin", "ldu", "ldgx", "accumulate"))
TembLoraBwdDesc = _struct("TembLoraBwdDesc", _ptrs("g", "t", "up", "emb", "d_up", "d_down", "scale") + _ints("C", "ted"))
# image sliders: fp32 AutoencoderKL encoder (csrc/vae.hip)
SgemmDesc = _struct("SgemmDesc", _ptrs("x", "w", "bias", "residual", "c")
                    + _ints("ldx", "ldw", "ldr", "ldc", "M", "N", "K", "mode", "cin", "batch", "hs", "ws", "ho", "wo", "stride",
                            "pad", "bias_per_row") + [("alpha", c_f32)] + _ints("upsample", "split_bf16"))
Gn32Desc = _struct("Gn32Desc", _ptrs("x", "gamma", "beta", "stats", "y") + _ints("ldx", "ldy", "C", "batch", "hw", "groups")
                   + [("eps", c_f32)] + _ints("act") + _ptrs("partial", "ticket"))
Softmax32Desc = _struct("Softmax32Desc", _ptrs("x") + [("ld", c_i64)] + _ints("rows", "cols"))
VaeConvDesc = _struct("VaeConvDesc", _ptrs("x", "w", "bias", "qw", "qb", "y") + _ints("batch", "h", "wd", "cin", "cout")
                      + [("inv_scaling", c_f32)])
BatchDesc = _struct("BatchDesc", _ptrs("table", "prefix") + _ints("n", "total", "arg", "pad_") + _ptrs("slabs", "tickets"))
Gather16Desc = _struct("Gather16Desc", _ptrs("src", "idx", "out") + [("n", c_i64)])
LoraLnFoldDesc = _struct("LoraLnFoldDesc", _ptrs("items") + _ints("n", "pad_"))
LORA_LNFOLD_ITEM_I64 = 7          # slh_lora_lnfold_item as int64 words: a, gamma, beta, a_out, s_out, c_out, rows | K << 32
LORA_LNFOLD_MAX_ROWS = 16         # the kernel's grid is 16 rows per item


def lnfold_item(a: int, gamma: int, beta: int, a_out: int, s_out: int, c_out: int, rows: int, K: int) -> tuple:
    """One slh_lora_lnfold_item as int64 words.  The items live in device memory where the library cannot check them, so the limits of
    the kernel are checked here: rows <= 16 (its grid; further rows would be left out silently) and K % 8 == 0."""
    if not (1 <= rows <= LORA_LNFOLD_MAX_ROWS) or K <= 0 or K % 8:
        raise SlidersHipError(f"slh_lora_ln_fold item: rows = {rows} must be 1..{LORA_LNFOLD_MAX_ROWS} and K = {K} a positive multiple of 8")
    return (a, gamma, beta, a_out, s_out, c_out, rows | (K << 32))
LoraMergeDesc = _struct("LoraMergeDesc", _ptrs("items", "prefix") + _ints("n", "total"))
# slh_lora_merge_item: one row range of one stored matrix (include/sliders_hip.h)
LoraMergeItem = _struct("LoraMergeItem", _ptrs("base", "out", "u", "d", "c", "gamma", "beta", "bias", "lns", "lnb")
                        + _ints("n0", "rows", "N", "K", "R", "ldu", "ldd", "ld", "w_layout", "pad_"))
VaeSampleDesc = _struct("VaeSampleDesc", _ptrs("moments", "post_noise", "noise", "latent_f32", "noisy_f32", "noisy_bf16")
                        + _ints("batch", "hw") + [("scaling", c_f32), ("sqrt_alpha", c_f32), ("sqrt_one_minus_alpha", c_f32)]
                        + _ints("pad_"))

# opcodes (enum in sliders_hip.h)
OP_GEMM, OP_SKINNY, OP_GEMV, OP_GN_STATS, OP_GN_APPLY, OP_LAYERNORM, OP_ATTN_FWD, OP_TRANSPOSE_HEADS = range(1, 9)
OP_TEMBED, OP_CONV_IN, OP_ELEMENTWISE, OP_CFG_DDIM, OP_LOSS, OP_WGRAD, OP_ADAMW = range(9, 16)
OP_GN_BWD_STATS, OP_GN_BWD_APPLY, OP_LAYERNORM_BWD, OP_ATTN_BWD, OP_MEMSET = range(16, 21)
OP_LORA_CONV_DGRAD, OP_TEMB_LORA_BWD = 21, 22
OP_SGEMM, OP_GN32_STATS, OP_GN32_APPLY, OP_SOFTMAX32, OP_VAE_CONV_IN, OP_VAE_MOMENTS, OP_VAE_SAMPLE, OP_VAE_POST_QUANT = range(23, 31)
OP_LION = 31
OP_WGRAD_BATCH, OP_TRANSPOSE_BATCH, OP_GATHER16, OP_GN_FUSED = 32, 33, 34, 35
OP_LORA_LN_FOLD = 36
OP_LORA_MERGE = 38
OP_DDPM_EDIT = 39
OP_DDPM_EDIT_BLEND, OP_EPS_ABSDIFF = 40, 41
OP_XATTN_MAP = 42

EW_COPY, EW_ADD, EW_GEGLU_FWD, EW_GEGLU_BWD, EW_UPSAMPLE_BWD, EW_COLSUM = range(6)

# C entry point and descriptor per opcode: what call() launches and what load() holds against the library's own op table (slh_op_info)
_ENTRY = {
    OP_GEMM: ("slh_gemm", GemmDesc), OP_SKINNY: ("slh_skinny", SkinnyDesc), OP_GEMV: ("slh_gemv", GemvDesc),
    OP_GN_STATS: ("slh_gn_stats", GnDesc), OP_GN_APPLY: ("slh_gn_apply", GnDesc),
    OP_LAYERNORM: ("slh_layernorm", LnDesc), OP_ATTN_FWD: ("slh_attn_fwd", AttnDesc),
    OP_TRANSPOSE_HEADS: ("slh_transpose_heads", TransposeDesc), OP_TEMBED: ("slh_timestep_embed", TembedDesc),
    OP_CONV_IN: ("slh_conv_in", ConvInDesc), OP_ELEMENTWISE: ("slh_elementwise", EwDesc),
    OP_CFG_DDIM: ("slh_cfg_ddim", CfgDdimDesc), OP_LOSS: ("slh_guidance_loss", LossDesc),
    OP_WGRAD: ("slh_lora_wgrad", WgradDesc), OP_ADAMW: ("slh_adamw", AdamwDesc),
    OP_GN_BWD_STATS: ("slh_gn_bwd_stats", GnBwdDesc), OP_GN_BWD_APPLY: ("slh_gn_bwd_apply", GnBwdDesc),
    OP_LAYERNORM_BWD: ("slh_layernorm_bwd", LnBwdDesc), OP_ATTN_BWD: ("slh_attn_bwd", AttnBwdDesc), OP_MEMSET: ("slh_memset", MemsetDesc),
    OP_LORA_CONV_DGRAD: ("slh_lora_conv_dgrad", LoraCdgradDesc), OP_TEMB_LORA_BWD: ("slh_temb_lora_bwd", TembLoraBwdDesc),
    OP_SGEMM: ("slh_sgemm", SgemmDesc), OP_GN32_STATS: ("slh_gn32_stats", Gn32Desc), OP_GN32_APPLY: ("slh_gn32_apply", Gn32Desc),
    OP_SOFTMAX32: ("slh_softmax32", Softmax32Desc), OP_VAE_CONV_IN: ("slh_vae_conv_in", VaeConvDesc),
    OP_VAE_MOMENTS: ("slh_vae_moments", VaeConvDesc), OP_VAE_SAMPLE: ("slh_vae_sample", VaeSampleDesc),
    OP_VAE_POST_QUANT: ("slh_vae_post_quant", VaeConvDesc), OP_LION: ("slh_lion", LionDesc),
    OP_WGRAD_BATCH: ("slh_lora_wgrad_batch", BatchDesc), OP_TRANSPOSE_BATCH: ("slh_transpose_heads_batch", BatchDesc),
    OP_GATHER16: ("slh_gather16", Gather16Desc), OP_GN_FUSED: ("slh_gn_fused", GnDesc),
    OP_LORA_LN_FOLD: ("slh_lora_ln_fold", LoraLnFoldDesc), OP_LORA_MERGE: ("slh_lora_merge", LoraMergeDesc),
    OP_DDPM_EDIT: ("slh_ddpm_edit_step", DdpmEditDesc),
    OP_DDPM_EDIT_BLEND: ("slh_ddpm_edit_blend", DdpmEditBlendDesc), OP_EPS_ABSDIFF: ("slh_eps_absdiff", EpsAbsdiffDesc),
    OP_XATTN_MAP: ("slh_xattn_map", XattnMapDesc),
}

# every other export: name -> (restype, argtypes), applied once by load()
_P, _str = C.POINTER, C.c_char_p
_HOST_FNS = {
    "slh_version": (c_i32, []), "slh_last_error": (_str, []),
    "slh_run_program": (c_i32, [c_vp, c_i64, c_vp]), "slh_op_info": (c_i32, [c_i32, _P(c_i32), _P(_str), _P(c_i32)]),
    "slh_graph_capture": (c_i32, [c_vp, c_i64, _P(c_vp)]), "slh_graph_launch": (c_i32, [c_vp, c_vp]), "slh_graph_destroy": (c_i32, [c_vp]),
    "slh_gemm_kernel_name": (c_i32, [_P(GemmDesc), _str, c_i32]),
    "slh_gemm_launch_query": (c_i32, [_P(GemmDesc), _str, c_i32, _P(c_i32), _P(c_i32), _P(C.c_uint64)]),
    "slh_gemm_tile_ok": (c_i32, [_P(GemmDesc)]), "slh_gemm_ln_chunk_cols": (c_i32, [_P(GemmDesc)]),
    "slh_skinny_kernel_name": (c_i32, [_P(SkinnyDesc), _str, c_i32]), "slh_sgemm_form": (c_i32, [_P(SgemmDesc)]),
    "slh_attn_fwd_carries_touch": (c_i32, [_P(AttnDesc)]), "slh_attn_fwd_kernel_name": (c_i32, [_P(AttnDesc), _str, c_i32]),
    "slh_attn_bwd_kernel_names": (c_i32, [_P(AttnBwdDesc), _str, _str, c_i32]),
    "slh_gn_row_blocks": (c_i32, [c_i32, c_i32, c_i32]), "slh_gn_clusters": (c_i32, [c_i32]), "slh_gn32_row_blocks": (c_i32, [c_i32]),
    "slh_gn_fused_ok": (c_i32, [c_i32, c_i32, c_i32]),
    "slh_lora_wgrad_blocks": (c_i32, [_P(WgradDesc)]), "slh_lora_wgrad_single_blocks": (c_i32, [_P(WgradDesc)]),
    "slh_lora_wgrad_geometry": (c_i32, [_P(WgradDesc), c_i32, _P(c_i32)]),
    "slh_transpose_heads_blocks": (c_i32, [_P(TransposeDesc)]), "slh_lora_merge_blocks": (c_i32, [_P(LoraMergeItem)]),
}
# the step entry points that take (ptrs, dims, coef, stream): three flat arrays instead of a descriptor (_three_arrays calls them)
_HOST_FNS.update((name, (c_i32, [_P(c_vp), _P(c_i32), _P(c_f32), c_vp])) for name in (
    "slh_sigma_step", "slh_latent_blend", "slh_direction_threshold", "slh_eps_direction", "slh_eps_direction_momentum", "slh_edit_step2"))

EXPORTS = list(_HOST_FNS) + [name for name, _ in _ENTRY.values()]


class SlidersHipError(RuntimeError):
    pass


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libsliders_hip.so; raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SlidersHipError(
            f"{LIB_PATH} not found: the HIP extension is not built. There is no CPU fallback; run "
            f"`make -C {os.path.join(_HERE, 'csrc')}` (or __graft_entry__.build()).")
    # PyTorch-ROCm bundles its own libamdhip64.so.7; load it first so this library binds to the SAME HIP
    # runtime instance (streams and device pointers are shared with torch).  Loading /opt/rocm's copy first
    # leaves two runtimes in the process and every launch fails with "no ROCm-capable device is detected".
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    signatures = dict(_HOST_FNS)
    signatures.update((name, (c_i32, [_P(desc), c_vp])) for name, desc in _ENTRY.values())
    for name, (restype, argtypes) in signatures.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    # the library's op table, keyed by opcode, against this binding's
    theirs = {}
    op, entry, size = c_i32(), _str(), c_i32()
    for i in range(lib.slh_op_info(-1, None, None, None)):
        lib.slh_op_info(i, C.byref(op), C.byref(entry), C.byref(size))
        theirs[op.value] = (entry.value.decode(), size.value)
    if set(theirs) != set(_ENTRY):
        raise SlidersHipError(f"binding/library mismatch: opcodes only in the library {sorted(set(theirs) - set(_ENTRY))}, "
                              f"only in the binding {sorted(set(_ENTRY) - set(theirs))}")
    for opcode, (name, desc) in _ENTRY.items():
        if (name, C.sizeof(desc)) != theirs[opcode]:
            field = "entry" if name != theirs[opcode][0] else f"sizeof({desc.__name__})"
            raise SlidersHipError(f"binding/library mismatch: opcode {opcode} {field}: binding {(name, C.sizeof(desc))}, library {theirs[opcode]}")
    _lib = lib
    return lib


def last_error() -> str:
    return load().slh_last_error().decode()


def check(rc: int, what: str = ""):
    if rc != 0:
        raise SlidersHipError(f"{what} failed (rc={rc}): {last_error()}")


def _gn_workspace(row_blocks_fn: str, *shape):
    """(rows of the [rows][groups][2] fp32 partial-sum scratch, zeroed uint32 tickets) PER SAMPLE of a statistics launch with
    R = row_blocks_fn(*shape) row blocks (include/sliders_hip.h, slh_gn_desc)."""
    l = load()
    r = getattr(l, row_blocks_fn)(*shape)
    if r <= 0:
        raise SlidersHipError(f"{row_blocks_fn}{shape}: unsupported shape")
    c = l.slh_gn_clusters(r)
    return r + c, 1 + c


def gn_workspace(channels: int, hw: int, groups: int):
    """_gn_workspace of slh_gn_stats / slh_gn_bwd_stats"""
    return _gn_workspace("slh_gn_row_blocks", channels, hw, groups)


TILE_64x160 = 0x5425      # the 64 x 160 tile of csrc/gemm5.hip (bits 12-15 = 5: family; 4 ring slots; 2 x 5 blocks of 16 x 16 per wave)
TILE_128x256 = 0x7648     # four-wave tiles of csrc/gemm7.hip (bits 12-15 = 7; ring slots | X blocks | W blocks of 16 rows per wave)
TILE_128x160 = 0x7645
TILE_256x320 = 0x748A     # eight compute waves (gemm7w_kernel): GEGLU.proj as one round of 256 workgroups


def gemm_tile_ok(desc) -> bool:
    """slh_gemm_tile_ok: the tile named by desc.tile (0: the library's heuristic) can run this descriptor - every check of slh_gemm
    but the split-K workspace and ln_lora_s / ln_lora_c, which a caller provisions after choosing the tile"""
    return bool(load().slh_gemm_tile_ok(C.byref(desc)))


def gemm5_ok(desc) -> bool:
    """The 64 x 160 tile can run this descriptor: slh_gemm_tile_ok for desc.tile, or for TILE_64x160 where desc.tile is of another family"""
    from .tuning import tile_fields, tile_ok          # (tuning imports this module)
    return tile_ok(desc, desc.tile if tile_fields(desc.tile).family == 5 else TILE_64x160)


def gemm7_ok(desc) -> bool:
    """The tile of csrc/gemm7.hip named by desc.tile (0x7648 / 0x7645 / 0x748a) can run this descriptor (slh_gemm_tile_ok)"""
    from .tuning import tile_fields
    return tile_fields(desc.tile).family == 7 and gemm_tile_ok(desc)


def gemm_ln_chunk_cols(desc) -> int:
    """slh_gemm_ln_chunk_cols: width of the LayerNorm chunks desc's tile writes to desc.ln_out (80 or 64), 0 where it cannot"""
    return load().slh_gemm_ln_chunk_cols(C.byref(desc))


def gn_fused_ok(channels: int, hw: int, groups: int) -> int:
    """slh_gn_fused (statistics + normalisation in one launch) applies to this shape: 0 no, 1 the register-resident kernel for
    tiny tensors, 2 sibling workgroups over a cache-resident slab"""
    return int(load().slh_gn_fused_ok(channels, hw, groups))


def gn32_workspace(hw: int):
    """_gn_workspace of slh_gn32_stats"""
    return _gn_workspace("slh_gn32_row_blocks", hw)


_BATCH_KINDS = {OP_WGRAD_BATCH: ("slh_lora_wgrad_blocks", WgradDesc), OP_TRANSPOSE_BATCH: ("slh_transpose_heads_blocks", TransposeDesc)}


def batch_table(opcode: int, descs, device, arg: int = 0):
    """n problems of one kind -> (BatchDesc, tensors to keep alive): the descriptors packed into a device byte table and the
    int32 prefix sums of the workgroups each needs (include/sliders_hip.h, slh_batch_desc).  Every descriptor is validated by
    the library here, at plan time (slh_*_blocks); device = None builds a pointer-less descriptor for dry-run planning."""
    import torch
    fn_name, dtype = _BATCH_KINDS[opcode]
    fn = getattr(load(), fn_name)
    prefix = [0]
    slab_geom = 0
    if opcode == OP_WGRAD_BATCH:
        # slh_lora_wgrad_blocks takes the geometry from each descriptor's slabs, the kernel from the batch's: one choice per batch
        kinds = {bool(d.slabs) for d in descs}
        if len(kinds) > 1:
            raise SlidersHipError("slh_lora_wgrad_batch: the problems of one batch must all be built with slabs or all without")
        slab_geom = int(kinds.pop()) if kinds else 0
    for d in descs:
        assert isinstance(d, dtype)
        nb = fn(C.byref(d))         # host-side geometry only: also in dry-run planning (the arena is sized from it)
        if nb <= 0:
            raise SlidersHipError(f"{fn_name}: {last_error()}")
        prefix.append(prefix[-1] + nb)
    if device is None:
        bd = BatchDesc(table=0x1000, prefix=0x1000, n=len(descs), total=prefix[-1], arg=arg)
        bd.slab_geom = slab_geom
        return bd, ()
    raw = b"".join(bytes(d) for d in descs)
    table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
    pre = torch.tensor(prefix, dtype=torch.int32, device=device)
    bd = BatchDesc(table=table.data_ptr(), prefix=pre.data_ptr(), n=len(descs), total=prefix[-1], arg=arg)
    bd.slab_geom = slab_geom          # (a Python attribute, not a field: checked by check_batch before every launch / recording)
    return bd, (table, pre)


def check_batch(opcode: int, desc):
    """A weight-gradient batch carries slabs exactly when its table was built from descriptors with slabs (batch_table): prefix holds
    the workgroup counts of that geometry and the kernel picks its geometry from the batch's slabs - refuse a disagreement here, on
    the host, before anything is launched or recorded."""
    if opcode == OP_WGRAD_BATCH and isinstance(desc, BatchDesc):
        geom = getattr(desc, "slab_geom", None)
        if geom is None:
            raise SlidersHipError("slh_lora_wgrad_batch: build the batch descriptor with lib.batch_table (it records the table's geometry)")
        if bool(desc.slabs) != bool(geom):
            raise SlidersHipError(f"slh_lora_wgrad_batch: the table was built for the {'slab' if geom else 'atomic'} geometry, the batch "
                                  f"{'carries' if desc.slabs else 'has no'} slabs")


def merge_table(items, device):
    """slh_lora_merge items -> (LoraMergeDesc, tensors to keep alive).  Every item is validated by the library here
    (slh_lora_merge_blocks); the device table and the running sum of workgroups are built once and reused by every launch."""
    import torch
    l = load()
    prefix = [0]
    for it in items:
        nb = l.slh_lora_merge_blocks(C.byref(it))
        if nb <= 0:
            raise SlidersHipError(f"slh_lora_merge_blocks: {last_error()}")
        prefix.append(prefix[-1] + nb)
    table = torch.frombuffer(bytearray(b"".join(bytes(it) for it in items)), dtype=torch.uint8).to(device)
    pre = torch.tensor(prefix, dtype=torch.int32, device=device)
    return LoraMergeDesc(items=table.data_ptr(), prefix=pre.data_ptr(), n=len(items), total=prefix[-1]), (table, pre)


def wgrad_single_blocks(desc) -> int:
    """Workgroups (= slabs = tickets) of a stand-alone slh_lora_wgrad launch with the fixed-order reduction."""
    nb = load().slh_lora_wgrad_single_blocks(C.byref(desc))
    if nb <= 0:
        raise SlidersHipError(f"slh_lora_wgrad_single_blocks: {last_error()}")
    return nb


def wgrad_geometry(desc, kind: int):
    """slh_lora_wgrad_geometry: (gx, splits, taps, rows_per_block) of desc's problem for kind 0 (fp32 atomics), 1 (single launch with
    slabs) or 2 (inside a batch with slabs), from the library's one geometry function; shape fields only, no device needed."""
    out = (c_i32 * 4)()
    if load().slh_lora_wgrad_geometry(C.byref(desc), kind, out) != 0:
        raise SlidersHipError(f"slh_lora_wgrad_geometry: {last_error()}")
    return tuple(out)


def _kernel_names(query: str, desc, cap: int, bufs: int = 1) -> tuple:
    """One of the library's name queries: `bufs` kernel names of at most cap bytes each for desc, or the library's refusal raised."""
    lib = load()
    out = [C.create_string_buffer(cap) for _ in range(bufs)]
    rc = getattr(lib, query)(C.byref(desc), *out, cap)
    if rc != 0:
        raise SlidersHipError(f"{query} failed ({rc}): {lib.slh_last_error().decode()}")
    return tuple(b.value.decode() for b in out)


def skinny_kernel_name(desc) -> str:
    """slh_skinny_kernel_name: the instantiation slh_skinny would launch for this descriptor ('skinny<12,16>': accumulator rows, lanes
    per output row), named by the selection function slh_skinny launches through; raises for a descriptor slh_skinny refuses."""
    return _kernel_names("slh_skinny_kernel_name", desc, 64)[0]


SGEMM_FORMS = ("exact", "split<64>", "split<128>")      # SLH_SGEMM_EXACT / _SPLIT64 / _SPLIT128


def sgemm_form(desc) -> str:
    """slh_sgemm_form: the kernel slh_sgemm would launch for this descriptor - 'exact' (sgemm_kernel), 'split<64>' or 'split<128>'
    (sgemm_bf16x3_kernel<TM>) - as the selection function slh_sgemm launches through decides it; raises for a descriptor slh_sgemm
    refuses.  Shape fields only, no device needed."""
    rc = load().slh_sgemm_form(C.byref(desc))
    if not 0 <= rc < len(SGEMM_FORMS):
        raise SlidersHipError(f"slh_sgemm_form failed ({rc}): {last_error()}")
    return SGEMM_FORMS[rc]


def attn_carries_touch(desc) -> bool:
    """slh_attn_fwd_carries_touch: this attention launch runs the key-split form, whose idle workgroup slots can stream weights for a
    later product (slh_attn_desc.pf_*)"""
    return bool(load().slh_attn_fwd_carries_touch(C.byref(desc)))


def attn_fwd_kernel_name(desc) -> str:
    """slh_attn_fwd_kernel_name: the instantiation slh_attn_fwd would launch for this descriptor ('attn_fwd_kernel<4, 1, true>',
    'attn_fwd_ks_kernel'), named by the dispatch code itself; raises for a descriptor slh_attn_fwd refuses."""
    return _kernel_names("slh_attn_fwd_kernel_name", desc, 96)[0]


def attn_bwd_kernel_names(desc):
    """slh_attn_bwd_kernel_names: (dq, dkv) instantiations slh_attn_bwd would launch ('attn_bwd_dq_kernel<2>',
    'attn_bwd_dkv_kernel<2, 2>'; dkv is '' with need_dkv = 0); raises for a descriptor slh_attn_bwd refuses."""
    return _kernel_names("slh_attn_bwd_kernel_names", desc, 96, bufs=2)


def gemm_kernel_name(desc) -> str:
    """slh_gemm_kernel_name: the kernel instantiation slh_gemm would launch for this descriptor, spelled as rocprofv3 prints it
    (e.g. 'gemm8pb_kernel<1, 5, 0, false>').  The library runs its whole dispatch with the launch replaced by a record of the template
    it selected, so a new tile can never be mis-named here; raises (with the library's message) for a descriptor slh_gemm refuses."""
    return _kernel_names("slh_gemm_kernel_name", desc, 160)[0]


def gemm_launch_query(desc):
    """slh_gemm_launch_query: (kernel name, grid, block size, FNV-1a hash of the kernel's argument bytes) of the launch slh_gemm would
    make for this descriptor - a function of the descriptor alone, no device needed; raises for a descriptor slh_gemm refuses."""
    lib = load()
    buf, grid, block, h = C.create_string_buffer(160), c_i32(), c_i32(), C.c_uint64()
    rc = lib.slh_gemm_launch_query(C.byref(desc), buf, 160, C.byref(grid), C.byref(block), C.byref(h))
    if rc != 0:
        raise SlidersHipError(f"slh_gemm_launch_query failed ({rc}): {lib.slh_last_error().decode()}")
    return buf.value.decode(), grid.value, block.value, h.value


def call(opcode: int, desc, stream: int):
    """Launch one op directly (used by the per-kernel parity tests)."""
    lib = load()
    name, _ = _ENTRY[opcode]
    check_batch(opcode, desc)
    check(getattr(lib, name)(C.byref(desc), c_vp(stream)), name)


def _three_arrays(name: str, stream: int, ptrs, dims, coef=()):
    """One (ptrs, dims, coef, stream) entry point: device addresses, int32 dimensions, fp32 coefficients (rounded to fp32 here, as the
    kernels read them; none: NULL)."""
    coef = (c_f32 * len(coef))(*coef) if coef else None
    check(getattr(load(), name)((c_vp * len(ptrs))(*ptrs), (c_i32 * len(dims))(*dims), coef, c_vp(stream)), name)


def sigma_step(stream: int, *, eps: int, x: int, out: int, nb: int, chw: int, kind: int, p: float, q: float, sigma: float = 0.0,
               a: float = 1.0, c=(0.0,), c_n: float = 0.0, s_next: float = 1.0, guidance: float = 0.0, single: bool = False,
               eps_text: int = 0, hist=(), noise: int = 0, hist_out: int = 0, in_bf16: int = 0, in2_bf16: int = 0):
    """slh_sigma_step (include/sliders_hip.h): one launch of the fp32 sampler step.  Pointers are device addresses (0: absent); hist:
    the addresses of H[1..n_hist], newest first; c: c[0..n_hist] (the coefficients beyond are passed as 0); the other scalars are
    rounded to fp32 here, as the kernel reads them."""
    hist, c = tuple(hist), tuple(c)
    if len(hist) > 3 or len(c) > 4:
        raise SlidersHipError(f"slh_sigma_step: {len(hist)} history buffers, {len(c)} coefficients: at most 3 and 4")
    _three_arrays("slh_sigma_step", stream, (eps, eps_text, x, *hist, *(0,) * (3 - len(hist)), noise, out, hist_out, in_bf16, in2_bf16),
                  (nb, chw, len(hist), kind, int(bool(single))), (p, q, sigma, a, *c, *(0.0,) * (4 - len(c)), c_n, s_next, guidance))


def latent_blend(stream: int, *, e: int, keep: int, mask: int, out: int, nb: int, chw: int, hw: int, fp32: bool, s_next: float = 1.0,
                 in_bf16: int = 0, in2_bf16: int = 0):
    """slh_latent_blend (include/sliders_hip.h): one launch of a localised sampling step's blend, out = keep where the mask is 0, e where
    it is 1, keep + m (e - keep) between.  Pointers are device addresses (0: absent); fp32: e / keep / out are fp32 and the bf16 copies
    are rne(out * s_next) (s_next rounded to fp32 here, as the kernel reads it), else they are bf16 and the copies are out's bits."""
    _three_arrays("slh_latent_blend", stream, (e, keep, mask, out, in_bf16, in2_bf16), (nb, chw, hw, 1 if fp32 else 0), (s_next,))


def edit_step2(stream: int, *, eps: int, x: int, resid: int, out: int, nb: int, chw: int, hw: int, mode: int, guidance: float,
               c_sqrt_beta_t: float, c_inv_sqrt_alpha_t: float, c_sqrt_alpha_t: float, c_sqrt_alpha_prev: float, c_dir: float,
               c_corr: float = 0.0, v_prediction: int = 0, eps_text: int = 0, x0_prev: int = 0, target: int = 0, keep: int = 0, mask: int = 0,
               x0_out: int = 0, out_bf16: int = 0, out2_bf16: int = 0):
    """slh_edit_step2 (include/sliders_hip.h): one launch of the second-order edit step.  Pointers are device addresses (0: absent);
    x0_prev = 0 is a first-order step and c_corr is not read; mode 0 writes resid from target, mode 1 reads it; keep and mask (mode 1)
    blend the result.  The scalars are rounded to fp32 here, as the kernel reads them."""
    _three_arrays("slh_edit_step2", stream, (eps, eps_text, x, x0_prev, target, resid, keep, mask, out, x0_out, out_bf16, out2_bf16),
                  (nb, chw, hw, mode, v_prediction),
                  (guidance, c_sqrt_beta_t, c_inv_sqrt_alpha_t, c_sqrt_alpha_t, c_sqrt_alpha_prev, c_dir, c_corr))


MAX_DIRECTIONS = 3          # prompt pairs per slh_direction_threshold / slh_eps_direction[_momentum] call


def _direction_rows(what: str, pos, neg, per_direction, counted: str, cast):
    """(pos, neg, per_direction, K), each of the three padded with zeros to MAX_DIRECTIONS; per_direction: K n_keep values (cast: int) or
    K coefficients (float)"""
    pos, neg, per_direction = tuple(pos), tuple(neg), tuple(cast(v) for v in per_direction)
    K = len(pos)
    if len(neg) != K or K > MAX_DIRECTIONS:
        raise SlidersHipError(f"{what}: {K} pos and {len(neg)} neg rows: the same number of each, at most {MAX_DIRECTIONS}")
    if len(per_direction) != K:
        raise SlidersHipError(f"{what}: {len(per_direction)} {counted} for {K} directions")
    pad = MAX_DIRECTIONS - K
    return pos + (0,) * pad, neg + (0,) * pad, per_direction + (cast(),) * pad, K


def direction_threshold(stream: int, *, pos, neg, thr: int, n_keep, nb: int, chw: int, hw: int):
    """slh_direction_threshold (include/sliders_hip.h): thr[b][k][ch] (int32, [nb][K][chw / hw]) = the n_keep[k]-th largest key of
    e+_k - e-_k over the hw pixels of channel ch of sample b.  pos, neg: K device addresses each (bf16 [nb][chw]); n_keep: K counts."""
    pos, neg, n_keep, K = _direction_rows("slh_direction_threshold", pos, neg, n_keep, "n_keep values", int)
    _three_arrays("slh_direction_threshold", stream, (*pos, *neg, thr), (nb, chw, hw, K, *n_keep))


def eps_direction(stream: int, *, t: int, out: int, pos, neg, c, nb: int, chw: int, hw: int, thr: int = 0):
    """slh_eps_direction (include/sliders_hip.h): out = rne_bf16(t + sum_k c[k] keep_k (e+_k - e-_k)), the guided text row a step kernel
    reads through eps_text.  pos, neg: K device addresses each; c: K coefficients (rounded to fp32 here, as the kernel reads them; a
    zero skips its term); thr: what slh_direction_threshold wrote, 0: every element is kept."""
    pos, neg, c, K = _direction_rows("slh_eps_direction", pos, neg, c, "coefficients", float)
    _three_arrays("slh_eps_direction", stream, (t, out, *pos, *neg, thr), (nb, chw, hw, K), c)


def eps_direction_momentum(stream: int, *, t: int, out: int, pos, neg, c, mom_in: int, mom_out: int, s_m: float, beta: float, nb: int,
                           chw: int, hw: int, thr: int = 0):
    """slh_eps_direction_momentum (include/sliders_hip.h): slh_eps_direction with the momentum state nu (fp32 [nb][chw]) read from mom_in:
    out = rne_bf16(t + sum_k c[k] keep_k d_k + s_m nu), mom_out = beta nu + (1 - beta) (sum_k c[k] keep_k d_k + s_m nu).  mom_out may be
    mom_in.  1 - beta is formed here in double and rounded once to fp32, as the kernel reads it; s_m == 0 is refused (eps_direction)."""
    pos, neg, c, K = _direction_rows("slh_eps_direction_momentum", pos, neg, c, "coefficients", float)
    _three_arrays("slh_eps_direction_momentum", stream, (t, out, *pos, *neg, thr, mom_in, mom_out), (nb, chw, hw, K),
                  (*c, s_m, beta, one_minus(beta)))


def one_minus(beta: float) -> float:
    """omb of slh_eps_direction_momentum: 1 - beta in double (beta as given, not its fp32 rounding); ctypes rounds it once to fp32"""
    return 1.0 - float(beta)


_GRAPHS_ON = os.environ.get("SLIDERS_HIPGRAPH", "1") != "0"


class Program:
    """Flat command buffer replayed by slh_run_program with one C call - or, once it has been replayed GRAPH_AFTER times
    unchanged and is long enough to matter, as one hipGraph submission (slh_graph_capture / slh_graph_launch).
    SLIDERS_HIPGRAPH=0 keeps plain launches."""

    GRAPH_AFTER = 2          # eager replays before capture (first runs also load the code objects)
    GRAPH_MIN_OPS = 64

    def __init__(self):
        self._chunks = []
        self.n_ops = 0
        self._buf = None
        self.op_names = []
        self.ops = []          # (opcode, descriptor) kept for per-op timing / tuning tools
        self._graphs = None    # captured graph handle
        self._runs = 0

    def _drop_graphs(self):
        if self._graphs is not None:
            load().slh_graph_destroy(self._graphs)
        self._graphs = None
        self._runs = 0

    def __del__(self):
        try:
            if self._graphs and _lib is not None:
                self._drop_graphs()
        except Exception:
            pass

    def add(self, opcode: int, desc, name: str = ""):
        check_batch(opcode, desc)
        raw = bytes(desc)
        pad = (-len(raw)) % 8
        hdr = C.c_int32 * 2
        self._chunks.append(bytes(hdr(opcode, len(raw))) + raw + b"\0" * pad)
        self.n_ops += 1
        self.op_names.append(name)
        self.ops.append((opcode, desc))
        self._buf = None
        if self._graphs:
            self._drop_graphs()

    def memset(self, ptr: int, nbytes: int, value: int = 0, name: str = "memset"):
        self.add(OP_MEMSET, MemsetDesc(ptr=ptr, nbytes=nbytes, value=value, pad=0), name)

    def extend(self, other: "Program"):
        self._chunks.extend(other._chunks)
        self.ops.extend(other.ops)
        self.n_ops += other.n_ops
        self.op_names.extend(other.op_names)
        self._buf = None
        if self._graphs:
            self._drop_graphs()

    def finalize(self):
        if self._buf is None:
            data = b"".join(self._chunks)
            self._buf = C.create_string_buffer(data, len(data))
        return self._buf

    def capture(self) -> bool:
        """Capture the graph now instead of after GRAPH_AFTER plain replays (recording launches nothing).  For programs
        whose kernels have all run before: the trainer's per-step variants of a pass it has already replayed."""
        if self._graphs is None and self.n_ops >= self.GRAPH_MIN_OPS and _GRAPHS_ON:
            buf = self.finalize()
            h = c_vp()
            check(load().slh_graph_capture(C.cast(buf, c_vp), len(buf), C.byref(h)), "slh_graph_capture")
            self._graphs = h
        return self._graphs is not None

    def run(self, stream: int, graph: bool = True):
        buf = self.finalize()
        lib = load()
        if graph and self.n_ops >= self.GRAPH_MIN_OPS and _GRAPHS_ON:
            g = self._graphs
            if g is None and self._runs >= self.GRAPH_AFTER:
                self.capture()
                g = self._graphs
            if g is not None:
                check(lib.slh_graph_launch(g, c_vp(stream)), "slh_graph_launch")
                return
        self._runs += 1
        check(lib.slh_run_program(C.cast(buf, c_vp), len(buf), c_vp(stream)), "slh_run_program")
