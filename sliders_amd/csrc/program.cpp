// Command-buffer executor: the host planner (sliders_amd/plan.py) flattens one UNet forward / backward /
// optimizer step into a byte buffer of {opcode, nbytes, descriptor} records; this walks it and launches every
// kernel on the caller's stream with no per-op host<->Python round trip (the reference pays one Python
// dispatch per torch op: ~1.2k per UNet forward).  The launches are plain stream work, so the
// caller may also capture a whole program into a hipGraph.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/sliders_hip.h"

void slh_set_error(const char* fmt, ...);

namespace {
// SLH_OP_MEMSET is a kernel of this library, not hipMemsetAsync: inside a captured hipGraph the runtime's memset node is a
// blit whose arguments live in the launch stream's blit ring, and replays on the legacy default stream were observed to zero
// the wrong bytes once other blits (torch fill_ / copies) had gone through that ring in between (round-4 notes).
__global__ void fill_kernel(unsigned char* p, unsigned v4, long n, int head) {
    // [0, head) bytes up to the first 16-byte boundary and the tail: thread 0's; the aligned middle: one uint4 per thread
    const long i = head + ((long)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (i + 16 <= n) *(uint4*)(p + i) = uint4{v4, v4, v4, v4};
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (long j = 0; j < head; ++j) p[j] = (unsigned char)v4;
        for (long j = head + ((n - head) & ~15L); j < n; ++j) p[j] = (unsigned char)v4;
    }
}
inline int fill_bytes(void* ptr, int value, long n, hipStream_t s) {
    if (n <= 0) return 0;
    long head = (long)((16 - ((uintptr_t)ptr & 15)) & 15);
    if (head > n) head = n;
    const unsigned b = (unsigned)value & 0xffu, v4 = b * 0x01010101u;
    const long threads = (n - head) / 16 + 1;
    fill_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>((unsigned char*)ptr, v4, n, (int)head);
    if (hipGetLastError() != hipSuccess) { slh_set_error("slh_run_program: memset launch failed"); return -2; }
    return 0;
}

template <typename T>
inline int run_desc(const unsigned char* p, int32_t nbytes, int (*fn)(const T*, slh_stream_t), slh_stream_t s,
                    const char* name) {
    if (nbytes != (int32_t)sizeof(T)) {
        slh_set_error("slh_run_program: %s descriptor is %d bytes, library expects %d", name, nbytes, (int)sizeof(T));
        return -3;
    }
    T d;
    memcpy(&d, p, sizeof(T));
    return fn(&d, s);
}
}  // namespace

extern "C" int slh_run_program(const void* program, int64_t nbytes, slh_stream_t stream) {
    const unsigned char* p = (const unsigned char*)program;
    const unsigned char* end = p + nbytes;
    int idx = 0;
    int rc_all = 0;
    while (p < end) {
        if (end - p < 8) { slh_set_error("slh_run_program: truncated record header at op %d", idx); return -3; }
        int32_t hdr[2];
        memcpy(hdr, p, 8);
        p += 8;
        const int32_t op = hdr[0], sz = hdr[1];
        if (sz < 0 || end - p < sz) { slh_set_error("slh_run_program: truncated record at op %d", idx); return -3; }
        int rc = 0;
        switch (op) {
            case SLH_OP_GEMM: rc = run_desc<slh_gemm_desc>(p, sz, slh_gemm, stream, "gemm"); break;
            case SLH_OP_SKINNY: rc = run_desc<slh_skinny_desc>(p, sz, slh_skinny, stream, "skinny"); break;
            case SLH_OP_GEMV: rc = run_desc<slh_gemv_desc>(p, sz, slh_gemv, stream, "gemv"); break;
            case SLH_OP_GN_STATS: rc = run_desc<slh_gn_desc>(p, sz, slh_gn_stats, stream, "gn_stats"); break;
            case SLH_OP_GN_APPLY: rc = run_desc<slh_gn_desc>(p, sz, slh_gn_apply, stream, "gn_apply"); break;
            case SLH_OP_GN_FUSED: rc = run_desc<slh_gn_desc>(p, sz, slh_gn_fused, stream, "gn_fused"); break;
            case SLH_OP_LORA_LN_FOLD: rc = run_desc<slh_lora_lnfold_desc>(p, sz, slh_lora_ln_fold, stream, "lora_ln_fold"); break;
            case SLH_OP_LORA_MERGE: rc = run_desc<slh_lora_merge_desc>(p, sz, slh_lora_merge, stream, "lora_merge"); break;
            case SLH_OP_LAYERNORM: rc = run_desc<slh_ln_desc>(p, sz, slh_layernorm, stream, "layernorm"); break;
            case SLH_OP_ATTN_FWD: rc = run_desc<slh_attn_desc>(p, sz, slh_attn_fwd, stream, "attn_fwd"); break;
            case SLH_OP_TRANSPOSE_HEADS:
                rc = run_desc<slh_transpose_desc>(p, sz, slh_transpose_heads, stream, "transpose_heads"); break;
            case SLH_OP_TEMBED: rc = run_desc<slh_tembed_desc>(p, sz, slh_timestep_embed, stream, "tembed"); break;
            case SLH_OP_CONV_IN: rc = run_desc<slh_convin_desc>(p, sz, slh_conv_in, stream, "conv_in"); break;
            case SLH_OP_ELEMENTWISE: rc = run_desc<slh_ew_desc>(p, sz, slh_elementwise, stream, "elementwise"); break;
            case SLH_OP_CFG_DDIM: rc = run_desc<slh_cfg_ddim_desc>(p, sz, slh_cfg_ddim, stream, "cfg_ddim"); break;
            case SLH_OP_DDPM_EDIT: rc = run_desc<slh_ddpm_edit_desc>(p, sz, slh_ddpm_edit_step, stream, "ddpm_edit"); break;
            case SLH_OP_DDPM_EDIT_BLEND:
                rc = run_desc<slh_ddpm_edit_blend_desc>(p, sz, slh_ddpm_edit_blend, stream, "ddpm_edit_blend"); break;
            case SLH_OP_EPS_ABSDIFF: rc = run_desc<slh_eps_absdiff_desc>(p, sz, slh_eps_absdiff, stream, "eps_absdiff"); break;
            case SLH_OP_XATTN_MAP: rc = run_desc<slh_xattn_map_desc>(p, sz, slh_xattn_map, stream, "xattn_map"); break;
            case SLH_OP_LOSS: rc = run_desc<slh_loss_desc>(p, sz, slh_guidance_loss, stream, "loss"); break;
            case SLH_OP_WGRAD: rc = run_desc<slh_wgrad_desc>(p, sz, slh_lora_wgrad, stream, "wgrad"); break;
            case SLH_OP_ADAMW: rc = run_desc<slh_adamw_desc>(p, sz, slh_adamw, stream, "adamw"); break;
            case SLH_OP_LION: rc = run_desc<slh_lion_desc>(p, sz, slh_lion, stream, "lion"); break;
            case SLH_OP_GN_BWD_STATS:
                rc = run_desc<slh_gn_bwd_desc>(p, sz, slh_gn_bwd_stats, stream, "gn_bwd_stats"); break;
            case SLH_OP_GN_BWD_APPLY:
                rc = run_desc<slh_gn_bwd_desc>(p, sz, slh_gn_bwd_apply, stream, "gn_bwd_apply"); break;
            case SLH_OP_LAYERNORM_BWD:
                rc = run_desc<slh_ln_bwd_desc>(p, sz, slh_layernorm_bwd, stream, "layernorm_bwd"); break;
            case SLH_OP_ATTN_BWD: rc = run_desc<slh_attn_bwd_desc>(p, sz, slh_attn_bwd, stream, "attn_bwd"); break;
            case SLH_OP_LORA_CONV_DGRAD:
                rc = run_desc<slh_lora_cdgrad_desc>(p, sz, slh_lora_conv_dgrad, stream, "lora_conv_dgrad"); break;
            case SLH_OP_TEMB_LORA_BWD:
                rc = run_desc<slh_temb_lora_bwd_desc>(p, sz, slh_temb_lora_bwd, stream, "temb_lora_bwd"); break;
            case SLH_OP_SGEMM: rc = run_desc<slh_sgemm_desc>(p, sz, slh_sgemm, stream, "sgemm"); break;
            case SLH_OP_GN32_STATS: rc = run_desc<slh_gn32_desc>(p, sz, slh_gn32_stats, stream, "gn32_stats"); break;
            case SLH_OP_GN32_APPLY: rc = run_desc<slh_gn32_desc>(p, sz, slh_gn32_apply, stream, "gn32_apply"); break;
            case SLH_OP_SOFTMAX32: rc = run_desc<slh_softmax32_desc>(p, sz, slh_softmax32, stream, "softmax32"); break;
            case SLH_OP_VAE_CONV_IN: rc = run_desc<slh_vae_conv_desc>(p, sz, slh_vae_conv_in, stream, "vae_conv_in"); break;
            case SLH_OP_VAE_MOMENTS: rc = run_desc<slh_vae_conv_desc>(p, sz, slh_vae_moments, stream, "vae_moments"); break;
            case SLH_OP_VAE_POST_QUANT: rc = run_desc<slh_vae_conv_desc>(p, sz, slh_vae_post_quant, stream, "vae_post_quant"); break;
            case SLH_OP_VAE_SAMPLE: rc = run_desc<slh_vae_sample_desc>(p, sz, slh_vae_sample, stream, "vae_sample"); break;
            case SLH_OP_WGRAD_BATCH: rc = run_desc<slh_batch_desc>(p, sz, slh_lora_wgrad_batch, stream, "wgrad_batch"); break;
            case SLH_OP_TRANSPOSE_BATCH: rc = run_desc<slh_batch_desc>(p, sz, slh_transpose_heads_batch, stream, "transpose_batch"); break;
            case SLH_OP_GATHER16: rc = run_desc<slh_gather16_desc>(p, sz, slh_gather16, stream, "gather16"); break;
            case SLH_OP_MEMSET: {
                if (sz != (int32_t)sizeof(slh_memset_desc)) { slh_set_error("slh_run_program: memset desc size"); return -3; }
                slh_memset_desc d;
                memcpy(&d, p, sizeof(d));
                rc = fill_bytes(d.ptr, d.value, (long)d.nbytes, (hipStream_t)stream);
                break;
            }
            default:
                slh_set_error("slh_run_program: unknown opcode %d at op %d", op, idx);
                return -3;
        }
        if (rc != 0) { rc_all = rc; break; }
        p += (sz + 7) & ~7;
        ++idx;
    }
    return rc_all;
}

// ---- hipGraph replay ------------------------------------------------------------------------------------------------
// A finalized command buffer is static (descriptors are passed to the kernels by value, everything that changes between
// replays - latents, timestep, adapter scale, adapter weights - lives behind device pointers), so the ~1000 launches of
// a UNet pass can be recorded once and re-submitted as one graph: no per-launch API call, argument marshalling or
// descriptor validation on the host, and the command processor sees the whole chain up front.
struct slh_graph_ {
    hipGraph_t graph;
    hipGraphExec_t exec;
};

extern "C" int slh_graph_capture(const void* program, int64_t nbytes, void** out) {
    if (!out) { slh_set_error("slh_graph_capture: null out"); return -3; }
    *out = nullptr;
    // recorded on a private stream (the caller's may be the legacy default stream, which cannot capture); the graph
    // itself is not tied to a stream
    hipStream_t s = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) { slh_set_error("slh_graph_capture: stream create: %s", hipGetErrorString(e)); return -2; }
    e = hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed);
    if (e != hipSuccess) {
        (void)hipStreamDestroy(s);
        slh_set_error("slh_graph_capture: begin capture: %s", hipGetErrorString(e));
        return -2;
    }
    const int rc = slh_run_program(program, nbytes, (slh_stream_t)s);
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(s, &g);
    (void)hipStreamDestroy(s);
    if (rc != 0) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess || !g) { slh_set_error("slh_graph_capture: end capture: %s", hipGetErrorString(e)); return -2; }
    hipGraphExec_t x = nullptr;
    e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(g);
        slh_set_error("slh_graph_capture: instantiate: %s", hipGetErrorString(e));
        return -2;
    }
    slh_graph_* h = new slh_graph_{g, x};
    *out = h;
    return 0;
}

extern "C" int slh_graph_launch(void* graph, slh_stream_t stream) {
    if (!graph) { slh_set_error("slh_graph_launch: null graph"); return -3; }
    hipError_t e = hipGraphLaunch(((slh_graph_*)graph)->exec, (hipStream_t)stream);
    if (e != hipSuccess) { slh_set_error("slh_graph_launch: %s", hipGetErrorString(e)); return -2; }
    return 0;
}

extern "C" int slh_graph_destroy(void* graph) {
    if (!graph) return 0;
    slh_graph_* h = (slh_graph_*)graph;
    (void)hipGraphExecDestroy(h->exec);
    (void)hipGraphDestroy(h->graph);
    delete h;
    return 0;
}

extern "C" int slh_desc_sizes(int32_t* out, int32_t cap) {
    const int32_t sizes[] = {
        (int32_t)sizeof(slh_gemm_desc),     (int32_t)sizeof(slh_skinny_desc),   (int32_t)sizeof(slh_gemv_desc),
        (int32_t)sizeof(slh_gn_desc),       (int32_t)sizeof(slh_gn_bwd_desc),   (int32_t)sizeof(slh_ln_desc),
        (int32_t)sizeof(slh_ln_bwd_desc),   (int32_t)sizeof(slh_attn_desc),     (int32_t)sizeof(slh_transpose_desc),
        (int32_t)sizeof(slh_attn_bwd_desc), (int32_t)sizeof(slh_tembed_desc),   (int32_t)sizeof(slh_convin_desc),
        (int32_t)sizeof(slh_ew_desc),       (int32_t)sizeof(slh_cfg_ddim_desc), (int32_t)sizeof(slh_loss_desc),
        (int32_t)sizeof(slh_wgrad_desc),    (int32_t)sizeof(slh_adamw_desc),    (int32_t)sizeof(slh_memset_desc),
        (int32_t)sizeof(slh_lora_cdgrad_desc), (int32_t)sizeof(slh_temb_lora_bwd_desc),
        (int32_t)sizeof(slh_sgemm_desc),    (int32_t)sizeof(slh_gn32_desc),     (int32_t)sizeof(slh_softmax32_desc),
        (int32_t)sizeof(slh_vae_conv_desc), (int32_t)sizeof(slh_vae_sample_desc), (int32_t)sizeof(slh_lion_desc),
        (int32_t)sizeof(slh_batch_desc),    (int32_t)sizeof(slh_gather16_desc), (int32_t)sizeof(slh_lora_lnfold_desc),
        (int32_t)sizeof(slh_lora_merge_desc), (int32_t)sizeof(slh_ddpm_edit_desc),
        (int32_t)sizeof(slh_ddpm_edit_blend_desc), (int32_t)sizeof(slh_eps_absdiff_desc), (int32_t)sizeof(slh_xattn_map_desc)};
    const int n = (int)(sizeof(sizes) / sizeof(sizes[0]));
    for (int i = 0; i < n && i < cap; ++i) out[i] = sizes[i];
    return n;
}
