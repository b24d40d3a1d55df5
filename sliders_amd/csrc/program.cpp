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
}  // namespace

extern "C" int slh_memset(const slh_memset_desc* d, slh_stream_t stream) {
    if (!d) { slh_set_error("slh_memset: null descriptor"); return -3; }
    const long n = (long)d->nbytes;
    if (n <= 0) return 0;
    if (!d->ptr) { slh_set_error("slh_memset: null ptr with nbytes = %ld", n); return -3; }
    long head = (long)((16 - ((uintptr_t)d->ptr & 15)) & 15);
    if (head > n) head = n;
    const unsigned b = (unsigned)d->value & 0xffu, v4 = b * 0x01010101u;
    const long threads = (n - head) / 16 + 1;
    hipStream_t s = (hipStream_t)stream;
    fill_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>((unsigned char*)d->ptr, v4, n, (int)head);
    if (hipGetLastError() != hipSuccess) { slh_set_error("slh_memset: launch failed"); return -2; }
    return 0;
}

namespace {
// The op table: THE association of an opcode with its entry point and its descriptor.  The executor dispatches through it and
// slh_op_info reports it, so a binding checks itself against the rows the executor runs.  A new op is one row here (plus its
// enumerator, struct and prototype in sliders_hip.h).
struct OpRow {
    int32_t opcode;
    const char* entry;
    int32_t desc_size;
    int (*run)(const unsigned char* rec, int32_t nbytes, slh_stream_t s, const char* entry);
};

template <typename T, int (*Fn)(const T*, slh_stream_t)>
int run_desc(const unsigned char* rec, int32_t nbytes, slh_stream_t s, const char* entry) {
    if (nbytes != (int32_t)sizeof(T)) {
        slh_set_error("slh_run_program: %s descriptor is %d bytes, library expects %d", entry, nbytes, (int)sizeof(T));
        return -3;
    }
    T d;
    memcpy(&d, rec, sizeof(T));
    return Fn(&d, s);
}

#define SLH_OP_ROW(op, fn, desc) {op, #fn, (int32_t)sizeof(desc), run_desc<desc, fn>}
constexpr OpRow kOps[] = {
    SLH_OP_ROW(SLH_OP_GEMM, slh_gemm, slh_gemm_desc),
    SLH_OP_ROW(SLH_OP_SKINNY, slh_skinny, slh_skinny_desc),
    SLH_OP_ROW(SLH_OP_GEMV, slh_gemv, slh_gemv_desc),
    SLH_OP_ROW(SLH_OP_GN_STATS, slh_gn_stats, slh_gn_desc),
    SLH_OP_ROW(SLH_OP_GN_APPLY, slh_gn_apply, slh_gn_desc),
    SLH_OP_ROW(SLH_OP_LAYERNORM, slh_layernorm, slh_ln_desc),
    SLH_OP_ROW(SLH_OP_ATTN_FWD, slh_attn_fwd, slh_attn_desc),
    SLH_OP_ROW(SLH_OP_TRANSPOSE_HEADS, slh_transpose_heads, slh_transpose_desc),
    SLH_OP_ROW(SLH_OP_TEMBED, slh_timestep_embed, slh_tembed_desc),
    SLH_OP_ROW(SLH_OP_CONV_IN, slh_conv_in, slh_convin_desc),
    SLH_OP_ROW(SLH_OP_ELEMENTWISE, slh_elementwise, slh_ew_desc),
    SLH_OP_ROW(SLH_OP_CFG_DDIM, slh_cfg_ddim, slh_cfg_ddim_desc),
    SLH_OP_ROW(SLH_OP_LOSS, slh_guidance_loss, slh_loss_desc),
    SLH_OP_ROW(SLH_OP_WGRAD, slh_lora_wgrad, slh_wgrad_desc),
    SLH_OP_ROW(SLH_OP_ADAMW, slh_adamw, slh_adamw_desc),
    SLH_OP_ROW(SLH_OP_GN_BWD_STATS, slh_gn_bwd_stats, slh_gn_bwd_desc),
    SLH_OP_ROW(SLH_OP_GN_BWD_APPLY, slh_gn_bwd_apply, slh_gn_bwd_desc),
    SLH_OP_ROW(SLH_OP_LAYERNORM_BWD, slh_layernorm_bwd, slh_ln_bwd_desc),
    SLH_OP_ROW(SLH_OP_ATTN_BWD, slh_attn_bwd, slh_attn_bwd_desc),
    SLH_OP_ROW(SLH_OP_MEMSET, slh_memset, slh_memset_desc),
    SLH_OP_ROW(SLH_OP_LORA_CONV_DGRAD, slh_lora_conv_dgrad, slh_lora_cdgrad_desc),
    SLH_OP_ROW(SLH_OP_TEMB_LORA_BWD, slh_temb_lora_bwd, slh_temb_lora_bwd_desc),
    SLH_OP_ROW(SLH_OP_SGEMM, slh_sgemm, slh_sgemm_desc),
    SLH_OP_ROW(SLH_OP_GN32_STATS, slh_gn32_stats, slh_gn32_desc),
    SLH_OP_ROW(SLH_OP_GN32_APPLY, slh_gn32_apply, slh_gn32_desc),
    SLH_OP_ROW(SLH_OP_SOFTMAX32, slh_softmax32, slh_softmax32_desc),
    SLH_OP_ROW(SLH_OP_VAE_CONV_IN, slh_vae_conv_in, slh_vae_conv_desc),
    SLH_OP_ROW(SLH_OP_VAE_MOMENTS, slh_vae_moments, slh_vae_conv_desc),
    SLH_OP_ROW(SLH_OP_VAE_SAMPLE, slh_vae_sample, slh_vae_sample_desc),
    SLH_OP_ROW(SLH_OP_VAE_POST_QUANT, slh_vae_post_quant, slh_vae_conv_desc),
    SLH_OP_ROW(SLH_OP_LION, slh_lion, slh_lion_desc),
    SLH_OP_ROW(SLH_OP_WGRAD_BATCH, slh_lora_wgrad_batch, slh_batch_desc),
    SLH_OP_ROW(SLH_OP_TRANSPOSE_BATCH, slh_transpose_heads_batch, slh_batch_desc),
    SLH_OP_ROW(SLH_OP_GATHER16, slh_gather16, slh_gather16_desc),
    SLH_OP_ROW(SLH_OP_GN_FUSED, slh_gn_fused, slh_gn_desc),
    SLH_OP_ROW(SLH_OP_LORA_LN_FOLD, slh_lora_ln_fold, slh_lora_lnfold_desc),
    SLH_OP_ROW(SLH_OP_LORA_MERGE, slh_lora_merge, slh_lora_merge_desc),
    SLH_OP_ROW(SLH_OP_DDPM_EDIT, slh_ddpm_edit_step, slh_ddpm_edit_desc),
    SLH_OP_ROW(SLH_OP_DDPM_EDIT_BLEND, slh_ddpm_edit_blend, slh_ddpm_edit_blend_desc),
    SLH_OP_ROW(SLH_OP_EPS_ABSDIFF, slh_eps_absdiff, slh_eps_absdiff_desc),
    SLH_OP_ROW(SLH_OP_XATTN_MAP, slh_xattn_map, slh_xattn_map_desc),
};
#undef SLH_OP_ROW
constexpr int kNumOps = (int)(sizeof(kOps) / sizeof(kOps[0]));

// opcode -> row, filled once: the executor pays one indexed load per record
constexpr int kOpSlots = 64;
constexpr bool opcodes_fit() {
    for (const OpRow& r : kOps)
        if (r.opcode <= 0 || r.opcode >= kOpSlots) return false;
    return true;
}
static_assert(opcodes_fit(), "an SLH_OP_* value outside (0, kOpSlots): widen kOpSlots");
struct OpIndex {
    const OpRow* at[kOpSlots] = {};
    OpIndex() { for (const OpRow& r : kOps) at[r.opcode] = &r; }
};
}  // namespace

extern "C" int slh_op_info(int index, int32_t* opcode, const char** entry, int32_t* desc_size) {
    if (index >= 0 && index < kNumOps) {
        if (opcode) *opcode = kOps[index].opcode;
        if (entry) *entry = kOps[index].entry;
        if (desc_size) *desc_size = kOps[index].desc_size;
    }
    return kNumOps;
}

extern "C" int slh_run_program(const void* program, int64_t nbytes, slh_stream_t stream) {
    static const OpIndex index;
    const unsigned char* p = (const unsigned char*)program;
    const unsigned char* end = p + nbytes;
    int idx = 0;
    while (p < end) {
        if (end - p < 8) { slh_set_error("slh_run_program: truncated record header at op %d", idx); return -3; }
        int32_t hdr[2];
        memcpy(hdr, p, 8);
        p += 8;
        const int32_t op = hdr[0], sz = hdr[1];
        if (sz < 0 || end - p < sz) { slh_set_error("slh_run_program: truncated record at op %d", idx); return -3; }
        const OpRow* row = op > 0 && op < kOpSlots ? index.at[op] : nullptr;
        if (!row) { slh_set_error("slh_run_program: unknown opcode %d at op %d", op, idx); return -3; }
        const int rc = row->run(p, sz, stream, row->entry);
        if (rc != 0) return rc;          // stop at the first failing op
        p += (sz + 7) & ~7;
        ++idx;
    }
    return 0;
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
