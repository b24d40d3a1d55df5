// slh_latent_blend: the blend behind every step of a LOCALISED sampling run (sliders_amd/sampler.py, docs/SAMPLING.md).  The step
// itself (slh_cfg_ddim, slh_sigma_step) has produced the latent e; `keep` is the latent the scale-0 chain of the same seed had after
// the same step (SampleTrace.visited), and the mask has one value per latent pixel, shared by the channels:
//
//   m   = mask[b * hw + i % hw]
//   out = m == 0 ? keep : m == 1 ? e : keep + m (e - keep)           blend_one (step_common.h), as slh_ddpm_edit_blend (csrc/edit.hip)
//   dtype 1 (fp32 master latent):  in_bf16 = in2_bf16 = rne(out * s_next)      as slh_sigma_step writes the next pass's input
//   dtype 0 (bf16 latent):         out = rne(the fp32 result);  in_bf16 = in2_bf16 = out's bits
//
// fp32 throughout (bf16 inputs widen exactly), one rounding per operation and nothing contracted, as csrc/sigma_step.hip: the
// restatement edit.blend_reference then describes the kernel.  The selects are on values: a NaN in e never reaches a pixel with
// m = 0, nor one in keep a pixel with m = 1.  Where m = 0 the chain stays on the base chain's bits at every step, so the image is
// the scale-0 image there bit for bit.
// Every thread reads all it needs of its elements before it writes any of them, and no thread touches another's, so out may alias
// e.  16-byte accesses (four fp32 / eight bf16 elements per thread) where every pointer, chw and hw allow them: hw a multiple of
// the vector means a vector never straddles a channel, so its mask values are consecutive and are read as vectors too.  Otherwise
// one element per thread (load_vec / store_vec, step_common.h).  Plain loads and stores; no atomics, nothing waits on another workgroup.
#include <cmath>
#include "step_common.h"
#include "../../include/sliders_hip.h"

namespace {

using namespace slh_step_detail;

struct latent_blend_args {
    const void* e; const void* keep; const float* mask;
    void* out; __bf16* in_bf16; __bf16* in2_bf16;
    long n;                                        // nb * chw
    int chw, hw;
    float s_next;
};

// T: the type of e / keep / out (float: dtype 1, __bf16: dtype 0).  VEC: 16 / sizeof(T) elements per thread, n is a multiple of it
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void latent_blend_kernel(const latent_blend_args d) {
#pragma clang fp contract(off)
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int V = VEC ? (F32 ? 4 : 8) : 1;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n / V) return;
    const long g = i * V;                           // the thread's first element
    const long b = g / d.chw;
    const int pix = (int)(g - b * d.chw) % d.hw;    // chw is a multiple of hw
    float e[V], k[V], m[V], o[V];
    load_vec<V>((const T*)d.e, g, e);
    load_vec<V>((const T*)d.keep, g, k);
    load_vec<V>(d.mask, b * d.hw + pix, m);
#pragma unroll
    for (int c = 0; c < V; ++c) o[c] = blend_one(e[c], k[c], m[c]);
    // everything is read; now the stores
    store_vec<V>((T*)d.out, g, o);
    if constexpr (F32) {
#pragma unroll
        for (int c = 0; c < V; ++c) o[c] = o[c] * d.s_next;
    }
    store_bf16_copies<V>(d.in_bf16, d.in2_bf16, g, o);      // bf16 latents: out's bits again
}

}  // namespace

extern "C" int slh_latent_blend(const void* const* ptrs, const int32_t* dims, const float* coef, slh_stream_t stream) {
    SLH_CHECK(ptrs && dims, "slh_latent_blend: null ptrs / dims");
    const int nb = dims[0], chw = dims[1], hw = dims[2], dtype = dims[3];
    SLH_CHECK(dtype == 0 || dtype == 1, "slh_latent_blend: dtype %d (0 bf16, 1 fp32)", dtype);
    if (const int rc = shape_check("slh_latent_blend", nb, chw, hw)) return rc;
    SLH_CHECK(ptrs[0] && ptrs[1] && ptrs[2] && ptrs[3], "slh_latent_blend: null e / keep / mask / out");
    SLH_CHECK(dtype == 0 || coef, "slh_latent_blend: dtype 1 needs coef (s_next)");
    SLH_CHECK(dtype == 0 || std::isfinite(coef[0]), "slh_latent_blend: s_next = %f is not finite", (double)coef[0]);
    const long n = (long)nb * chw;
    const long esz = dtype == 1 ? 4 : 2;
    latent_blend_args d;
    d.e = ptrs[0]; d.keep = ptrs[1]; d.mask = (const float*)ptrs[2]; d.out = const_cast<void*>(ptrs[3]);
    d.in_bf16 = (__bf16*)ptrs[4]; d.in2_bf16 = (__bf16*)ptrs[5];
    d.n = n; d.chw = chw; d.hw = hw;
    d.s_next = dtype == 1 ? coef[0] : 1.0f;
    const int V = dtype == 1 ? 4 : 8;
    bool vec = chw % V == 0 && hw % V == 0;
    for (const void* p : {d.e, d.keep, (const void*)d.out}) {
        SLH_CHECK(aligned(p, esz), "slh_latent_blend: an e / keep / out pointer (%p) is not %ld-byte aligned", p, esz);
        vec = vec && aligned(p, 16);
    }
    SLH_CHECK(aligned(d.mask, 4), "slh_latent_blend: the mask pointer (%p) is not 4-byte aligned", (const void*)d.mask);
    vec = vec && aligned(d.mask, 16);
    for (const void* p : {(const void*)d.in_bf16, (const void*)d.in2_bf16}) {
        SLH_CHECK(aligned(p, 2), "slh_latent_blend: a bf16 pointer (%p) is not 2-byte aligned", p);
        vec = vec && aligned(p, V * 2);
    }
    // keep is the base chain's and the mask the caller's: the next step, and the next scale, read them again
    const struct { const void* p; long bytes; const char* name; } outs[] = {{d.out, n * esz, "out"}, {d.in_bf16, n * 2, "in_bf16"}, {d.in2_bf16, n * 2, "in2_bf16"}};
    for (const auto& o : outs) {
        SLH_CHECK(!overlaps(d.keep, n * esz, o.p, o.bytes), "slh_latent_blend: keep overlaps %s", o.name);
        SLH_CHECK(!overlaps(d.mask, (long)nb * hw * 4, o.p, o.bytes), "slh_latent_blend: mask overlaps %s", o.name);
    }
    dim3 grid;
    if (const int rc = launch_grid("slh_latent_blend", vec ? n / V : n, n, grid)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    if (dtype == 1) {
        if (vec) hipLaunchKernelGGL((latent_blend_kernel<float, true>), grid, dim3(256), 0, s, d);
        else hipLaunchKernelGGL((latent_blend_kernel<float, false>), grid, dim3(256), 0, s, d);
    } else {
        if (vec) hipLaunchKernelGGL((latent_blend_kernel<__bf16, true>), grid, dim3(256), 0, s, d);
        else hipLaunchKernelGGL((latent_blend_kernel<__bf16, false>), grid, dim3(256), 0, s, d);
    }
    SLH_LAUNCH_CHECK("slh_latent_blend");
    return 0;
}
