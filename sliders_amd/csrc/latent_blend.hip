// slh_latent_blend: the blend behind every step of a LOCALISED sampling run (sliders_amd/sampler.py, docs/SAMPLING.md).  The step
// itself (slh_cfg_ddim, slh_sigma_step) has produced the latent e; `keep` is the latent the scale-0 chain of the same seed had after
// the same step (SampleTrace.visited), and the mask has one value per latent pixel, shared by the channels:
//
//   m   = mask[b * hw + i % hw]
//   out = m == 0 ? keep : m == 1 ? e : keep + m (e - keep)           the select-then-lerp of slh_ddpm_edit_blend (csrc/edit.hip)
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
// one element per thread.  Plain loads and stores; no atomics, nothing waits on another workgroup.
#include <cmath>
#include "common.h"
#include "../../include/sliders_hip.h"

namespace {

struct latent_blend_args {
    const void* e; const void* keep; const float* mask;
    void* out; __bf16* in_bf16; __bf16* in2_bf16;
    long n;                                        // nb * chw
    int chw, hw;
    float s_next;
};

__device__ __forceinline__ float blend_one(float e, float k, float m) {
#pragma clang fp contract(off)
    // three roundings where 0 < m < 1: e - k, m *, k +
    const float o = k + m * (e - k);
    return m == 0.0f ? k : m == 1.0f ? e : o;
}

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
    const float* mp = d.mask + b * d.hw + pix;
    float e[V], k[V], m[V], o[V];
    if constexpr (!VEC) {
        e[0] = (float)((const T*)d.e)[g];
        k[0] = (float)((const T*)d.keep)[g];
        m[0] = mp[0];
    } else if constexpr (F32) {
        const f32x4 ev = ((const f32x4*)d.e)[i], kv = ((const f32x4*)d.keep)[i], mv = *(const f32x4*)mp;
        for (int c = 0; c < 4; ++c) { e[c] = ev[c]; k[c] = kv[c]; m[c] = mv[c]; }
    } else {
        const bf16x8 ev = ((const bf16x8*)d.e)[i], kv = ((const bf16x8*)d.keep)[i];
        const f32x4 m0 = ((const f32x4*)mp)[0], m1 = ((const f32x4*)mp)[1];
        for (int c = 0; c < 8; ++c) { e[c] = (float)ev[c]; k[c] = (float)kv[c]; m[c] = c < 4 ? m0[c] : m1[c - 4]; }
    }
#pragma unroll
    for (int c = 0; c < V; ++c) o[c] = blend_one(e[c], k[c], m[c]);
    // everything is read; now the stores
    if constexpr (!VEC) {
        __bf16 ob;
        if constexpr (F32) {
            ((float*)d.out)[g] = o[0];
            ob = (__bf16)(o[0] * d.s_next);         // round to nearest even
        } else {
            ob = (__bf16)o[0];
            ((__bf16*)d.out)[g] = ob;
        }
        if (d.in_bf16) d.in_bf16[g] = ob;
        if (d.in2_bf16) d.in2_bf16[g] = ob;
    } else if constexpr (F32) {
        f32x4 ov;
        bf16x4 ob;
        for (int c = 0; c < 4; ++c) { ov[c] = o[c]; ob[c] = (__bf16)(o[c] * d.s_next); }
        ((f32x4*)d.out)[i] = ov;
        if (d.in_bf16) ((bf16x4*)d.in_bf16)[i] = ob;
        if (d.in2_bf16) ((bf16x4*)d.in2_bf16)[i] = ob;
    } else {
        bf16x8 ob;
        for (int c = 0; c < 8; ++c) ob[c] = (__bf16)o[c];
        ((bf16x8*)d.out)[i] = ob;
        if (d.in_bf16) ((bf16x8*)d.in_bf16)[i] = ob;
        if (d.in2_bf16) ((bf16x8*)d.in2_bf16)[i] = ob;
    }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// [a, a + na) and [b, b + nb) bytes share an address (a null b: no)
inline bool overlaps(const void* a, long na, const void* b, long nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return b && x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

}  // namespace

extern "C" int slh_latent_blend(const void* const* ptrs, const int32_t* dims, const float* coef, slh_stream_t stream) {
    SLH_CHECK(ptrs && dims, "slh_latent_blend: null ptrs / dims");
    const int nb = dims[0], chw = dims[1], hw = dims[2], dtype = dims[3];
    SLH_CHECK(dtype == 0 || dtype == 1, "slh_latent_blend: dtype %d (0 bf16, 1 fp32)", dtype);
    SLH_CHECK(nb >= 1 && chw >= 1 && hw >= 1, "slh_latent_blend: nb = %d, chw = %d, hw = %d", nb, chw, hw);
    SLH_CHECK(chw % hw == 0, "slh_latent_blend: chw = %d is not a multiple of hw = %d", chw, hw);
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
    const long threads = vec ? n / V : n;
    SLH_CHECK((threads + 255) / 256 < (1L << 31), "slh_latent_blend: nb * chw = %ld is too large for one launch", n);
    const dim3 grid((unsigned)((threads + 255) / 256));
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
