// slh_sigma_step: the step between two UNet replays of every sigma-space sampler (euler, euler_a, lms, dpmpp_2m) and of ddpm, on an
// fp32 master latent (sliders_amd/sampler.py, docs/SAMPLING.md).  One launch, element-wise over nb x chw:
//
//   m   = u + g (t - u)                     CFG combine of the bf16 epsilon halves, in fp32 (single branch: m = u, g is not read)
//   x0  = p x + q m                         the predicted clean sample; p, q carry epsilon / v prediction (schedulers.step_row)
//   H0  = kind == 0 ? (x - x0) / sigma      the derivative (euler, euler_a, lms)
//                   : x0                    the denoised sample (ddpm, dpmpp_2m)
//   acc = a x;  acc += c[0] H0;  acc += c[k] H[k], k = 1 .. n_hist ascending;  acc += c_n noise (where there is noise)
//   out = acc;  hist_out = H0;  in_bf16 = in2_bf16 = rne(out * s_next)
//
// fp32 throughout, one rounding per operation and nothing contracted, as csrc/edit.hip: the plain-torch restatement in
// tests/test_sigma_step_host.py (same operations, same order) then describes the kernel, and the bound derived there holds for it.
// Every thread reads all it needs of its elements before it writes any of them, and no thread touches another's, so out may alias x
// and hist_out may alias a history slot (the ring's oldest, which this step reads last and the next step no longer needs).
// Four elements per thread where every buffer allows 16-byte fp32 / 8-byte bf16 accesses, the n % 4 elements left over (and the whole
// range otherwise) one element per thread.  Plain loads and vector stores only; no atomics, nothing waits on another workgroup.
#include "common.h"
#include "../../include/sliders_hip.h"

namespace {

struct sigma_step_args {
    const __bf16* eps_u; const __bf16* eps_t;      // eps_t = NULL: single branch
    const float* x; const float* h[3]; const float* noise;
    float* out; float* hist_out; __bf16* in_bf16; __bf16* in2_bf16;
    long n;                                        // nb * chw
    int n_hist, kind;
    float p, q, sigma, a, c[4], c_n, s_next, g;
};

// one element: (u, t, x, the history values, the noise value) -> out; H0 through h0
__device__ __forceinline__ float sigma_step_one(const sigma_step_args& d, float u, float t, float x, const float* h, float nz, float& h0) {
#pragma clang fp contract(off)
    const float m = d.eps_t ? u + d.g * (t - u) : u;
    const float x0 = d.p * x + d.q * m;
    h0 = d.kind == 0 ? (x - x0) / d.sigma : x0;
    float acc = d.a * x;
    acc = acc + d.c[0] * h0;
    for (int k = 0; k < 3; ++k)
        if (k < d.n_hist) acc = acc + d.c[k + 1] * h[k];
    if (d.noise) acc = acc + d.c_n * nz;
    return acc;
}

template <bool VEC>
__global__ __launch_bounds__(256) void sigma_step_kernel(const sigma_step_args d) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nv = VEC ? d.n / 4 : 0;             // threads [0, nv) take four elements each, [nv, nv + n - 4 nv) one each
    if (VEC && i < nv) {
        const bf16x4 u = ((const bf16x4*)d.eps_u)[i];
        const bf16x4 t = d.eps_t ? ((const bf16x4*)d.eps_t)[i] : u;
        const f32x4 x = ((const f32x4*)d.x)[i];
        f32x4 h[3] = {}, nz = {};
        for (int k = 0; k < 3; ++k)
            if (k < d.n_hist) h[k] = ((const f32x4*)d.h[k])[i];
        if (d.noise) nz = ((const f32x4*)d.noise)[i];
        f32x4 o, h0;
        bf16x4 ob;
        for (int e = 0; e < 4; ++e) {
            const float he[3] = {h[0][e], h[1][e], h[2][e]};
            float h0e;
            o[e] = sigma_step_one(d, (float)u[e], (float)t[e], x[e], he, nz[e], h0e);
            h0[e] = h0e;
            ob[e] = (__bf16)(o[e] * d.s_next);      // round to nearest even
        }
        ((f32x4*)d.out)[i] = o;
        if (d.hist_out) ((f32x4*)d.hist_out)[i] = h0;
        if (d.in_bf16) ((bf16x4*)d.in_bf16)[i] = ob;
        if (d.in2_bf16) ((bf16x4*)d.in2_bf16)[i] = ob;
        return;
    }
    const long j = 4 * nv + (i - nv);
    if (j >= d.n) return;
    const float u = (float)d.eps_u[j];
    const float t = d.eps_t ? (float)d.eps_t[j] : u;
    const float x = d.x[j];
    float h[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3; ++k)
        if (k < d.n_hist) h[k] = d.h[k][j];
    const float nz = d.noise ? d.noise[j] : 0.f;
    float h0;
    const float o = sigma_step_one(d, u, t, x, h, nz, h0);
    const __bf16 ob = (__bf16)(o * d.s_next);       // round to nearest even
    d.out[j] = o;
    if (d.hist_out) d.hist_out[j] = h0;
    if (d.in_bf16) d.in_bf16[j] = ob;
    if (d.in2_bf16) d.in2_bf16[j] = ob;
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int slh_sigma_step(const void* const* ptrs, const int32_t* dims, const float* coef, slh_stream_t stream) {
    SLH_CHECK(ptrs && dims && coef, "slh_sigma_step: null ptrs / dims / coef");
    const int nb = dims[0], chw = dims[1], n_hist = dims[2], kind = dims[3], single = dims[4];
    SLH_CHECK(nb >= 1 && chw >= 1, "slh_sigma_step: nb = %d, chw = %d", nb, chw);
    SLH_CHECK(n_hist >= 0 && n_hist <= 3, "slh_sigma_step: n_hist = %d (0..3)", n_hist);
    SLH_CHECK(kind == 0 || kind == 1, "slh_sigma_step: kind %d (0 derivative, 1 denoised)", kind);
    SLH_CHECK(single == 0 || single == 1, "slh_sigma_step: single = %d (0 the CFG pair, 1 the single branch)", single);
    SLH_CHECK(ptrs[0] && ptrs[2] && ptrs[7], "slh_sigma_step: null eps / x / out");
    for (int k = 0; k < n_hist; ++k) SLH_CHECK(ptrs[3 + k], "slh_sigma_step: n_hist = %d but H[%d] is null", n_hist, k + 1);
    SLH_CHECK(!(single && ptrs[1]), "slh_sigma_step: the single branch has no eps_text");
    SLH_CHECK(kind == 1 || coef[2] != 0.0f, "slh_sigma_step: sigma = 0 with kind 0 (the derivative divides by it)");
    const long n = (long)nb * chw;
    sigma_step_args d;
    d.eps_u = (const __bf16*)ptrs[0];
    d.eps_t = single ? nullptr : ptrs[1] ? (const __bf16*)ptrs[1] : d.eps_u + n;
    d.x = (const float*)ptrs[2];
    for (int k = 0; k < 3; ++k) d.h[k] = k < n_hist ? (const float*)ptrs[3 + k] : nullptr;
    d.noise = (const float*)ptrs[6];
    d.out = (float*)ptrs[7];
    d.hist_out = (float*)ptrs[8];
    d.in_bf16 = (__bf16*)ptrs[9];
    d.in2_bf16 = (__bf16*)ptrs[10];
    d.n = n; d.n_hist = n_hist; d.kind = kind;
    d.p = coef[0]; d.q = coef[1]; d.sigma = coef[2]; d.a = coef[3];
    for (int k = 0; k < 4; ++k) d.c[k] = coef[4 + k];
    d.c_n = coef[8]; d.s_next = coef[9]; d.g = coef[10];
    const void* const f32s[] = {d.x, d.h[0], d.h[1], d.h[2], d.noise, d.out, d.hist_out};
    const void* const bf16s[] = {d.eps_u, d.eps_t, d.in_bf16, d.in2_bf16};
    bool vec = true;
    for (const void* p : f32s) {
        SLH_CHECK(aligned(p, 4), "slh_sigma_step: an fp32 pointer (%p) is not 4-byte aligned", p);
        vec = vec && aligned(p, 16);
    }
    for (const void* p : bf16s) {
        SLH_CHECK(aligned(p, 2), "slh_sigma_step: a bf16 pointer (%p) is not 2-byte aligned", p);
        vec = vec && aligned(p, 8);
    }
    const long threads = vec ? n / 4 + n % 4 : n;
    SLH_CHECK((threads + 255) / 256 < (1L << 31), "slh_sigma_step: nb * chw = %ld is too large for one launch", n);
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (vec) hipLaunchKernelGGL(sigma_step_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, d);
    else hipLaunchKernelGGL(sigma_step_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, d);
    SLH_LAUNCH_CHECK("slh_sigma_step");
    return 0;
}
