// slh_sigma_step: the step between two UNet replays of every sigma-space sampler (euler, euler_a, lms, dpmpp_2m) and of ddpm, on an
// fp32 master latent (sliders_amd/sampler.py, docs/SAMPLING.md).  One launch, element-wise over nb x chw:
//
//   m   = u + g (t - u)                     CFG combine of the bf16 epsilon halves, in fp32 (cfg_combine, step_common.h; single
//                                           branch: m = u, g is not read)
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
// range otherwise) one element per thread (load_vec / store_vec, step_common.h).  Plain loads and vector stores only; no atomics,
// nothing waits on another workgroup.
#include "step_common.h"
#include "../../include/sliders_hip.h"

namespace {

using namespace slh_step_detail;

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
    const float m = d.eps_t ? cfg_combine(u, t, d.g) : u;
    const float x0 = d.p * x + d.q * m;
    h0 = d.kind == 0 ? (x - x0) / d.sigma : x0;
    float acc = d.a * x;
    acc = acc + d.c[0] * h0;
    for (int k = 0; k < 3; ++k)
        if (k < d.n_hist) acc = acc + d.c[k + 1] * h[k];
    if (d.noise) acc = acc + d.c_n * nz;
    return acc;
}

// the V elements from g on: every load, then the arithmetic, then every store
template <int V>
__device__ __forceinline__ void sigma_step_elems(const sigma_step_args& d, const long g) {
#pragma clang fp contract(off)
    float u[V], t[V], x[V], h[3][V] = {}, nz[V] = {}, o[V], h0[V], ob[V];
    load_vec<V>(d.eps_u, g, u);
    if (d.eps_t) load_vec<V>(d.eps_t, g, t);
    load_vec<V>(d.x, g, x);
    for (int k = 0; k < 3; ++k)
        if (k < d.n_hist) load_vec<V>(d.h[k], g, h[k]);
    if (d.noise) load_vec<V>(d.noise, g, nz);
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const float he[3] = {h[0][e], h[1][e], h[2][e]};
        o[e] = sigma_step_one(d, u[e], d.eps_t ? t[e] : u[e], x[e], he, nz[e], h0[e]);
        ob[e] = o[e] * d.s_next;
    }
    store_vec<V>(d.out, g, o);
    if (d.hist_out) store_vec<V>(d.hist_out, g, h0);
    store_bf16_copies<V>(d.in_bf16, d.in2_bf16, g, ob);
}

template <bool VEC>
__global__ __launch_bounds__(256) void sigma_step_kernel(const sigma_step_args d) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nv = VEC ? d.n / 4 : 0;             // threads [0, nv) take four elements each, [nv, nv + n - 4 nv) one each
    if (VEC && i < nv) return sigma_step_elems<4>(d, 4 * i);
    const long j = 4 * nv + (i - nv);
    if (j < d.n) sigma_step_elems<1>(d, j);
}

}  // namespace

extern "C" int slh_sigma_step(const void* const* ptrs, const int32_t* dims, const float* coef, slh_stream_t stream) {
    SLH_CHECK(ptrs && dims && coef, "slh_sigma_step: null ptrs / dims / coef");
    const int nb = dims[0], chw = dims[1], n_hist = dims[2], kind = dims[3], single = dims[4];
    if (const int rc = shape_check("slh_sigma_step", nb, chw)) return rc;
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
    d.eps_t = single ? nullptr : text_half(ptrs[0], ptrs[1], n);
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
    dim3 grid;
    if (const int rc = launch_grid("slh_sigma_step", vec ? n / 4 + n % 4 : n, n, grid)) return rc;
    if (vec) hipLaunchKernelGGL(sigma_step_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, d);
    else hipLaunchKernelGGL(sigma_step_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, d);
    SLH_LAUNCH_CHECK("slh_sigma_step");
    return 0;
}
