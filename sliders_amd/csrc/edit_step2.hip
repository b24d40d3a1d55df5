// slh_edit_step2: one step of the SECOND-ORDER residual noise space that edits a given image (sliders_amd/edit.py, docs/EDIT.md,
// "Second-order noise space"): slh_ddpm_edit_step's mean mu_1 with the multistep correction of SDE-DPM-Solver++ 2M added, the mode
// branch of slh_ddpm_edit_step, and - with keep and mask - the blend of slh_ddpm_edit_blend, in one launch.  Per element:
//
//   e    = u + g (t - u)                                       CFG combine (cfg_combine, step_common.h)
//   x0h, mu_1                                                  ddpm_mu_x0 (step_common.h): the code slh_ddpm_edit_step forms them with
//   with x0_prev:  d = x0h - x0_prev;  p = c_corr d;  mu = mu_1 + p          without: mu = mu_1, nothing is read or multiplied
//   mode 0 (invert):  resid = target - mu   written            mode 1 (edit):  resid   read
//   o    = mu + resid                                          never `target`: the edit can only recompute mu + d
//   with keep, mask:  o = m == 0 ? keep : m == 1 ? o : keep + m (o - keep)   blend_one (step_common.h)
//   out = o;  x0_out = x0h;  out_bf16 = out2_bf16 = rne(o)
//
// fp32 throughout, one rounding per operation and nothing contracted, as csrc/edit.hip: the restatement edit.ddpm_mu2_reference (one
// tensor operation per operation here, in this order) then describes the kernel.  mu is one piece of code ahead of the mode branch, so
// an edit over the same epsilon, the same history and the inversion's residuals walks the inversion's latents again bit for bit; and
// without x0_prev the launch writes what slh_ddpm_edit_step / slh_ddpm_edit_blend write, bit for bit.
// Every thread reads all it needs of its elements before it writes any of them, and no thread touches another's, so out may alias x
// and x0_out may alias x0_prev.  Four elements per thread (16-byte fp32, 8-byte bf16 accesses) where every pointer, chw and hw allow
// them - hw a multiple of four means a vector never straddles a channel, so its mask values are consecutive - otherwise one element
// per thread (load_vec / store_vec, step_common.h).  Plain loads and vector stores only; no LDS, no atomics, nothing waits on another
// workgroup.
#include <cmath>
#include "step_common.h"
#include "../../include/sliders_hip.h"

namespace {

using namespace slh_step_detail;

struct edit_step2_args {
    const __bf16* eps_u; const __bf16* eps_t;
    const float* x; const float* x0_prev; const float* target; float* resid; const float* keep; const float* mask;
    float* out; float* x0_out; __bf16* out_bf16; __bf16* out2_bf16;
    long n;                                        // nb * chw
    int chw, hw, mode;
    mu_coef c;
    float c_corr;
};

// the V elements from g on: every load, then the arithmetic, then every store
template <int V>
__device__ __forceinline__ void edit_step2_elems(const edit_step2_args& d, const long g) {
#pragma clang fp contract(off)
    float u[V], t[V], x[V], h[V] = {}, r[V], k[V] = {}, m[V] = {}, o[V], x0[V];
    load_vec<V>(d.eps_u, g, u);
    load_vec<V>(d.eps_t, g, t);
    load_vec<V>(d.x, g, x);
    if (d.x0_prev) load_vec<V>(d.x0_prev, g, h);
    load_vec<V>(d.mode == 0 ? d.target : (const float*)d.resid, g, r);          // mode 0: the target, mode 1: the residual
    if (d.mask) {
        const long b = g / d.chw;
        const int pix = (int)(g - b * d.chw) % d.hw;                            // chw is a multiple of hw
        load_vec<V>(d.keep, g, k);
        load_vec<V>(d.mask, b * d.hw + pix, m);
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
        float mu = ddpm_mu_x0(d.c, u[e], t[e], x[e], x0[e]);
        if (d.x0_prev) {                            // three more roundings; skipped, not multiplied by zero, without a history
            const float dd = x0[e] - h[e];
            const float p = d.c_corr * dd;
            mu = mu + p;
        }
        if (d.mode == 0) r[e] = r[e] - mu;          // resid = target - mu
        o[e] = mu + r[e];
        if (d.mask) o[e] = blend_one(o[e], k[e], m[e]);
    }
    if (d.mode == 0) store_vec<V>(d.resid, g, r);
    store_vec<V>(d.out, g, o);
    if (d.x0_out) store_vec<V>(d.x0_out, g, x0);
    store_bf16_copies<V>(d.out_bf16, d.out2_bf16, g, o);
}

// V = 4: n is a multiple of four (chw is)
template <int V>
__global__ __launch_bounds__(256) void edit_step2_kernel(const edit_step2_args d) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < d.n / V) edit_step2_elems<V>(d, i * V);
}

}  // namespace

extern "C" int slh_edit_step2(const void* const* ptrs, const int32_t* dims, const float* coef, slh_stream_t stream) {
    static const char* const name = "slh_edit_step2";
    SLH_CHECK(ptrs && dims && coef, "%s: null ptrs / dims / coef", name);
    const int nb = dims[0], chw = dims[1], hw = dims[2], mode = dims[3], v_prediction = dims[4];
    if (const int rc = shape_check(name, nb, chw, hw)) return rc;
    SLH_CHECK(mode == 0 || mode == 1, "%s: mode %d (0 invert, 1 edit)", name, mode);
    SLH_CHECK(v_prediction == 0 || v_prediction == 1, "%s: v_prediction = %d (0, 1)", name, v_prediction);
    SLH_CHECK(ptrs[0] && ptrs[2] && ptrs[5] && ptrs[8], "%s: null eps / x / resid / out", name);
    SLH_CHECK(mode == 1 || ptrs[4], "%s: mode 0 (invert) needs target", name);
    SLH_CHECK(!ptrs[6] == !ptrs[7], "%s: keep and mask go together (keep %p, mask %p)", name, ptrs[6], ptrs[7]);
    SLH_CHECK(mode == 1 || !ptrs[7], "%s: mode 0 (invert) takes no mask", name);
    SLH_CHECK(!ptrs[3] || (std::isfinite(coef[6]) && coef[6] != 0.0f), "%s: x0_prev with c_corr = %f (finite and not zero; order 1: no x0_prev)",
              name, (double)coef[6]);
    const long n = (long)nb * chw;
    edit_step2_args d;
    d.eps_u = (const __bf16*)ptrs[0];
    d.eps_t = text_half(ptrs[0], ptrs[1], n);
    d.x = (const float*)ptrs[2];
    d.x0_prev = (const float*)ptrs[3];
    d.target = mode == 0 ? (const float*)ptrs[4] : nullptr;          // mode 1: not read
    d.resid = (float*)ptrs[5];
    d.keep = (const float*)ptrs[6];
    d.mask = (const float*)ptrs[7];
    d.out = (float*)ptrs[8];
    d.x0_out = (float*)ptrs[9];
    d.out_bf16 = (__bf16*)ptrs[10];
    d.out2_bf16 = (__bf16*)ptrs[11];
    d.n = n; d.chw = chw; d.hw = hw; d.mode = mode;
    d.c = mu_coef{coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], v_prediction};
    d.c_corr = coef[6];
    bool vec = chw % 4 == 0 && hw % 4 == 0;
    for (const void* p : {(const void*)d.x, (const void*)d.x0_prev, (const void*)d.target, (const void*)d.resid, (const void*)d.keep,
                          (const void*)d.mask, (const void*)d.out, (const void*)d.x0_out}) {
        SLH_CHECK(aligned(p, 4), "%s: an fp32 pointer (%p) is not 4-byte aligned", name, p);
        vec = vec && aligned(p, 16);
    }
    for (const void* p : {(const void*)d.eps_u, (const void*)d.eps_t, (const void*)d.out_bf16, (const void*)d.out2_bf16}) {
        SLH_CHECK(aligned(p, 2), "%s: a bf16 pointer (%p) is not 2-byte aligned", name, p);
        vec = vec && aligned(p, 8);
    }
    // what the launch reads and what it writes.  The two legal aliases are the SAME address: an output that overlaps its input at an
    // offset would be read by one thread after another has written it
    struct range { const void* p; long bytes; const char* name; };
    const range ins[] = {{d.eps_u, ptrs[1] ? n * 2 : n * 4, "eps"}, {ptrs[1], n * 2, "eps_text"}, {d.x, n * 4, "x"}, {d.x0_prev, n * 4, "x0_prev"},
                         {d.target, n * 4, "target"}, {mode == 1 ? d.resid : nullptr, n * 4, "resid"}, {d.keep, n * 4, "keep"},
                         {d.mask, (long)nb * hw * 4, "mask"}};
    const range outs[] = {{mode == 0 ? d.resid : nullptr, n * 4, "resid"}, {d.out, n * 4, "out"}, {d.x0_out, n * 4, "x0_out"},
                          {d.out_bf16, n * 2, "out_bf16"}, {d.out2_bf16, n * 2, "out2_bf16"}};
    for (int a = 0; a < 5; ++a) {
        const range& o = outs[a];
        if (!o.p) continue;
        for (int b = 0; b < 8; ++b) {
            const range& i = ins[b];
            const bool alias = o.p == i.p && ((a == 1 && b == 2) || (a == 2 && b == 3));          // out == x, x0_out == x0_prev
            SLH_CHECK(alias || !i.p || !overlaps(i.p, i.bytes, o.p, o.bytes), "%s: %s overlaps %s", name, o.name, i.name);
        }
        for (int b = a + 1; b < 5; ++b)
            SLH_CHECK(!overlaps(o.p, o.bytes, outs[b].p, outs[b].bytes), "%s: %s overlaps %s", name, o.name, outs[b].name);
    }
    dim3 grid;
    if (const int rc = launch_grid(name, vec ? n / 4 : n, n, grid)) return rc;
    if (vec) hipLaunchKernelGGL(edit_step2_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, d);
    else hipLaunchKernelGGL(edit_step2_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, d);
    SLH_LAUNCH_CHECK(name);
    return 0;
}
