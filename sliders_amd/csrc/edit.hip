// slh_ddpm_edit_step: one step of the residual DDPM noise space that edits a given image (sliders_amd/edit.py, docs/EDIT.md).
//
//   e   = u + g (t - u)                                        CFG combine of the bf16 epsilon halves, in fp32 (cfg_combine, step_common.h)
//   mu  = c_sqrt_alpha_prev x0(x, e) + c_dir eps(x, e)         the DDIM mean of x_{t-1}, epsilon or v prediction
//   mode 0 (invert):  resid = target - mu                      written
//   mode 1 (edit):    resid                                    read
//   out = mu + resid                                           the fp32 master latent; bf16(out) is the next UNet input
//
// The point of the form is that an edit which reads the residuals an inversion wrote, over the same epsilon, walks the inversion's
// latents again bit for bit: mu is one piece of code ahead of the mode branch, out is mu + resid in both modes (never `target`), and
// nothing here may be contracted - an fma formed in one mode's copy of the code and not in the other's would break the identity, and
// the fp32 restatement in sliders_amd/edit.py (plain tensor ops, one rounding per operation) would no longer describe the kernel.
// One element per thread, as cfg_ddim_kernel: a latent is 4 x 128 x 128 values, the launch is a few microseconds of HBM traffic.
//
// slh_ddpm_edit_blend: the edit step of a LOCALISED edit.  e = mu + resid as mode 1 above (ddpm_mu: the one piece of code both
// kernels form mu with), then blended against `keep`, the latent the inversion's own chain had after this step, under a mask with
// one value per latent pixel:  out = keep where m == 0, e where m == 1 (both exactly), keep + m (e - keep) between (blend_one,
// step_common.h: the one piece of code slh_latent_blend blends with too).  Where the
// mask is 0 the edited latent is the inversion's at every step, so the result is the reconstruction there bit for bit; and an edit
// at scale 0 has e == keep, so keep + m * 0 is keep under any mask.
//
// slh_eps_absdiff: sum over the channels of |e_a - e_b| for two CFG-combined epsilon pairs - where a slider acts, for one noise
// draw (SliderEditor.footprint).  One thread per pixel, the channels in ascending order: no atomics, the same bits every run.
#include "step_common.h"
#include "../../include/sliders_hip.h"

namespace {

using namespace slh_step_detail;

// the coefficients both step kernels read from their descriptors (mu_coef, ddpm_mu: step_common.h, shared with csrc/edit_step2.hip)
template <typename D>
__device__ __forceinline__ mu_coef coef_of(const D& d) {
    return mu_coef{d.guidance, d.c_sqrt_beta_t, d.c_inv_sqrt_alpha_t, d.c_sqrt_alpha_t, d.c_sqrt_alpha_prev, d.c_dir, d.v_prediction};
}

__global__ __launch_bounds__(256) void ddpm_edit_kernel(const slh_ddpm_edit_desc d) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long n = (long)d.nb * d.chw;
    if (i >= n) return;
    const __bf16* eps = (const __bf16*)d.eps;
    const __bf16* text = text_half(d.eps, d.eps_text, n);
    const float mu = ddpm_mu(coef_of(d), (float)eps[i], (float)text[i], d.x[i]);
    float r;
    if (d.mode == 0) {
        r = d.target[i] - mu;
        d.resid[i] = r;
    } else {
        r = d.resid[i];
    }
    const float o = mu + r;
    d.out[i] = o;
    store_bf16_copies<1>((__bf16*)d.out_bf16, (__bf16*)d.out2_bf16, i, &o);
}

__global__ __launch_bounds__(256) void ddpm_edit_blend_kernel(const slh_ddpm_edit_blend_desc d) {
#pragma clang fp contract(off)
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;          // the entry point refuses nb * chw >= 2^31
    const unsigned n = (unsigned)d.nb * (unsigned)d.chw;
    if (i >= n) return;
    const __bf16* eps = (const __bf16*)d.eps;
    const __bf16* text = text_half(d.eps, d.eps_text, n);
    const float mu = ddpm_mu(coef_of(d), (float)eps[i], (float)text[i], d.x[i]);
    const float e = mu + d.resid[i];                                   // ddpm_edit_kernel's mode 1, to the bit
    const float k = d.keep[i];
    const float m = d.mask[i / (unsigned)d.chw * (unsigned)d.hw + i % (unsigned)d.hw];   // chw is a multiple of hw: i % hw is the pixel
    const float o = blend_one(e, k, m);                                // three more roundings where 0 < m < 1
    d.out[i] = o;
    store_bf16_copies<1>((__bf16*)d.out_bf16, (__bf16*)d.out2_bf16, i, &o);
}

__global__ __launch_bounds__(256) void eps_absdiff_kernel(const slh_eps_absdiff_desc d) {
#pragma clang fp contract(off)
    const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;          // b * hw + p; the entry point refuses nb * chw >= 2^31
    if (j >= (unsigned)d.nb * (unsigned)d.hw) return;
    const unsigned n = (unsigned)d.nb * (unsigned)d.chw;
    const __bf16* a = (const __bf16*)d.eps_a;
    const __bf16* b = (const __bf16*)d.eps_b;
    const __bf16* at = text_half(d.eps_a, d.eps_a_text, n);
    const __bf16* bt = text_half(d.eps_b, d.eps_b_text, n);
    unsigned i = j / (unsigned)d.hw * (unsigned)d.chw + j % (unsigned)d.hw;
    float acc = 0.0f;
    for (int c = 0; c < d.chw / d.hw; ++c, i += d.hw) {
        const float ea = cfg_combine((float)a[i], (float)at[i], d.guidance);
        const float eb = cfg_combine((float)b[i], (float)bt[i], d.guidance);
        acc = acc + fabsf(ea - eb);
    }
    d.out[j] = acc;
}

}  // namespace

extern "C" int slh_ddpm_edit_blend(const slh_ddpm_edit_blend_desc* d, slh_stream_t stream) {
    SLH_CHECK(d && d->eps && d->x && d->resid && d->out, "slh_ddpm_edit_blend: null eps / x / resid / out");
    SLH_CHECK(d->keep && d->mask, "slh_ddpm_edit_blend: null keep / mask");
    if (const int rc = shape_check("slh_ddpm_edit_blend", d->nb, d->chw, d->hw)) return rc;
    const long n = (long)d->nb * d->chw;
    SLH_CHECK(n < (1L << 31), "slh_ddpm_edit_blend: nb * chw = %ld: the kernel indexes with 32 bits", n);
    // keep and mask are the inversion's and the caller's: a step that wrote over them (or read them half written, where they overlap
    // out at an offset) would leave the next step, and the next edit, another image to keep.  out may alias x, as slh_ddpm_edit_step's
    SLH_CHECK(!overlaps(d->keep, n * 4, d->out, n * 4), "slh_ddpm_edit_blend: keep aliases out");
    SLH_CHECK(!overlaps(d->mask, (long)d->nb * d->hw * 4, d->out, n * 4), "slh_ddpm_edit_blend: mask aliases out");
    dim3 grid;
    if (const int rc = launch_grid("slh_ddpm_edit_blend", n, n, grid)) return rc;
    hipLaunchKernelGGL(ddpm_edit_blend_kernel, grid, dim3(256), 0, (hipStream_t)stream, *d);
    SLH_LAUNCH_CHECK("slh_ddpm_edit_blend");
    return 0;
}

extern "C" int slh_eps_absdiff(const slh_eps_absdiff_desc* d, slh_stream_t stream) {
    SLH_CHECK(d && d->eps_a && d->eps_b && d->out, "slh_eps_absdiff: null eps_a / eps_b / out");
    if (const int rc = shape_check("slh_eps_absdiff", d->nb, d->chw, d->hw)) return rc;
    const long n = (long)d->nb * d->chw;
    SLH_CHECK(n < (1L << 31), "slh_eps_absdiff: nb * chw = %ld: the kernel indexes with 32 bits", n);
    dim3 grid;
    if (const int rc = launch_grid("slh_eps_absdiff", (long)d->nb * d->hw, n, grid)) return rc;      // one thread per pixel
    hipLaunchKernelGGL(eps_absdiff_kernel, grid, dim3(256), 0, (hipStream_t)stream, *d);
    SLH_LAUNCH_CHECK("slh_eps_absdiff");
    return 0;
}

extern "C" int slh_ddpm_edit_step(const slh_ddpm_edit_desc* d, slh_stream_t stream) {
    SLH_CHECK(d && d->eps && d->x && d->out, "slh_ddpm_edit_step: null eps / x / out");
    SLH_CHECK(d->mode == 0 || d->mode == 1, "slh_ddpm_edit_step: mode %d (0 invert, 1 edit)", d->mode);
    SLH_CHECK(d->resid, "slh_ddpm_edit_step: mode %d needs resid", d->mode);
    SLH_CHECK(d->mode == 1 || d->target, "slh_ddpm_edit_step: mode 0 (invert) needs target");
    if (const int rc = shape_check("slh_ddpm_edit_step", d->nb, d->chw)) return rc;
    const long n = (long)d->nb * d->chw;
    dim3 grid;
    if (const int rc = launch_grid("slh_ddpm_edit_step", n, n, grid)) return rc;
    hipLaunchKernelGGL(ddpm_edit_kernel, grid, dim3(256), 0, (hipStream_t)stream, *d);
    SLH_LAUNCH_CHECK("slh_ddpm_edit_step");
    return 0;
}
