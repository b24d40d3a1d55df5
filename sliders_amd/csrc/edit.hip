// slh_ddpm_edit_step: one step of the residual DDPM noise space that edits a given image (sliders_amd/edit.py, docs/EDIT.md).
//
//   e   = u + g (t - u)                                        CFG combine of the bf16 epsilon halves, in fp32
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
#include "common.h"
#include "../../include/sliders_hip.h"

namespace {

__global__ __launch_bounds__(256) void ddpm_edit_kernel(const slh_ddpm_edit_desc d) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long n = (long)d.nb * d.chw;
    if (i >= n) return;
    const __bf16* eps = (const __bf16*)d.eps;
    const float u = (float)eps[i];
    const float t = d.eps_text ? (float)((const __bf16*)d.eps_text)[i] : (float)eps[n + i];
    const float x = d.x[i];
    // 8 roundings on the longest path from the inputs to mu (epsilon prediction; 7 with v prediction): docs/EDIT.md counts them
    const float e = u + d.guidance * (t - u);
    float x0, pe;
    if (d.v_prediction) {
        x0 = d.c_sqrt_alpha_t * x - d.c_sqrt_beta_t * e;
        pe = d.c_sqrt_alpha_t * e + d.c_sqrt_beta_t * x;
    } else {
        x0 = (x - d.c_sqrt_beta_t * e) * d.c_inv_sqrt_alpha_t;
        pe = e;
    }
    const float mu = d.c_sqrt_alpha_prev * x0 + d.c_dir * pe;
    float r;
    if (d.mode == 0) {
        r = d.target[i] - mu;
        d.resid[i] = r;
    } else {
        r = d.resid[i];
    }
    const float o = mu + r;
    d.out[i] = o;
    const __bf16 ob = (__bf16)o;       // round to nearest even
    if (d.out_bf16) ((__bf16*)d.out_bf16)[i] = ob;
    if (d.out2_bf16) ((__bf16*)d.out2_bf16)[i] = ob;
}

}  // namespace

extern "C" int slh_ddpm_edit_step(const slh_ddpm_edit_desc* d, slh_stream_t stream) {
    SLH_CHECK(d && d->eps && d->x && d->out, "slh_ddpm_edit_step: null eps / x / out");
    SLH_CHECK(d->mode == 0 || d->mode == 1, "slh_ddpm_edit_step: mode %d (0 invert, 1 edit)", d->mode);
    SLH_CHECK(d->resid, "slh_ddpm_edit_step: mode %d needs resid", d->mode);
    SLH_CHECK(d->mode == 1 || d->target, "slh_ddpm_edit_step: mode 0 (invert) needs target");
    SLH_CHECK(d->nb > 0 && d->chw > 0, "slh_ddpm_edit_step: nb = %d, chw = %d", d->nb, d->chw);
    const long n = (long)d->nb * d->chw;
    hipLaunchKernelGGL(ddpm_edit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *d);
    SLH_LAUNCH_CHECK("slh_ddpm_edit_step");
    return 0;
}
