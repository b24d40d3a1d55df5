// The pieces the element-wise step kernels share (edit.hip, edit_step2.hip, sigma_step.hip, latent_blend.hip, eps_direction.hip): the
// CFG combine, the DDIM mean of the edit steps, the select-then-lerp blend, the text half of an epsilon pair, vector-or-scalar operand access and the bf16 copies of a result; on the
// host the alignment, overlap and shape checks (the launch sizing is common.h's launch_grid).  Each is stated here once.  These kernels are held bit for bit
// to plain-torch restatements in the same operation order (tests/*_ref.py, edit.ddpm_mu_reference, edit.blend_reference): fp32, one
// rounding per operation, nothing contracted.
// EVERY DEVICE FUNCTION HERE THAT DOES ARITHMETIC CARRIES ITS OWN `#pragma clang fp contract(off)`.  The setting belongs to the
// instructions of the function they are written in, not to the kernel they are inlined into: without the pragma the compiler may fuse
// a helper's multiply and add into one fma (one rounding instead of two) whatever the calling kernel says.  Do not lose it.  (The
// access helpers and text_half only convert and move: there is nothing in them to contract.)
// gfx950 only.
#pragma once
#include "common.h"

namespace slh_step_detail {

// ---- device side ----------------------------------------------------------------------------------------------------------------
// CFG combine of the epsilon halves u (unconditional) and t (text): three roundings, t - u, g *, u +
__device__ __forceinline__ float cfg_combine(float u, float t, float g) {
#pragma clang fp contract(off)      // the product and the sum must stay two instructions
    return u + g * (t - u);
}

// out = k where m == 0, e where m == 1 (both exactly), k + m (e - k) between: three roundings there, e - k, m *, k +.  The selects
// are on the value of m and come after the lerp: a NaN on the side that is not selected never reaches the result.
__device__ __forceinline__ float blend_one(float e, float k, float m) {
#pragma clang fp contract(off)      // the product and the sum must stay two instructions
    const float o = k + m * (e - k);
    return m == 0.0f ? k : m == 1.0f ? e : o;
}

// the coefficients of the DDIM mean, as the edit step kernels read them from their descriptors or their coef array
struct mu_coef {
    float guidance, c_sqrt_beta_t, c_inv_sqrt_alpha_t, c_sqrt_alpha_t, c_sqrt_alpha_prev, c_dir;
    int v_prediction;
};

// CFG combine + the DDIM mean of x_{t-1} from the epsilon halves u, t and the master latent x; the predicted clean sample through x0.
// The one piece of code slh_ddpm_edit_step, slh_ddpm_edit_blend and slh_edit_step2 form them with.
__device__ __forceinline__ float ddpm_mu_x0(const mu_coef& c, float u, float t, float x, float& x0) {
#pragma clang fp contract(off)
    // 8 roundings on the longest path from the inputs to mu (epsilon prediction; 7 with v prediction): docs/EDIT.md counts them
    const float e = cfg_combine(u, t, c.guidance);
    float pe;
    if (c.v_prediction) {
        x0 = c.c_sqrt_alpha_t * x - c.c_sqrt_beta_t * e;
        pe = c.c_sqrt_alpha_t * e + c.c_sqrt_beta_t * x;
    } else {
        x0 = (x - c.c_sqrt_beta_t * e) * c.c_inv_sqrt_alpha_t;
        pe = e;
    }
    return c.c_sqrt_alpha_prev * x0 + c.c_dir * pe;
}
__device__ __forceinline__ float ddpm_mu(const mu_coef& c, float u, float t, float x) {
    float x0;
    return ddpm_mu_x0(c, u, t, x, x0);
}

// The text half of an epsilon pair of n elements each: its own buffer where one is given, else the rows behind the unconditional
// half.  A pointer, chosen once per thread (or once on the host), not once per element.
__host__ __device__ __forceinline__ const __bf16* text_half(const void* eps, const void* eps_text, long n) {
    return eps_text ? (const __bf16*)eps_text : (const __bf16*)eps + n;
}

// V elements of T (bf16 or fp32) go in accesses of W: all of them where they fit 16 bytes (one element, four or eight bf16, four fp32),
// else 16 bytes each (eight fp32 are two accesses).  The caller has made sure the address is aligned to the access.
template <int V, typename T>
struct vec_access {
    static constexpr int W = V * sizeof(T) > 16 ? 16 / sizeof(T) : V;
    typedef T __attribute__((ext_vector_type(W))) type;
};

// v[0..V) = the V elements of p from g on, widened to fp32 (exact)
template <int V, typename T>
__device__ __forceinline__ void load_vec(const T* p, long g, float* v) {
    using A = vec_access<V, T>;
#pragma unroll
    for (int a = 0; a < V / A::W; ++a) {
        const typename A::type x = ((const typename A::type*)(p + g))[a];
#pragma unroll
        for (int e = 0; e < A::W; ++e) v[a * A::W + e] = (float)x[e];
    }
}

// the store to match; a bf16 destination takes the round-to-nearest-even of v
template <int V, typename T>
__device__ __forceinline__ void store_vec(T* p, long g, const float* v) {
    using A = vec_access<V, T>;
#pragma unroll
    for (int a = 0; a < V / A::W; ++a) {
        typename A::type x;
#pragma unroll
        for (int e = 0; e < A::W; ++e) x[e] = (T)v[a * A::W + e];
        ((typename A::type*)(p + g))[a] = x;
    }
}

// the bf16 rounding of an fp32 result (the next UNet pass's input) to up to two destinations, each if it is given; V = 1, 4 or 8
template <int V>
__device__ __forceinline__ void store_bf16_copies(__bf16* a, __bf16* b, long g, const float* v) {
    typename vec_access<V, __bf16>::type r;
#pragma unroll
    for (int e = 0; e < V; ++e) r[e] = (__bf16)v[e];       // round to nearest even, once for both
    if (a) *(decltype(r)*)(a + g) = r;
    if (b) *(decltype(r)*)(b + g) = r;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// [a, a + na) and [b, b + nb) bytes share an address (a null b: no)
inline bool overlaps(const void* a, long na, const void* b, long nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return b && x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

// the shape of a batch of latents: nb samples of chw elements, and where the entry point has pixels, hw of them per channel
inline int shape_check(const char* name, int nb, int chw) {
    SLH_CHECK(nb >= 1 && chw >= 1, "%s: nb = %d, chw = %d", name, nb, chw);
    return 0;
}
inline int shape_check(const char* name, int nb, int chw, int hw) {
    SLH_CHECK(nb >= 1 && chw >= 1 && hw >= 1, "%s: nb = %d, chw = %d, hw = %d", name, nb, chw, hw);
    SLH_CHECK(chw % hw == 0, "%s: chw = %d is not a multiple of hw = %d", name, chw, hw);
    return 0;
}

using ::launch_grid;      // common.h: the grid of a launch over n = nb * chw elements, refused where it does not fit

}  // namespace slh_step_detail
