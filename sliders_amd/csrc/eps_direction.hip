// slh_direction_threshold, slh_eps_direction, slh_eps_direction_momentum: prompt-direction sampling (sliders_amd/directions.py, docs/SAMPLING.md, "Prompt-direction
// sampling").  One UNet pass has produced, next to the text row t, the rows e+_k, e-_k of up to three prompt pairs on the same latent;
// the guided text row the step kernels then read through their eps_text input is
//
//   d_k  = e+_k - e-_k                                  one fp32 subtraction of the two widened bf16 values
//   key  = the upper 16 bits of the fp32 bit pattern of |d_k|       (an integer, monotone in |d_k|)
//   keep = key >= tau[b][k][channel]                    tau: the n_keep-th largest key among the hw pixels of that (sample, direction,
//                                                       channel), counted with multiplicity; every tie at tau is kept
//   acc  = t;  acc = acc + c_k * d_k  for k ascending with c_k != 0, where kept;   out = rne_bf16(acc)
//
// fp32 throughout, one rounding per operation and nothing contracted, as csrc/sigma_step.hip and csrc/latent_blend.hip: the
// restatement in tests/eps_direction_ref.py (same operations, same order) describes the kernel.  A term with c_k == 0 is dropped on the
// host: its rows are never read, so NaN there never reaches out.  slh_eps_direction_momentum is the same combine with SEGA's momentum
// term, an fp32 state per element carried from pass to pass (its kernel below; tests/eps_momentum_ref.py restates it).
//
// slh_direction_threshold: one workgroup per (sample, direction, channel).  A radix select over the 16-bit key in two 8-bit passes:
// count the keys by their high byte, find the bin that holds the n_keep-th largest, count that bin's keys by their low byte, find the
// bin again.  The counters are integers in LDS, 32 copies per bin (one per lane modulo 32, so the lanes of a wave that hit the same
// bin - with real differences nearly all share one exponent - land in 32 different banks); the bin is found from a suffix sum over the
// 256 counts.  Integer arithmetic only, so tau and with it the kept set are exact and the same in every run; no floating-point
// atomics, nothing waits on another workgroup.  Any hw >= 1: the loops stride over the group.
// 16-byte accesses (eight bf16 elements per thread) where every pointer, chw and hw allow them; hw a multiple of 8 means a vector
// never straddles a channel.  Otherwise one element per thread (load_vec / store_vec, step_common.h).
#include <cmath>
#include "step_common.h"
#include "../../include/sliders_hip.h"

namespace {

using namespace slh_step_detail;

constexpr int DIR_MAX = 3;         // prompt pairs per call
constexpr int HIST_COPIES = 32;    // LDS counters per bin

__device__ __forceinline__ unsigned direction_key(float pos, float neg) {
#pragma clang fp contract(off)
    const float d = pos - neg;
    return (__builtin_bit_cast(unsigned, d) & 0x7FFFFFFFu) >> 16;
}

struct direction_threshold_args {
    const __bf16* pos[DIR_MAX]; const __bf16* neg[DIR_MAX];
    int* thr;                                      // [nb][K][C]
    int n_keep[DIR_MAX];
    int K, C, hw, chw;
};

__device__ __forceinline__ void hist_clear(int* hist) {
    for (int i = threadIdx.x; i < 256 * HIST_COPIES; i += 256) hist[i] = 0;
    __syncthreads();
}

__device__ __forceinline__ void hist_count(int* hist, unsigned bin) { atomicAdd(&hist[bin * HIST_COPIES + (threadIdx.x & (HIST_COPIES - 1))], 1); }

// The bin of the `need`-th largest entry of the 256-bin histogram (1 <= need <= the number of entries counted), and how many of that
// bin's entries are still needed once every higher bin is taken.  All 256 threads call it; the result is workgroup-uniform.
__device__ __forceinline__ void hist_select(const int* hist, int* scan, int* result, int need, int& bin, int& rest) {
    __syncthreads();                               // the counts are complete
    const int tid = threadIdx.x;
    int own = 0;
    for (int j = 0; j < HIST_COPIES; ++j) own += hist[tid * HIST_COPIES + ((j + tid) & (HIST_COPIES - 1))];
    int sfx = own;                                 // becomes the number of entries in bins >= tid
    int* buf = scan;
    for (int o = 1; o < 256; o <<= 1) {
        buf[tid] = sfx;
        __syncthreads();
        if (tid + o < 256) sfx += buf[tid + o];
        buf = buf == scan ? scan + 256 : scan;
    }
    const int above = sfx - own;
    if (above < need && sfx >= need) { result[0] = tid; result[1] = need - above; }      // exactly one thread
    __syncthreads();
    bin = result[0];
    rest = result[1];
}

template <bool VEC>
__global__ __launch_bounds__(256) void direction_threshold_kernel(const direction_threshold_args d) {
    constexpr int V = VEC ? 8 : 1;
    __shared__ int hist[256 * HIST_COPIES];
    __shared__ int scan[512];
    __shared__ int result[2];
    const int g = blockIdx.x;                      // (b * K + k) * C + ch
    const int ch = g % d.C, k = (g / d.C) % d.K, b = g / (d.C * d.K);
    const long row = (long)b * d.chw + (long)ch * d.hw;
    // (selects, not d.pos[k]: an argument array indexed by a run-time k would be copied to scratch)
    const __bf16* pos = (k == 0 ? d.pos[0] : k == 1 ? d.pos[1] : d.pos[2]) + row;
    const __bf16* neg = (k == 0 ? d.neg[0] : k == 1 ? d.neg[1] : d.neg[2]) + row;
    int hi = 0, lo = 0, need = k == 0 ? d.n_keep[0] : k == 1 ? d.n_keep[1] : d.n_keep[2];
    for (int pass = 0; pass < 2; ++pass) {
        hist_clear(hist);
        for (int i = threadIdx.x; i < d.hw / V; i += 256) {
            float p[V], n[V];
            load_vec<V>(pos, (long)i * V, p);
            load_vec<V>(neg, (long)i * V, n);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const unsigned key = direction_key(p[e], n[e]);
                if (pass == 0) hist_count(hist, key >> 8);
                else if ((int)(key >> 8) == hi) hist_count(hist, key & 255u);
            }
        }
        if (pass == 0) hist_select(hist, scan, result, need, hi, need);
        else hist_select(hist, scan, result, need, lo, need);
    }
    if (threadIdx.x == 0) d.thr[g] = (hi << 8) | lo;
}

struct eps_direction_args {
    const __bf16* t; __bf16* out;
    const __bf16* pos[DIR_MAX]; const __bf16* neg[DIR_MAX];      // the terms with c != 0, ascending
    const int* thr;                                              // [nb][K][C] or NULL
    float c[DIR_MAX];
    int slot[DIR_MAX];                                           // a term's direction index k (its row of thr)
    int terms, K, C, hw, chw;
    long n;                                                      // nb * chw
};

// acc[e] = t, then acc[e] = acc[e] + c_j * d_j over the kept terms, for the V elements from g on; SUM: g_sum[e], the same products
// summed from +0 in the same order.  The one combine body of both kernels below.
template <int V, bool SUM>
__device__ __forceinline__ void direction_combine(const eps_direction_args& d, const long g, float* acc, float* g_sum) {
#pragma clang fp contract(off)
    const long b = g / d.chw;
    const int ch = (int)(g - b * d.chw) / d.hw;
    load_vec<V>(d.t, g, acc);
    if constexpr (SUM)
        for (int e = 0; e < V; ++e) g_sum[e] = 0.0f;
#pragma unroll
    for (int j = 0; j < DIR_MAX; ++j) {
        if (j >= d.terms) break;
        const unsigned tau = d.thr ? (unsigned)d.thr[(b * d.K + d.slot[j]) * d.C + ch] : 0u;
        float p[V], m[V];
        load_vec<V>(d.pos[j], g, p);
        load_vec<V>(d.neg[j], g, m);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float diff = p[e] - m[e];
            const unsigned key = (__builtin_bit_cast(unsigned, diff) & 0x7FFFFFFFu) >> 16;
            const float prod = d.c[j] * diff;
            const float sum = acc[e] + prod;
            acc[e] = key >= tau ? sum : acc[e];      // a select on the key: a term that is not kept leaves acc's bits
            if constexpr (SUM) {
                const float gs = g_sum[e] + prod;
                g_sum[e] = key >= tau ? gs : g_sum[e];
            }
        }
    }
}

// VEC: eight elements per thread, n a multiple of 8 (and hw, where thr is given)
template <bool VEC>
__global__ __launch_bounds__(256) void eps_direction_kernel(const eps_direction_args d) {
    constexpr int V = VEC ? 8 : 1;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n / V) return;
    float acc[V];
    direction_combine<V, false>(d, i * V, acc, nullptr);
    store_vec<V>(d.out, i * V, acc);
}

// slh_eps_direction_momentum: the combine above with SEGA's momentum, nu the fp32 state between two passes:
//   acc, g  as above (g: the kept products summed from +0)
//   q = s_m * nu;  acc = acc + q;  gm = g + q;  a = beta * nu;  b = omb * gm;  nu' = a + b;  out = rne_bf16(acc);  mom_out = nu'
// mom_out may be mom_in: a thread reads its elements of nu before it writes them, and no other thread touches them.
struct eps_momentum_args {
    eps_direction_args e;
    const float* mom_in; float* mom_out;                         // fp32 [nb][chw]
    float s_m, beta, omb;
};

template <bool VEC>
__global__ __launch_bounds__(256) void eps_direction_momentum_kernel(const eps_momentum_args d) {
#pragma clang fp contract(off)
    constexpr int V = VEC ? 8 : 1;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.e.n / V) return;
    const long g = i * V;
    float acc[V], gm[V], nu[V];
    load_vec<V>(d.mom_in, g, nu);
    direction_combine<V, true>(d.e, g, acc, gm);
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const float q = d.s_m * nu[e];
        acc[e] = acc[e] + q;
        gm[e] = gm[e] + q;
        const float a = d.beta * nu[e];
        const float b = d.omb * gm[e];
        nu[e] = a + b;
    }
    store_vec<V>(d.e.out, g, acc);
    store_vec<V>(d.mom_out, g, nu);
}

// the shape every entry point below takes: nb, chw, hw and K directions
inline int direction_shape_check(const char* name, int nb, int chw, int hw, int K) {
    if (const int rc = shape_check(name, nb, chw, hw)) return rc;
    SLH_CHECK(K >= 1 && K <= DIR_MAX, "%s: K = %d directions (1..%d)", name, K, DIR_MAX);
    return 0;
}

}  // namespace

extern "C" int slh_direction_threshold(const void* const* ptrs, const int32_t* dims, const float*, slh_stream_t stream) {
    SLH_CHECK(ptrs && dims, "slh_direction_threshold: null ptrs / dims");
    const int nb = dims[0], chw = dims[1], hw = dims[2], K = dims[3];
    if (const int rc = direction_shape_check("slh_direction_threshold", nb, chw, hw, K)) return rc;
    direction_threshold_args d;
    d.thr = (int*)ptrs[6];
    SLH_CHECK(d.thr, "slh_direction_threshold: null thr");
    SLH_CHECK(aligned(d.thr, 4), "slh_direction_threshold: the thr pointer (%p) is not 4-byte aligned", (const void*)d.thr);
    const long n = (long)nb * chw, groups = (long)nb * K * (chw / hw);
    bool vec = hw % 8 == 0;
    for (int k = 0; k < DIR_MAX; ++k) {
        d.pos[k] = k < K ? (const __bf16*)ptrs[k] : nullptr;
        d.neg[k] = k < K ? (const __bf16*)ptrs[DIR_MAX + k] : nullptr;
        d.n_keep[k] = k < K ? dims[4 + k] : 0;
        if (k >= K) continue;
        SLH_CHECK(d.pos[k] && d.neg[k], "slh_direction_threshold: null pos[%d] / neg[%d]", k, k);
        SLH_CHECK(d.n_keep[k] >= 1 && d.n_keep[k] <= hw, "slh_direction_threshold: n_keep[%d] = %d (1..hw = %d)", k, d.n_keep[k], hw);
        for (const void* p : {(const void*)d.pos[k], (const void*)d.neg[k]}) {
            SLH_CHECK(aligned(p, 2), "slh_direction_threshold: a bf16 pointer (%p) is not 2-byte aligned", p);
            SLH_CHECK(!overlaps(p, n * 2, d.thr, groups * 4), "slh_direction_threshold: thr overlaps pos[%d] / neg[%d]", k, k);
            vec = vec && aligned(p, 16);
        }
    }
    SLH_CHECK(groups < (1L << 31), "slh_direction_threshold: %ld groups are too many for one launch", groups);
    d.K = K; d.C = chw / hw; d.hw = hw; d.chw = chw;
    const dim3 grid((unsigned)groups);
    if (vec) hipLaunchKernelGGL(direction_threshold_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, d);
    else hipLaunchKernelGGL(direction_threshold_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, d);
    SLH_LAUNCH_CHECK("slh_direction_threshold");
    return 0;
}

// What slh_eps_direction and slh_eps_direction_momentum share: every check of the former, and its launch arguments.  vec: 16-byte
// accesses are possible as far as these pointers and shapes go.
static int direction_fill(const char* name, const void* const* ptrs, const int32_t* dims, const float* coef, eps_direction_args& d, bool& vec) {
    SLH_CHECK(ptrs && dims && coef, "%s: null ptrs / dims / coef", name);
    const int nb = dims[0], chw = dims[1], hw = dims[2], K = dims[3];
    if (const int rc = direction_shape_check(name, nb, chw, hw, K)) return rc;
    d.t = (const __bf16*)ptrs[0];
    d.out = (__bf16*)ptrs[1];
    d.thr = (const int*)ptrs[8];
    SLH_CHECK(d.t && d.out, "%s: null t / out", name);
    SLH_CHECK(aligned(d.thr, 4), "%s: the thr pointer (%p) is not 4-byte aligned", name, (const void*)d.thr);
    const long n = (long)nb * chw, groups = (long)nb * K * (chw / hw);
    vec = chw % 8 == 0 && (!d.thr || hw % 8 == 0);
    for (const void* p : {(const void*)d.t, (const void*)d.out}) {
        SLH_CHECK(aligned(p, 2), "%s: a bf16 pointer (%p) is not 2-byte aligned", name, p);
        vec = vec && aligned(p, 16);
    }
    SLH_CHECK(!overlaps(d.out, n * 2, d.t, n * 2), "%s: out overlaps t", name);
    SLH_CHECK(!overlaps(d.out, n * 2, d.thr, groups * 4), "%s: out overlaps thr", name);
    d.terms = 0;
    for (int k = 0; k < DIR_MAX; ++k) d.pos[k] = d.neg[k] = nullptr, d.c[k] = 0.0f, d.slot[k] = 0;
    for (int k = 0; k < K; ++k) {
        const void* pos = ptrs[2 + k];
        const void* neg = ptrs[2 + DIR_MAX + k];
        SLH_CHECK(pos && neg, "%s: null pos[%d] / neg[%d]", name, k, k);
        SLH_CHECK(std::isfinite(coef[k]), "%s: c[%d] = %f is not finite", name, k, (double)coef[k]);
        for (const void* p : {pos, neg}) {
            SLH_CHECK(aligned(p, 2), "%s: a bf16 pointer (%p) is not 2-byte aligned", name, p);
            SLH_CHECK(!overlaps(d.out, n * 2, p, n * 2), "%s: out overlaps pos[%d] / neg[%d]", name, k, k);
        }
        if (coef[k] == 0.0f) continue;             // skipped, not multiplied: its rows are not read
        vec = vec && aligned(pos, 16) && aligned(neg, 16);
        d.pos[d.terms] = (const __bf16*)pos; d.neg[d.terms] = (const __bf16*)neg;
        d.c[d.terms] = coef[k]; d.slot[d.terms] = k;
        ++d.terms;
    }
    d.K = K; d.C = chw / hw; d.hw = hw; d.chw = chw; d.n = n;
    return 0;
}

extern "C" int slh_eps_direction(const void* const* ptrs, const int32_t* dims, const float* coef, slh_stream_t stream) {
    eps_direction_args d;
    bool vec;
    if (const int rc = direction_fill("slh_eps_direction", ptrs, dims, coef, d, vec)) return rc;
    dim3 grid;
    if (const int rc = launch_grid("slh_eps_direction", vec ? d.n / 8 : d.n, d.n, grid)) return rc;
    if (vec) hipLaunchKernelGGL(eps_direction_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, d);
    else hipLaunchKernelGGL(eps_direction_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, d);
    SLH_LAUNCH_CHECK("slh_eps_direction");
    return 0;
}

extern "C" int slh_eps_direction_momentum(const void* const* ptrs, const int32_t* dims, const float* coef, slh_stream_t stream) {
    static const char* const name = "slh_eps_direction_momentum";
    eps_momentum_args m;
    eps_direction_args& d = m.e;
    bool vec;
    if (const int rc = direction_fill(name, ptrs, dims, coef, d, vec)) return rc;
    m.mom_in = (const float*)ptrs[9];
    m.mom_out = (float*)ptrs[10];
    m.s_m = coef[3]; m.beta = coef[4]; m.omb = coef[5];
    SLH_CHECK(m.mom_in && m.mom_out, "%s: null mom_in / mom_out", name);
    for (const void* p : {(const void*)m.mom_in, (const void*)m.mom_out}) {
        SLH_CHECK(aligned(p, 4), "%s: an fp32 pointer (%p) is not 4-byte aligned", name, p);
        vec = vec && aligned(p, 16);
    }
    SLH_CHECK(std::isfinite(m.s_m) && std::isfinite(m.beta) && std::isfinite(m.omb), "%s: s_m = %f, beta = %f, omb = %f: not finite", name,
              (double)m.s_m, (double)m.beta, (double)m.omb);
    SLH_CHECK(m.s_m != 0.0f, "%s: s_m == 0: without momentum call slh_eps_direction (adding a zero would turn a -0 of acc into +0)", name);
    const long n = d.n, groups = (long)dims[0] * d.K * d.C;
    SLH_CHECK(m.mom_out == m.mom_in || !overlaps(m.mom_out, n * 4, m.mom_in, n * 4), "%s: mom_out overlaps mom_in without being it", name);
    SLH_CHECK(!overlaps(d.out, n * 2, m.mom_in, n * 4), "%s: out overlaps mom_in", name);
    SLH_CHECK(!overlaps(d.out, n * 2, m.mom_out, n * 4), "%s: out overlaps mom_out", name);
    SLH_CHECK(!overlaps(m.mom_out, n * 4, d.t, n * 2), "%s: mom_out overlaps t", name);
    SLH_CHECK(!overlaps(m.mom_out, n * 4, d.thr, groups * 4), "%s: mom_out overlaps thr", name);
    for (int k = 0; k < d.K; ++k)
        for (const void* p : {ptrs[2 + k], ptrs[2 + DIR_MAX + k]})
            SLH_CHECK(!overlaps(m.mom_out, n * 4, p, n * 2), "%s: mom_out overlaps pos[%d] / neg[%d]", name, k, k);
    dim3 grid;
    if (const int rc = launch_grid(name, vec ? n / 8 : n, n, grid)) return rc;
    if (vec) hipLaunchKernelGGL(eps_direction_momentum_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, m);
    else hipLaunchKernelGGL(eps_direction_momentum_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, m);
    SLH_LAUNCH_CHECK(name);
    return 0;
}
