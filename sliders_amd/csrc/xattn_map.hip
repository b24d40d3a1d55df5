// slh_xattn_map: where the prompt's words live in a cross-attention layer (SliderEditor.word_map, docs/EDIT.md "A mask from a word").
//
//   term[b][i] = coef * sum_{h < H} sum_{j < Tk} wt[b][j] * P[b0 + b, h, i, j],      P = softmax_j(scale * q_i . k_j) over the Tk real keys
//   out = term (accumulate 0)  or  out + term (accumulate 1: the layers of one level, ordered by the stream)
//
// The probabilities are never formed in memory: per query row and head the kernel keeps the running maximum m, the denominator l and
// the weighted numerator a (the flash form, in blocks of KB keys: one rescale per block), and a / l is the head's share.
//
// Form: plain vector code, one query row per lane, the head's key slice [Tk][D] staged in LDS and read back as broadcasts.
//   - The row's q stays in registers as packed bf16 (D / 2 dwords: 32 at the head dim 64 of SDXL, 96 at 192); every lane of a wave
//     reads the SAME key address, so the LDS read is a broadcast: no bank conflict at any D, no padding of the slice.
//   - The key loop runs over exactly Tk keys (a last block of Tk % KB): the 77 text keys cost 77 keys, not the 128 an MFMA form
//     would pay for two 64-key tiles (or 80 with 16-key tiles, plus the masking of the tail in the softmax).
//   - A workgroup owns 64 query rows of one sample.  Its W waves take the heads round-robin (wave w: heads w, w + W, ...), each with
//     its own slice in LDS; after every round of W heads the shares are exchanged through LDS and wave 0 adds them IN HEAD ORDER, so
//     the sum over the heads is one chain in ascending h whatever W is.  No atomics, no other workgroup is waited for.
//   - LDS: W * Tk * D * 2 bytes for the slices + W * 256 for the exchange, W = min(H, 8, what fits 64 KB): 6 waves and 60 KB at
//     SDXL's shapes (Tk 77, D 64), two workgroups per CU; one wave and 48 KB at Tk 128, D 192.
// The work is small (2 * Tq * Tk * D flops per head: about 0.1 GFLOP for SDXL's 64 x 64 level) and runs in side passes only; what
// this form gives up against MFMA is throughput it does not need, what it gains is one rounding model (fp32 fma chains) for the bound.
#include "common.h"
#include "../../include/sliders_hip.h"

namespace {

constexpr int XM_ROWS = 64;        // query rows per workgroup: one per lane
constexpr int XM_KB = 8;           // keys per softmax block
constexpr int XM_MAX_WAVES = 8;
constexpr int XM_LDS_BUDGET = 64 * 1024;

__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

// DT: head-dim tier (the row's q is DT / 8 uint4 registers, chunks past D are skipped by a wave-uniform test)
template <int DT>
__global__ __launch_bounds__(XM_MAX_WAVES * 64) void xattn_map_kernel(const slh_xattn_map_desc d, const int W) {
    extern __shared__ __attribute__((aligned(16))) unsigned char xm_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D = d.D, Tk = d.Tk, H = d.H;
    const int b = blockIdx.y;
    const int row = blockIdx.x * XM_ROWS + lane;
    const bool live = row < d.Tq;
    const int rowc = live ? row : d.Tq - 1;                       // lanes past Tq compute the last row again and store nothing
    const int slice = Tk * D;                                     // bf16 elements of one head's keys
    uint4* ks = (uint4*)(xm_lds + (size_t)wave * slice * 2);
    float* share = (float*)(xm_lds + (size_t)W * slice * 2);      // [W][64]
    const __bf16* qrow = (const __bf16*)d.q + ((long)(d.b0 + b) * d.Tq + rowc) * d.ldq;
    const __bf16* kb = (const __bf16*)d.k + (long)(d.b0 + b) * Tk * d.ldk;
    const float* wt = d.wt + (long)b * Tk;
    const int dch = D >> 3;                                       // 16-byte chunks of a head row
    float tot = 0.0f;
    for (int h0 = 0; h0 < H; h0 += W) {
        const int h = h0 + wave;
        uint4 qv[DT / 8];
        if (h < H) {
            // this wave's slice: [Tk][D] of head h, 16 bytes per lane and trip
            for (int c = lane; c < Tk * dch; c += 64) {
                const int j = c / dch, cc = c - j * dch;
                ks[c] = *(const uint4*)(kb + (long)j * d.ldk + h * D + cc * 8);
            }
#pragma unroll
            for (int c = 0; c < DT / 8; ++c)
                if (c < dch) qv[c] = *(const uint4*)(qrow + h * D + c * 8);
        }
        __syncthreads();                                          // every wave arrives, also one without a head in this round
        if (h < H) {
            float m = -INFINITY, l = 0.0f, a = 0.0f;
            for (int j0 = 0; j0 < Tk; j0 += XM_KB) {
                float s[XM_KB];
#pragma unroll
                for (int jj = 0; jj < XM_KB; ++jj) s[jj] = 0.0f;
#pragma unroll
                for (int c = 0; c < DT / 8; ++c) {
                    if (c < dch) {
                        uint4 qq = qv[c];
                        // opaque copy: without it the bf16 -> fp32 conversions of the whole row are hoisted out of the key loop
                        // (D more registers: spills at D > 64)
                        asm volatile("" : "+v"(qq.x), "+v"(qq.y), "+v"(qq.z), "+v"(qq.w));
                        const float q0 = bf_lo(qq.x), q1 = bf_hi(qq.x), q2 = bf_lo(qq.y), q3 = bf_hi(qq.y);
                        const float q4 = bf_lo(qq.z), q5 = bf_hi(qq.z), q6 = bf_lo(qq.w), q7 = bf_hi(qq.w);
#pragma unroll
                        for (int jj = 0; jj < XM_KB; ++jj) {
                            const int j = min(j0 + jj, Tk - 1);   // the tail block reads the last key again; its logits are dropped below
                            const uint4 kk = ks[j * dch + c];     // one address per wave: a broadcast
                            float t = s[jj];
                            t = fmaf(q0, bf_lo(kk.x), t); t = fmaf(q1, bf_hi(kk.x), t);
                            t = fmaf(q2, bf_lo(kk.y), t); t = fmaf(q3, bf_hi(kk.y), t);
                            t = fmaf(q4, bf_lo(kk.z), t); t = fmaf(q5, bf_hi(kk.z), t);
                            t = fmaf(q6, bf_lo(kk.w), t); t = fmaf(q7, bf_hi(kk.w), t);
                            s[jj] = t;
                        }
                    }
                }
                float bm = -INFINITY;
#pragma unroll
                for (int jj = 0; jj < XM_KB; ++jj) {
                    s[jj] = j0 + jj < Tk ? s[jj] * d.scale : -INFINITY;
                    bm = fmaxf(bm, s[jj]);
                }
                const float mn = fmaxf(m, bm);                    // finite: key j0 is a real key
                const float alpha = __expf(m - mn);               // 0 on the first block (m = -inf), 1 where the maximum stays
                float ls = 0.0f, as = 0.0f;
#pragma unroll
                for (int jj = 0; jj < XM_KB; ++jj) {
                    const float e = __expf(s[jj] - mn);           // 0 for the dropped keys of the tail (-inf)
                    const float w = j0 + jj < Tk ? wt[j0 + jj] : 0.0f;
                    ls = ls + e;
                    as = fmaf(w, e, as);
                }
                l = fmaf(l, alpha, ls);
                a = fmaf(a, alpha, as);
                m = mn;
            }
            share[wave * 64 + lane] = a / l;                      // l >= 1 up to rounding: the maximum's own term
        }
        __syncthreads();
        if (wave == 0) {
            const int n = min(W, H - h0);
            for (int w = 0; w < n; ++w) tot = tot + share[w * 64 + lane];     // heads h0 .. h0 + n - 1, ascending
        }
        __syncthreads();                                          // the next round writes share and the slices again
    }
    if (wave == 0 && live) {
        const float term = d.coef * tot;
        float* o = d.out + (long)b * d.Tq + row;
        *o = d.accumulate ? *o + term : term;
    }
}

inline int xm_waves(const slh_xattn_map_desc* d) {
    const int slice = d->Tk * d->D * 2 + 64 * 4;
    int w = XM_LDS_BUDGET / slice;
    if (w > XM_MAX_WAVES) w = XM_MAX_WAVES;
    if (w > d->H) w = d->H;
    return w < 1 ? 1 : w;
}

}  // namespace

extern "C" int slh_xattn_map(const slh_xattn_map_desc* d, slh_stream_t stream) {
    SLH_CHECK(d && d->q && d->k && d->wt && d->out, "slh_xattn_map: null q / k / wt / out");
    SLH_CHECK(d->D >= 8 && d->D <= 192 && d->D % 8 == 0, "slh_xattn_map: D = %d: expected a multiple of 8 in 8 .. 192", d->D);
    SLH_CHECK(d->Tk >= 1 && d->Tk <= 128, "slh_xattn_map: Tk = %d: expected 1 .. 128 keys", d->Tk);
    SLH_CHECK(d->Tq >= 1 && d->H >= 1, "slh_xattn_map: Tq = %d, H = %d: expected both >= 1", d->Tq, d->H);
    SLH_CHECK(d->B >= 1 && d->nb >= 1 && d->b0 >= 0 && (long)d->b0 + d->nb <= d->B,
              "slh_xattn_map: samples b0 = %d .. b0 + nb = %ld of B = %d", d->b0, (long)d->b0 + d->nb, d->B);
    SLH_CHECK((long)d->H * d->D <= d->ldq && d->ldq % 8 == 0, "slh_xattn_map: ldq = %d: expected a multiple of 8 >= H * D = %ld", d->ldq,
              (long)d->H * d->D);
    SLH_CHECK((long)d->H * d->D <= d->ldk && d->ldk % 8 == 0, "slh_xattn_map: ldk = %d: expected a multiple of 8 >= H * D = %ld", d->ldk,
              (long)d->H * d->D);
    SLH_CHECK(((uintptr_t)d->q & 15) == 0 && ((uintptr_t)d->k & 15) == 0, "slh_xattn_map: q and k must be 16-byte aligned");
    SLH_CHECK(d->nb <= 65535, "slh_xattn_map: nb = %d: at most 65535 collected samples", d->nb);
    SLH_CHECK(d->accumulate == 0 || d->accumulate == 1, "slh_xattn_map: accumulate = %d (0 write, 1 add)", d->accumulate);
    const int W = xm_waves(d);
    const size_t lds = (size_t)W * ((size_t)d->Tk * d->D * 2 + 64 * 4);
    const dim3 grid((unsigned)((d->Tq + XM_ROWS - 1) / XM_ROWS), (unsigned)d->nb);
    const hipStream_t s = (hipStream_t)stream;
    if (d->D <= 64) hipLaunchKernelGGL(xattn_map_kernel<64>, grid, dim3(W * 64), lds, s, *d, W);
    else if (d->D <= 128) hipLaunchKernelGGL(xattn_map_kernel<128>, grid, dim3(W * 64), lds, s, *d, W);
    else hipLaunchKernelGGL(xattn_map_kernel<192>, grid, dim3(W * 64), lds, s, *d, W);
    SLH_LAUNCH_CHECK("slh_xattn_map");
    return 0;
}
