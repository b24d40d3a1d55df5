// slh_lora_merge: fold adapters into the frozen weights, in the layouts the GEMM kernels stream (include/sliders_hip.h).
//
//   out[n][k] = bf16( float(base[n][k]) + sum_{r < R} (c[r] * U[n - n0][r]) * D[r][k] )           n0 <= n < n0 + rows
//
// For inference the adapters are constants of a denoise loop, so W' = W + sum_i s_i (alpha_i / r_i) B_i A_i is computed once and the
// adapter-free programs run on it: any rank, any number of sliders (their factors are concatenated along R, the scales live in c).
// One workgroup owns 64 rows of one item and walks K, so the row sums of a LayerNorm-folded copy need no atomics and every
// addition happens in an order fixed by the launch geometry alone:
//   * the adapter sum is one fp32 fma chain per element, r ascending: acc = fma(c[r] * U[n][r], D[r][k], acc), from acc = 0;
//   * a row sum adds a thread's 8-element slots in ascending k, then the 8 slot lanes (xor 1, 2, 4), then the two K halves.
// A thread computes 4 rows x 8 k (one 16-byte slot per row): per adapter row it needs 4 U and 8 D values for 32 fmas, all served
// by the L1 / L2 (U and D are a few hundred KB); base is read and out written once, 16 bytes at a time.
#include "common.h"
#include "../../include/sliders_hip.h"

namespace {
// element offset of the 16-byte slot ks (k = 8 ks) of stored row n
__device__ __forceinline__ long merge_slot_off(const slh_lora_merge_item& it, int n, int ks) {
    if (it.w_layout == 0) return (long)n * it.ld + (long)ks * 8;
    // pack_gemm_w: [N/64][K/64] blocks of 64 rows x 8 slots x 8 elements, slot s of row r at physical slot s ^ ((r >> 1) & 7)
    const int r = n & 63;
    return ((((long)(n >> 6) * (it.K >> 6) + (ks >> 3)) * 64 + r) << 6) + (((ks & 7) ^ ((r >> 1) & 7)) << 3);
}

__global__ __launch_bounds__(256) void lora_merge_kernel(const slh_lora_merge_item* items, const int32_t* prefix, int n_items) {
    const int bid = blockIdx.x;
    const int lo = batch_find(prefix, n_items, bid);
    const slh_lora_merge_item it = items[lo];
    const int row0 = (bid - prefix[lo]) * 64;   // first row of this workgroup, relative to the item
    const int tid = threadIdx.x;
    const int half = tid >> 7, rg = (tid >> 3) & 15, slot = tid & 7;
    const int R = it.R, KS = it.K >> 3;
    const __bf16* base = (const __bf16*)it.base;
    __bf16* out = (__bf16*)it.out;
    const bool fold = it.gamma != nullptr;

    int irow[4];                                // item-relative rows of this thread, clamped for the loads
    bool rok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = row0 + rg + 16 * j;
        rok[j] = i < it.rows;
        irow[j] = rok[j] ? i : it.rows - 1;
    }
    float s_acc[4] = {0.f, 0.f, 0.f, 0.f}, b_acc[4] = {0.f, 0.f, 0.f, 0.f};

    for (int ks0 = 0; ks0 < KS; ks0 += 16) {
        const int ks_raw = ks0 + half * 8 + slot;
        const bool kok = ks_raw < KS;
        const int ks = kok ? ks_raw : KS - 1;
        const int k = ks * 8;
        long off[4];
        bf16x8 bv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            off[j] = merge_slot_off(it, it.n0 + irow[j], ks);
            bv[j] = *(const bf16x8*)(base + off[j]);
        }
        float acc[4][8];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
        for (int r0 = 0; r0 < R; r0 += 4) {
            float cu[4][4];
            f32x4 dl[4], dh[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool live = r0 + q < R;
                const int rr = live ? r0 + q : R - 1;
                const float cq = live ? it.c[rr] : 0.f;
                const float* dp = it.d + (long)rr * it.ldd + k;
                dl[q] = *(const f32x4*)dp;
                dh[q] = *(const f32x4*)(dp + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) cu[j][q] = cq * it.u[(long)irow[j] * it.ldu + rr];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[j][e] = __builtin_fmaf(cu[j][q], dl[q][e], acc[j][e]);
                        acc[j][e + 4] = __builtin_fmaf(cu[j][q], dh[q][e], acc[j][e + 4]);
                    }
        }
        if (!fold) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bf16x8 ov;
#pragma unroll
                for (int e = 0; e < 8; ++e) ov[e] = (__bf16)((float)bv[j][e] + acc[j][e]);
                if (rok[j] && kok) *(bf16x8*)(out + off[j]) = ov;
            }
        } else {
            const bf16x8 gv = *(const bf16x8*)((const __bf16*)it.gamma + k);
            const bf16x8 tv = *(const bf16x8*)((const __bf16*)it.beta + k);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bf16x8 ov;
                float s = 0.f, b = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float m = (float)bv[j][e] + acc[j][e];
                    ov[e] = (__bf16)(m * (float)gv[e]);
                    s += (float)ov[e];
                    b += round_bf16(m) * (float)tv[e];
                }
                if (rok[j] && kok) {
                    *(bf16x8*)(out + off[j]) = ov;
                    s_acc[j] += s;
                    b_acc[j] += b;
                }
            }
        }
    }
    if (!fold) return;
    __shared__ float red[2][2][64];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float s = s_acc[j], b = b_acc[j];
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            s += __shfl_xor(s, o, 64);
            b += __shfl_xor(b, o, 64);
        }
        if (slot == 0) { red[half][0][rg + 16 * j] = s; red[half][1][rg + 16 * j] = b; }
    }
    __syncthreads();
    if (tid < 64 && row0 + tid < it.rows) {
        const int n = it.n0 + row0 + tid;
        it.lns[n] = red[0][0][tid] + red[1][0][tid];
        const float bias = it.bias ? (float)((const __bf16*)it.bias)[n] : 0.f;
        it.lnb[n] = bias + (red[0][1][tid] + red[1][1][tid]);
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

extern "C" int slh_lora_merge_blocks(const slh_lora_merge_item* it) {
    SLH_CHECK(it && it->base && it->out && it->u && it->d && it->c, "slh_lora_merge: null pointer in item");
    SLH_CHECK(it->rows > 0 && it->n0 >= 0 && (long)it->n0 + it->rows <= it->N, "slh_lora_merge: rows [%d, %d + %d) outside the %d stored rows",
              it->n0, it->n0, it->rows, it->N);
    SLH_CHECK(it->R >= 1 && it->ldu >= it->R, "slh_lora_merge: R = %d, ldu = %d", it->R, it->ldu);
    SLH_CHECK(it->K > 0 && it->K % 8 == 0 && it->ldd >= it->K && it->ldd % 4 == 0, "slh_lora_merge: K = %d, ldd = %d", it->K, it->ldd);
    SLH_CHECK(it->w_layout == 0 || it->w_layout == 1, "slh_lora_merge: w_layout %d", it->w_layout);
    if (it->w_layout == 1) SLH_CHECK(it->K % 64 == 0, "slh_lora_merge: tile-packed matrices have K %% 64 == 0 (K = %d)", it->K);
    else SLH_CHECK(it->ld >= it->K && it->ld % 8 == 0, "slh_lora_merge: row-major ld = %d (K = %d)", it->ld, it->K);
    SLH_CHECK(al16(it->base) && al16(it->out) && al16(it->d), "slh_lora_merge: base / out / d must be 16-byte aligned");
    if (it->gamma)
        SLH_CHECK(it->beta && it->lns && it->lnb && al16(it->gamma) && al16(it->beta), "slh_lora_merge: a folded copy needs gamma, beta (16-byte aligned), lns, lnb");
    return (it->rows + 63) / 64;
}

extern "C" int slh_lora_merge(const slh_lora_merge_desc* d, slh_stream_t stream) {
    SLH_CHECK(d && d->items && d->prefix && d->n > 0 && d->total > 0, "slh_lora_merge: null pointer / empty");
    hipLaunchKernelGGL(lora_merge_kernel, dim3(d->total), dim3(256), 0, (hipStream_t)stream, d->items, d->prefix, d->n);
    SLH_LAUNCH_CHECK("slh_lora_merge");
    return 0;
}
