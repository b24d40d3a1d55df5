// Flash-style attention backward (loss.backward() through Attention, train_lora_xl.py:345), head dims 64 (SDXL)
// and 40 / 80 / 160 (SD-1.x, as DT = ceil(D/64) d-tiles with zero-filled columns >= D).  gfx950 only; same
// MFMA/LDS idioms as attention.hip (scores recomputed, never materialised in HBM).
//
//   delta[q]  = sum_d dO[q][d] * O[q][d]
//   P         = exp2(S*c - lse2[q]),  S = Q K^T,  c = scale*log2(e)
//   dP        = dO V^T ;  dS = P * (dP - delta[q])
//   dQ = scale * dS K ;  dK = scale * dS^T Q ;  dV = P^T dO
//
// Two passes, both free of atomics and deterministic:
//   dq kernel  : one wave per 32 queries, loops over key tiles   (tiles: K, V natural; K^T for the dQ product)
//   dkv kernel : one wave per 32 keys,    loops over query tiles (tiles: Q, dO natural; Q^T, dO^T transposed)
// As in the forward the first MFMA of each pair is issued with swapped operands and permuted rows so that the
// probabilities land in registers in exactly the k-order the second MFMA's B operand needs.
// Cross-attention (text K/V carry no gradient in the reference) runs the dq kernel only.
#include "attention_common.h"

using namespace slh_attn_detail;

namespace {

__global__ __launch_bounds__(256) void attn_delta_kernel(const slh_attn_bwd_desc p, int D) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;   // (b, q, h)
    const long total = (long)p.B * p.Tq * p.H;
    if (idx >= total) return;
    const int h = (int)(idx % p.H);
    const long bq = idx / p.H;
    const int b = (int)(bq / p.Tq), q = (int)(bq - (long)b * p.Tq);
    const __bf16* o = (const __bf16*)p.o + bq * p.ldo + h * D;
    const __bf16* g = (const __bf16*)p.d_o + bq * p.lddo + h * D;
    float s = 0.f;
    for (int i = 0; i < D; i += 8) {
        const bf16x8 a = *(const bf16x8*)(o + i);
        const bf16x8 c = *(const bf16x8*)(g + i);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += (float)a[e] * (float)c[e];
    }
    p.delta[((long)b * p.H + h) * p.Tq + q] = s;
}

// ---- dQ ------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const slh_attn_bwd_desc p) {
    __shared__ __attribute__((aligned(16))) char smem[6 * DT * 8192];
    char* sK = smem;                      // [2][DT][64 kv][128 B]
    char* sV = smem + 2 * DT * 8192;      // [2][DT][64 kv][128 B]
    char* sKT = smem + 4 * DT * 8192;     // [2][DT][64 d ][128 B]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane & 31, lhi = lane >> 5;
    const int vb = xcd_virtual_block(blockIdx.x, gridDim.x);      // consecutive values: same head, next 128-row block
    const int nqb = (p.Tq + 127) / 128;
    const int h = (vb / nqb) % p.H, b = vb / (nqb * p.H);
    const int q0 = (vb % nqb) * 128 + wave * 32;
    const int D = head_dim(p);
    const __bf16* K = (const __bf16*)p.k;
    const __bf16* V = (const __bf16*)p.v;
    const __bf16* KT = (const __bf16*)p.kt;

    int qrow = q0 + lrow;
    const bool qvalid = qrow < p.Tq;
    qrow = qvalid ? qrow : p.Tq - 1;
    bf16x8 qf[DT * 4], gf[DT * 4];
#pragma unroll
    for (int ks = 0; ks < DT * 4; ++ks) {
        qf[ks] = load_row_chunk((const __bf16*)p.q + ((long)b * p.Tq + qrow) * p.ldq + h * D, ks * 16 + lhi * 8, D);
        gf[ks] = load_row_chunk((const __bf16*)p.d_o + ((long)b * p.Tq + qrow) * p.lddo + h * D, ks * 16 + lhi * 8, D);
    }
    const float lse2 = p.lse[((long)b * p.H + h) * p.Tq + qrow];
    const float delta = p.delta[((long)b * p.H + h) * p.Tq + qrow];
    const float c = p.scale * 1.4426950408889634f;
    const int prow = perm_row(lrow);

    const int nt = (p.Tk + 63) / 64;
    auto stage = [&](int buf, int t) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const StageRow r(wave + 4 * i, lane);
                const int kv = r.token(t, p.Tk), col = r.col(dt);
                const bool ok = col < D;
                glds16(ok ? K + ((long)b * p.Tk + kv) * p.ldk + h * D + col : (const __bf16*)slh_zero_page,
                       sK + (buf * DT + dt) * 8192 + (wave + 4 * i) * 1024);
                glds16(ok ? V + ((long)b * p.Tk + kv) * p.ldv + h * D + col : (const __bf16*)slh_zero_page,
                       sV + (buf * DT + dt) * 8192 + (wave + 4 * i) * 1024);
                glds16(KT + (((long)b * p.H + h) * (64 * DT) + dt * 64 + r.row) * p.ldkt + t * 64 + r.ks * 8,
                       sKT + (buf * DT + dt) * 8192 + (wave + 4 * i) * 1024);
            }
        }
    };
    f32x16 acc[2 * DT];
#pragma unroll
    for (int dd = 0; dd < 2 * DT; ++dd)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[dd][r] = 0.f;

    stage(0, 0);
    for (int t = 0; t < nt; ++t) {
        lds_dma_syncthreads();       // tile t landed (all waves), everybody is past tile t-1
        if (t + 1 < nt) stage((t + 1) & 1, t + 1);
        const char* cK = sK + (t & 1) * DT * 8192;
        const char* cV = sV + (t & 1) * DT * 8192;
        const char* cKT = sKT + (t & 1) * DT * 8192;
        bf16x8 ds[2][2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const bf16x8 kf = *(const bf16x8*)(cK + dt * 8192 + lds_off(kt * 32 + prow, ks * 2 + lhi));
                    const bf16x8 vf = *(const bf16x8*)(cV + dt * 8192 + lds_off(kt * 32 + prow, ks * 2 + lhi));
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[dt * 4 + ks], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, gf[dt * 4 + ks], dp, 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kv = t * 64 + kt * 32 + 16 * (r >> 3) + 8 * lhi + (r & 7);
                float pv = __builtin_amdgcn_exp2f(s[r] * c - lse2);   // raw v_exp_f32 (argument <= 0), like the forward
                if (kv >= p.Tk) pv = 0.f;
                ds[kt][r >> 3][r & 7] = (__bf16)(pv * (dp[r] - delta));
            }
        }
#pragma unroll
        for (int dd = 0; dd < 2 * DT; ++dd)
#pragma unroll
            for (int kstep = 0; kstep < 4; ++kstep) {
                const bf16x8 kf = *(const bf16x8*)(cKT + (dd >> 1) * 8192 + lds_off((dd & 1) * 32 + lrow, kstep * 2 + lhi));
                acc[dd] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, ds[kstep >> 1][kstep & 1], acc[dd], 0, 0, 0);
            }
    }
    if (qvalid)
        store_acc_row<DT>((__bf16*)p.dq + ((long)b * p.Tq + qrow) * p.lddq + h * D, lhi, D, [&](int dd, int r) { return acc[dd][r] * p.scale; });
}

// ---- dK, dV --------------------------------------------------------------------------------------------
// NBUF = 2: double-buffered query tiles; NBUF = 1 (DT = 3: 4 x 3 x 8 KB per buffer) single-buffered
template <int DT, int NBUF>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const slh_attn_bwd_desc p) {
    __shared__ __attribute__((aligned(16))) char smem[4 * NBUF * DT * 8192];
    char* sQ = smem;                          // [NBUF][DT][64 q][128 B]
    char* sG = smem + NBUF * DT * 8192;       // dO
    char* sQT = smem + 2 * NBUF * DT * 8192;  // [NBUF][DT][64 d][128 B]
    char* sGT = smem + 3 * NBUF * DT * 8192;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane & 31, lhi = lane >> 5;
    const int vb = xcd_virtual_block(blockIdx.x, gridDim.x);      // consecutive values: same head, next 128-row block
    const int nkb = (p.Tk + 127) / 128;
    const int h = (vb / nkb) % p.H, b = vb / (nkb * p.H);
    const int k0 = (vb % nkb) * 128 + wave * 32;
    const int D = head_dim(p);
    const __bf16* Q = (const __bf16*)p.q;
    const __bf16* G = (const __bf16*)p.d_o;
    const __bf16* QT = (const __bf16*)p.qt;
    const __bf16* GT = (const __bf16*)p.dot;

    int krow = k0 + lrow;
    const bool kvalid = krow < p.Tk;
    krow = kvalid ? krow : p.Tk - 1;
    bf16x8 kf[DT * 4], vf[DT * 4];
#pragma unroll
    for (int ks = 0; ks < DT * 4; ++ks) {
        kf[ks] = load_row_chunk((const __bf16*)p.k + ((long)b * p.Tk + krow) * p.ldk + h * D, ks * 16 + lhi * 8, D);
        vf[ks] = load_row_chunk((const __bf16*)p.v + ((long)b * p.Tk + krow) * p.ldv + h * D, ks * 16 + lhi * 8, D);
    }
    const float c = p.scale * 1.4426950408889634f;
    const int prow = perm_row(lrow);
    const int nt = (p.Tq + 63) / 64;
    auto stage = [&](int buf, int t) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const StageRow r(wave + 4 * i, lane);
                const int q = r.token(t, p.Tq), col = r.col(dt);
                const bool ok = col < D;
                const int o = stage_off(buf * DT + dt, wave + 4 * i);
                glds16(ok ? Q + ((long)b * p.Tq + q) * p.ldq + h * D + col : (const __bf16*)slh_zero_page, sQ + o);
                glds16(ok ? G + ((long)b * p.Tq + q) * p.lddo + h * D + col : (const __bf16*)slh_zero_page, sG + o);
                const long trow = (((long)b * p.H + h) * (64 * DT) + dt * 64 + r.row) * p.ldqt + t * 64 + r.ks * 8;
                glds16(QT + trow, sQT + o);
                glds16(GT + trow, sGT + o);
            }
        }
    };
    f32x16 dk[2 * DT], dv[2 * DT];
#pragma unroll
    for (int dd = 0; dd < 2 * DT; ++dd)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[dd][r] = 0.f; dv[dd][r] = 0.f; }

    if (NBUF == 2) stage(0, 0);
    for (int t = 0; t < nt; ++t) {
        if (NBUF == 2) {
            lds_dma_syncthreads();    // tile t landed (all waves), everybody is past tile t-1
            if (t + 1 < nt) stage((t + 1) & 1, t + 1);
        } else {
            __syncthreads();          // everybody finished reading the single buffer
            stage(0, t);
            lds_dma_syncthreads();    // tile t landed for all waves
        }
        const int bufo = (NBUF == 2 ? (t & 1) : 0) * DT * 8192;
        // per-query lse2 / delta straight from global (L1-resident; the arrays are padded by 64 floats whose contents are never used)
        const float* cL = p.lse + ((long)b * p.H + h) * p.Tq + t * 64;
        const float* cD = p.delta + ((long)b * p.H + h) * p.Tq + t * 64;
        bf16x8 pb[2][2], dsb[2][2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const bf16x8 qa = *(const bf16x8*)(sQ + bufo + dt * 8192 + lds_off(qt * 32 + prow, ks * 2 + lhi));
                    const bf16x8 ga = *(const bf16x8*)(sG + bufo + dt * 8192 + lds_off(qt * 32 + prow, ks * 2 + lhi));
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kf[dt * 4 + ks], s, 0, 0, 0);     // S[q][kv = lane]
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga, vf[dt * 4 + ks], dp, 0, 0, 0);   // dP[q][kv = lane]
                }
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int qb = qt * 32 + 16 * hf + 8 * lhi;
                float lv[8], dl[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) { lv[e] = cL[qb + e]; dl[e] = cD[qb + e]; }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int r = hf * 8 + e;
                    float pv = __builtin_amdgcn_exp2f(s[r] * c - lv[e]);
                    const bool dead = t * 64 + qb + e >= p.Tq;
                    if (dead) pv = 0.f;
                    pb[qt][hf][e] = (__bf16)pv;
                    // rows >= Tq: dl / lv come from beyond the arrays (the next head's values, or the padding, which may hold anything -
                    // NaN, Inf): select, never multiply, so that nothing read there reaches the dK MFMA
                    dsb[qt][hf][e] = dead ? (__bf16)0.f : (__bf16)(pv * (dp[r] - dl[e]));
                }
            }
        }
#pragma unroll
        for (int dd = 0; dd < 2 * DT; ++dd)
#pragma unroll
            for (int kstep = 0; kstep < 4; ++kstep) {
                const int o = bufo + (dd >> 1) * 8192 + lds_off((dd & 1) * 32 + lrow, kstep * 2 + lhi);
                const bf16x8 ga = *(const bf16x8*)(sGT + o);
                const bf16x8 qa = *(const bf16x8*)(sQT + o);
                dv[dd] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga, pb[kstep >> 1][kstep & 1], dv[dd], 0, 0, 0);
                dk[dd] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, dsb[kstep >> 1][kstep & 1], dk[dd], 0, 0, 0);
            }
    }
    if (kvalid) {
        // (dK is scaled and dV is not, and their stores alternate: stated here, not two passes of store_acc_row)
        __bf16* DK = (__bf16*)p.dk + ((long)b * p.Tk + krow) * p.lddk + h * D;
        __bf16* DV = (__bf16*)p.dv + ((long)b * p.Tk + krow) * p.lddv + h * D;
#pragma unroll
        for (int dd = 0; dd < 2 * DT; ++dd)
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const int dcol = dd * 32 + qd * 8 + lhi * 4;
                if (dcol < D) {
                    bf16x4 a, g;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        a[e] = (__bf16)(dk[dd][qd * 4 + e] * p.scale);
                        g[e] = (__bf16)dv[dd][qd * 4 + e];
                    }
                    *(bf16x4*)(DK + dcol) = a;
                    *(bf16x4*)(DV + dcol) = g;
                }
            }
    }
}

// the descriptor checks of slh_attn_bwd
static int attn_bwd_check(const slh_attn_bwd_desc* d) {
    SLH_CHECK(d && d->q && d->k && d->v && d->o && d->d_o && d->lse && d->delta && d->dq && d->kt,
              "slh_attn_bwd: null pointer");
    const int D = head_dim(*d);
    SLH_CHECK(D % 8 == 0 && D <= 192, "slh_attn_bwd: head_dim %d unsupported", D);
    SLH_CHECK(d->ldq % 8 == 0 && d->ldk % 8 == 0 && d->ldv % 8 == 0 && d->ldo % 8 == 0 && d->lddo % 8 == 0 &&
                  d->lddq % 4 == 0 && d->ldkt % 64 == 0,
              "slh_attn_bwd: alignment");
    SLH_CHECK(d->ldkt >= ((d->Tk + 63) / 64) * 64, "slh_attn_bwd: KT must be padded to a multiple of 64 keys");
    if (d->need_dkv) {
        SLH_CHECK(d->qt && d->dot && d->dk && d->dv, "slh_attn_bwd: dK/dV need qt, dot, dk, dv");
        SLH_CHECK(d->ldqt % 64 == 0 && d->ldqt >= ((d->Tq + 63) / 64) * 64 && d->lddk % 4 == 0 && d->lddv % 4 == 0,
                  "slh_attn_bwd: QT/dOT padding");
    }
    return 0;
}

// The one place each that picks the dq / dkv instantiation: slh_attn_bwd launches through them, slh_attn_bwd_kernel_names names
// through them (common.h: slh_launch records the template instead of launching it while a name sink is set).
static void launch_bwd_dq(const slh_attn_bwd_desc* d, hipStream_t s) {
    const int DT = d_tiles(*d);
    const int gq = (int)((long)((d->Tq + 127) / 128) * d->H * d->B);
    if (DT == 1) slh_launch<attn_bwd_dq_kernel<1>>(gq, 256, s, *d, "attn_bwd_dq_kernel<1>");
    else if (DT == 2) slh_launch<attn_bwd_dq_kernel<2>>(gq, 256, s, *d, "attn_bwd_dq_kernel<2>");
    else slh_launch<attn_bwd_dq_kernel<3>>(gq, 256, s, *d, "attn_bwd_dq_kernel<3>");
}
static void launch_bwd_dkv(const slh_attn_bwd_desc* d, hipStream_t s) {
    const int DT = d_tiles(*d);
    const int gk = (int)((long)((d->Tk + 127) / 128) * d->H * d->B);
    if (DT == 1) slh_launch<attn_bwd_dkv_kernel<1, 2>>(gk, 256, s, *d, "attn_bwd_dkv_kernel<1, 2>");
    else if (DT == 2) slh_launch<attn_bwd_dkv_kernel<2, 2>>(gk, 256, s, *d, "attn_bwd_dkv_kernel<2, 2>");
    else slh_launch<attn_bwd_dkv_kernel<3, 1>>(gk, 256, s, *d, "attn_bwd_dkv_kernel<3, 1>");
}

}  // namespace

extern "C" int slh_attn_bwd(const slh_attn_bwd_desc* d, slh_stream_t stream) {
    if (attn_bwd_check(d)) return -1;
    hipStream_t s = (hipStream_t)stream;
    const long total = (long)d->B * d->Tq * d->H;
    hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, *d, head_dim(*d));
    launch_bwd_dq(d, s);
    if (d->need_dkv) launch_bwd_dkv(d, s);
    SLH_LAUNCH_CHECK("slh_attn_bwd");
    return 0;
}

// the names of the dq and dkv instantiations slh_attn_bwd would launch for d, as rocprofv3 prints them ("attn_bwd_dq_kernel<2>",
// "attn_bwd_dkv_kernel<2, 2>"; dkv is the empty string with need_dkv = 0): the descriptor checks and launch_bwd_dq / launch_bwd_dkv run
// with the launches replaced by a record of the selected template.  No device needed, nothing launched.  (attn_delta_kernel, which
// every call launches first, has one form.)
extern "C" int slh_attn_bwd_kernel_names(const slh_attn_bwd_desc* d, char* dq, char* dkv, int cap) {
    SLH_CHECK(dq && dkv && cap >= 32, "slh_attn_bwd_kernel_names: buffers");
    dq[0] = dkv[0] = 0;
    if (attn_bwd_check(d)) return -1;
    slh_name_sink_set(dq, cap);
    launch_bwd_dq(d, nullptr);
    if (d->need_dkv) {
        slh_name_sink_set(dkv, cap);
        launch_bwd_dkv(d, nullptr);
    }
    slh_name_sink_set(nullptr, 0);
    if (!dq[0] || (d->need_dkv && !dkv[0])) { slh_set_error("slh_attn_bwd_kernel_names: internal: no launch site recorded a name"); return -3; }
    return 0;
}
