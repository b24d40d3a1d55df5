// The pieces the attention kernels share (attention.hip, attention_bwd.hip): the XCD-aware block order, the permuted tile row, the
// zero-filled fragment load, the row arithmetic of the staging copies, the online-softmax tile of the forward kernels and the
// accumulator store.  Each is stated here once and leaves every kernel's registers, LDS and (but for a few prologue instructions)
// code as they were.  What differs between the kernels stays in them (the interleaved MFMA chains of the backward, the key-split
// pipeline and its merge) - and so do the MFMA loops and the addresses of the staging copies: out of a helper hipcc places their
// address arithmetic differently, and VGPR counts move (tried: score tile <4,1,true> 119 -> 122, second product <4,2,true> 170 -> 178,
// dq staging <1> 160 -> 156).
// gfx950 only.
#pragma once
#include "common.h"
#include "../../include/sliders_hip.h"

namespace slh_attn_detail {

// head dim of a descriptor (D = 0 means 64) and its DT = ceil(D/64) 64-wide d-tiles
template <class Desc>
__host__ __device__ __forceinline__ int head_dim(const Desc& d) { return d.D > 0 ? d.D : 64; }
template <class Desc>
__host__ __device__ __forceinline__ int d_tiles(const Desc& d) { return (head_dim(d) + 63) / 64; }

// XCD-aware block order (block i runs on XCD i % 8, each with its own 4 MB L2): every XCD gets a contiguous run of the
// (sample, head, query block) sequence with the query block fastest, so the query blocks that share one head's K / V
// meet in ONE L2 instead of all eight (counter pass of the round-3 tree: 103 MB fetched per T = 4096 launch for 31 MB of
// Q, K, V; L2 hit 52 %).  vb of nblk workgroups -> the virtual block id whose consecutive values land on the same XCD.
__device__ __forceinline__ int xcd_virtual_block(const int vb, const int nblk) {
    const int qd = nblk >> 3, rm = nblk & 7;
    const int xcd = vb & 7, idx = vb >> 3;
    return (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + idx;
}

// permuted tile row for the A operand of the transposed first product (swap bits 2 and 3): the C-layout register order is then
// exactly the k-order the B operand of the second product expects
__device__ __forceinline__ int perm_row(int r) {
    return (r & 3) | (((r >> 3) & 1) << 2) | (((r >> 2) & 1) << 3) | (r & 16);
}

// 8 elements of a row as a B-operand fragment; columns >= D are zero
__device__ __forceinline__ bf16x8 load_row_chunk(const __bf16* base, int col, int D) {
    if (col < D) return *(const bf16x8*)(base + col);
    bf16x8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = (__bf16)0.f;
    return z;
}

// Staging: one glds16 copies 8 rows of a 64-row tile (a "group": lane = 8 * row in group + 16-byte slot), and the slot a lane
// fetches is swizzled by its row, the way lds_off reads it back.  The lane's row and slot in group `group` of a tile ...
struct StageRow {
    int row, ks;
    __device__ __forceinline__ StageRow(int group, int lane) : row(group * 8 + (lane >> 3)), ks((lane & 7) ^ ((row >> 1) & 7)) {}
    // the first of its 8 columns in d-tile dt (columns >= D come from slh_zero_page)
    __device__ __forceinline__ int col(int dt) const { return dt * 64 + ks * 8; }
    // its token in token tile t of T tokens (rows past the end repeat the last token; the kernels mask them)
    __device__ __forceinline__ int token(int t, int T) const { const int x = t * 64 + row; return x < T ? x : T - 1; }
};
// ... and the byte offset of that group in tile `tile` of a [tiles][64][128 B] LDS array
__device__ __forceinline__ int stage_off(int tile, int group) { return tile * 8192 + group * 1024; }

// One 64-key tile of the online softmax.  s[kt][r] = S[q = lrow][kv = kt*32 + 16*(r>>3) + 8*lhi + (r&7)] of the tile; c =
// scale * log2(e).  Updates the running maximum and row sum of the lane's half row, leaves the probabilities in pb as the B
// fragments of the second product and returns alpha, the factor the accumulators are owed (rescale_if_moved).
__device__ __forceinline__ float softmax_tile(const f32x16 (&s)[2], const float c, float& m_run, float& l_run, bf16x8 (&pb)[2][2]) {
    float mx = s[0][0];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kt][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    // raw v_exp_f32 (arguments <= 0; results below 2^-126 flush to 0, which is what a probability that small is
    // worth) - the libm exp2f wraps every call in a denormal-range fixup that quadruples the VALU work here
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
    const float mc = m_new * c;
    m_run = m_new;
    // scalar fp32 softmax arithmetic (attention.hip is built with -fno-slp-vectorize): v_pk_fma/add/mul_f32 beside MFMAs cost more
    // than the two plain instructions they replace (same-box A/B, T = 4096: 149.9 -> 141.0 us)
    float ps = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kt][r], c, -mc));
            ps += pv;
            pb[kt][r >> 3][r & 7] = (__bf16)pv;
        }
    l_run = l_run * alpha + ps;
    return alpha;
}
// the running maximum settles after the first tiles: rescale the accumulators only when some row of the
// wave actually moved (alpha == 1 exactly otherwise, so skipping is bit-identical)
template <int N>
__device__ __forceinline__ void rescale_if_moved(f32x16 (&o)[N], const float alpha) {
    if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
        for (int dd = 0; dd < N; ++dd)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dd][r] *= alpha;
    }
}

// Accumulator store: the lane's 32 * DT d-values of one row go out as bf16x4 stores, columns < D only.  value(dd, r) is
// element r of accumulator dd as it is to be stored - the caller states the scaling (or none) there.
template <int DT, class F>
__device__ __forceinline__ void store_acc_row(__bf16* O, int lhi, int D, F value) {
#pragma unroll
    for (int dd = 0; dd < 2 * DT; ++dd)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            const int dcol = dd * 32 + qd * 8 + lhi * 4;
            if (dcol < D) {
                bf16x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (__bf16)value(dd, qd * 4 + e);
                *(bf16x4*)(O + dcol) = v;
            }
        }
}

}  // namespace slh_attn_detail
