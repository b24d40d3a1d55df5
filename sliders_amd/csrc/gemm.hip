// bf16 MFMA GEMM / implicit-GEMM 3x3 convolution with fused LoRA-up, bias, time-embedding, residual
// and GEGLU epilogues.  gfx950 (CDNA4) only.
//
//   C[M][N] = epi( A[M][K] . W[N][K]^T )
//
// Structure: 256 threads = 4 waves (2 x 2), block tile (64*MI) x (64*NI), K-step 64, double-buffered LDS
// filled with global_load_lds_dwordx4 (16 B/lane, no VGPR round trip), one barrier per K-step.
// LDS rows are 128 B (64 bf16); the 16-byte slot index is XOR-swizzled with (row>>1)&7 so that the 16-lane
// groups of ds_read_b128 touch 16 distinct 16-B bank slots.  global_load_lds writes lane-linear, so the
// swizzle is applied to the per-lane SOURCE address (inverse permutation) and again on the read.
// MFMA operand roles are swapped (W rows feed the A operand, activation rows the B operand) so that each
// lane ends up with 4 consecutive output columns of ONE output row per accumulator quad: 8-byte stores,
// per-lane LoRA T[m][0..3], per-lane residual reads.
//
// Reference semantics replaced: torch.nn.functional.linear / conv2d inside diffusers-0.20.2
// (ResnetBlock2D.conv1/conv2/conv_shortcut, Downsample2D.conv, Upsample2D.conv, Attention.to_q/k/v/out,
// GEGLU.proj, FeedForward.net.2, Transformer2DModel.proj_in/out) plus the LoRA branch of
// trainscripts/textsliders/lora.py:108-112.
#include "gemm_common.h"
#include "gemm_dispatch.h"
#include <cstdlib>
#include <cstring>

using namespace slh_gemm_detail;

namespace {

// WM = waves along M (2: 4-wave workgroup, tile 64*MI x 64*NI; 4: 8-wave workgroup, tile 128*MI x 64*NI - twice
// the W-tile reuse per byte pulled from L2, which is what bounds these kernels)
// waves per SIMD the LDS footprint allows (workgroups per CU x waves per workgroup / 4 SIMDs); handed to the
// register allocator as the occupancy target so the epilogue's temporaries cannot cost a resident wave
constexpr int gemm_waves_per_simd(int MI, int NI, int STAGES, bool LORA, int WM) {
    const int lds = STAGES * (32 * MI * WM + 64 * NI + (LORA ? 32 : 0)) * 128;
    int blocks = (160 * 1024) / lds;
    int w = blocks * 2 * WM / 4;
    if (LORA && MI * NI == 1 && WM == 2 && w > 4) w = 4;   // 64x64 + fused LoRA needs ~110 registers: 4 waves, not 5
    return w < 1 ? 1 : (w > 8 ? 8 : w);
}


template <int MI, int NI, int MODE, int STAGES, bool LORA, int WM, bool XA = false>
__global__ __launch_bounds__(128 * WM, gemm_waves_per_simd(MI, NI, STAGES, LORA, WM)) void gemm_kernel(const GemmArgs p) {
    constexpr int NW = 2 * WM;
    constexpr int BM = 32 * MI * WM;
    constexpr int BN = 64 * NI;
    constexpr int XI = BM / (8 * NW);  // glds instructions per wave for the X tile (8 rows each)
    constexpr int WI = BN / (8 * NW);
    static_assert(XI >= 1 && WI >= 1, "tile too small for this many waves");
    // LORA: the rank-r down matrix A (lora_down, [r][K], r <= 12, zero-padded to 32 rows) rides along as a third
    // operand tile; every wave multiplies it with the X fragments it already holds, so T = X.A^T of the block's own
    // rows is available in registers for the epilogue without a separate pass over X (lora.py:108-112 fused).
    constexpr int LROWS = LORA ? 32 : 0;
    static_assert(2 * WM * (2048 * NI + (LORA ? 2048 * MI : 0)) + 4 * BN * 4 <= STAGES * (BM + BN + LROWS) * 128,
                  "epilogue patches + adapter exchange + column vectors must fit the operand stages");
    __shared__ __attribute__((aligned(16))) char smem[STAGES * (BM + BN + LROWS) * 128];
    char* sX = smem;                        // [STAGES][BM][128 B]
    char* sW = smem + STAGES * BM * 128;    // [STAGES][BN][128 B]
    char* sL = smem + STAGES * (BM + BN) * 128;   // [STAGES][32][128 B]

    // the last pf_blocks workgroups of the grid (slh_gemm_desc.pf_*); only in the ring tile's instantiations: slh_gemm gives the
    // hint to no other tile, and the 16 loads in flight per thread do not fit the 80-register budgets of the small tiles
    if constexpr (STAGES == 4 && WM == 4 && MI == 1 && NI == 2) {
        if (gemm_weight_touch(p)) return;
    }
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    int tile_m, tile_n, ks_id;
    int kt_begin = 0, nk = p.K / BK;
    {
        gemm_map_tile(p, tile_m, tile_n, ks_id);
        if (p.splitk > 1) {
            kt_begin = ks_id * p.kper;          // K tiles per slice: computed once, by slh_gemm, which also makes every slice non-empty
            nk = min(nk, kt_begin + p.kper) - kt_begin;
        }
    }
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    // ---- per-lane fill geometry --------------------------------------------------------------
    const int frow = lane >> 3;   // row within the 8-row group written by one glds instruction
    const int fslot = lane & 7;   // physical 16-B slot in the row
    const int cin = p.ca0 + p.ca1;

    long xrow_off0[XI];           // dense: element offset of the row in source 0 / 1
    long xrow_off1[XI];
    int xb[XI], xoy[XI], xox[XI]; // conv: sample / output pixel of the row
    int xks[XI];                  // logical k-slot this lane fetches (inverse swizzle)
#pragma unroll
    for (int i = 0; i < XI; ++i) {
        const int row = (wave + NW * i) * 8 + frow;
        int m = m0 + row;
        m = m < p.M ? m : p.M - 1;
        xks[i] = fslot ^ ((row >> 1) & 7);
        if (MODE == 0) {
            xrow_off0[i] = (long)m * p.lda0;
            xrow_off1[i] = (long)m * p.lda1;
        } else {
            const RowPixel px = pixel_of_row(m, p.ho, p.wo);
            xb[i] = px.b; xoy[i] = px.oy; xox[i] = px.ox;
        }
    }
    const __bf16* wptr[WI];
#pragma unroll
    for (int i = 0; i < WI; ++i) {
        const int row = (wave + NW * i) * 8 + frow;
        int n = n0 + row;
        n = n < p.N ? n : p.N - 1;
        wptr[i] = w_row_src(p, n, row, fslot);
    }
    const int wkstep = p.w_packed ? 4096 : BK;   // elements between consecutive K tiles of one W row group

    // 2-slot loop: compiler-visible LDS-DMA.  (Issued from inline asm like the deep ring, hipcc counts
    // lgkmcnt in front of the MFMAs instead of waiting lgkmcnt(0), but the pass time did not change in a same-box A/B, and the
    // compiler's own vmcnt(0) in front of the epilogue barriers, which scripts/check_lds_dma_waits.py relies on, goes away.)
    auto stage_copy = [&](const void* src, void* lds_dst) {
        glds16(src, lds_dst);
    };
    auto stage = [&](int buf, int kt) {
        const int k0 = kt * BK;
        char* dX = sX + buf * (BM * 128);
        char* dW = sW + buf * (BN * 128);
        if (MODE == 0) {
            const SrcSel s = src_select(p, k0);
#pragma unroll
            for (int i = 0; i < XI; ++i) {
                const __bf16* src = s.base + (s.second ? xrow_off1[i] : xrow_off0[i]) + s.cc + (xks[i] << 3);
                stage_copy(src, dX + (wave + NW * i) * 1024);
            }
        } else {
            const int tap = k0 / cin;
            const int c0 = k0 - tap * cin;
            const int ky = tap / 3, kx = tap - ky * 3;
            const SrcSel s = src_select(p, c0);
#pragma unroll
            for (int i = 0; i < XI; ++i) {
                const ConvTap t = conv_tap(p, xb[i], xoy[i], xox[i], ky, kx);
                const __bf16* src = t.ok ? s.base + t.pix * s.ld + s.cc + (xks[i] << 3)
                                         : (const __bf16*)slh_zero_page;
                stage_copy(src, dX + (wave + NW * i) * 1024);
            }
        }
#pragma unroll
        for (int i = 0; i < WI; ++i) {
            stage_copy(wptr[i] + (long)kt * wkstep, dW + (wave + NW * i) * 1024);
        }
        if (LORA) {
            const int row = (wave & 3) * 8 + frow;   // with 8 waves the upper four re-issue the same rows (benign)
            stage_copy(lora_down_src(p, row, k0, fslot), sL + buf * (32 * 128) + (wave & 3) * 1024);
        }
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    f32x16 accl[MI];   // LORA: accl[i][r'] = T[m = ...i*32 + lrow][rank index (r'&3) + 8*(r'>>2) + 4*lhi]
    if (LORA) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) accl[i][r] = 0.f;
    }
    const int lrow = lane & 31, lhi = lane >> 5;

    float ln_mean[MI], ln_rstd[MI];
    f32x2 ln_pairs[MI][LN_MAXC];
    const bool ln_on = MODE == 0 && !LORA && p.ln_in != nullptr;   // (never with a fused adapter: slh_gemm rejects it)
    if (MODE == 0 && ln_on) gemm_ln_request<MI>(p, m0 + wm * (32 * MI), lrow, ln_pairs);
    auto ln_finish = [&]() {
        if (MODE == 0 && ln_on) gemm_ln_finish<MI>(p, m0 + wm * (32 * MI), lrow, tile_n == 0 && wn == 0 && lhi == 0, ln_pairs, ln_mean, ln_rstd);
    };

    auto compute = [&](int buf) {
        const char* cX = sX + buf * (BM * 128);
        const char* cW = sW + buf * (BN * 128);
        // fragments are double-buffered in registers: the ds_read_b128 of k-step ks+1 are issued before the MFMAs
        // of k-step ks, so LDS latency hides under the matrix pipe instead of being exposed 4x per K tile
        const char* cL = sL + buf * (32 * 128);
        bf16x8 xf[2][MI], wf[2][NI], lf[2];
        auto load_frags = [&](int set, int ks) {
            if (LORA && (ks & 1) == wn) lf[set] = *(const bf16x8*)(cL + lds_off(lrow, ks * 2 + lhi));
#pragma unroll
            for (int i = 0; i < MI; ++i)
                xf[set][i] = *(const bf16x8*)(cX + lds_off(wm * (32 * MI) + i * 32 + lrow, ks * 2 + lhi));
#pragma unroll
            for (int j = 0; j < NI; ++j)
                wf[set][j] = *(const bf16x8*)(cW + lds_off(wn * (32 * NI) + j * 32 + lrow, ks * 2 + lhi));
        };
        load_frags(0, 0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (ks < 3) load_frags((ks + 1) & 1, ks + 1);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[ks & 1][j], xf[ks & 1][i], acc[i][j], 0, 0, 0);
            if (LORA && (ks & 1) == wn) {     // the two waves that share these rows split the adapter's K steps (see epilogue)
#pragma unroll
                for (int i = 0; i < MI; ++i)
                    accl[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lf[ks & 1], xf[ks & 1][i], accl[i], 0, 0, 0);
            }
        }
    };

    if constexpr (STAGES == 2) {
        stage(0, kt_begin);
        ln_finish();
        for (int kt = 0; kt < nk; ++kt) {
            lds_dma_syncthreads();  // drains this wave's glds (explicit vmcnt(0)) and orders all waves
            if (kt + 1 < nk) stage((kt + 1) & 1, kt_begin + kt + 1);
            compute(kt & 1);
        }
    } else {
        // ---- deep LDS ring (STAGES = 3 or 4 slots), for launches that leave ONE workgroup per CU -----------------
        // A CU with a single resident workgroup hides nothing behind other workgroups: with the 2-slot loop above
        // every K tile pays a full L2/HBM round trip (measured: fill alone = 1340 clk per 32 KB tile, i.e. 24 B/clk
        // of the 64 B/clk the CU can pull) and the first ds_read latency of each tile.  Here
        //   * S-2 whole K tiles are kept in flight (LDS-DMA outstanding across barriers, counted vmcnt),
        //   * the MFMA fragments are software-pipelined across k-steps AND across K tiles (the fragments of step
        //     ks+1 - or of the next tile's step 0 - are requested before the MFMAs of step ks issue),
        //   * ONE raw s_barrier per K tile sits in the middle of the tile (after k-step 1).
        // Protocol for K tile g (slot g % S), all counts per wave:
        //   ks0, ks1 : MFMAs of (g,0), (g,1); fragment reads of (g,1), (g,2)
        //   sync     : s_waitcnt vmcnt((S-3)*L) -> this wave's share of tile g+1 has landed (tiles g+2.. stay in
        //              flight); s_barrier -> every wave's share has, and every wave is past its last read of tile g-1
        //   ks2, ks3 : MFMAs of (g,2), (g,3); fragment reads of (g,3), (g+1,0); LDS-DMA of tile g+S-1 into the slot
        //              tile g-1 occupied, half of the pieces behind each k-step's reads
        // The source pointers of the L pieces are running pointers (advanced once per K tile; re-based when the
        // implicit GEMM moves to the next filter tap or the second concat source), so a piece costs one 64-bit add.
        constexpr int S = STAGES;
        constexpr int L = XI + WI + (LORA ? 1 : 0);   // LDS-DMA instructions per wave per K tile
        constexpr int H0 = (L + 1) / 2;               // pieces issued behind k-step 2 (the rest behind k-step 3)
        const char* xsrc[XI];
        int xadv[XI];
        const char* wsrc[WI];
        const char* lsrc = nullptr;
        int ladv = 0;
#pragma unroll
        for (int i = 0; i < WI; ++i) wsrc[i] = (const char*)(wptr[i] + (long)kt_begin * wkstep);
        if (LORA) {
            const int row = (wave & 3) * 8 + frow;
            lsrc = (const char*)lora_down_src(p, row, kt_begin * BK, fslot);
            ladv = row < p.lora_rank ? 128 : 0;
        }
        // K tile the next issue belongs to (relative to this workgroup's K slice); its channel offset / filter tap
        int i_kt = 0, i_c0 = kt_begin * BK, i_tap = 0;
        if (MODE == 1) { i_tap = i_c0 / cin; i_c0 -= i_tap * cin; }
        bool i_first = true;
        const unsigned lds0 = lds_addr_of(smem);
        const int wkbytes = wkstep * 2;

        // (re)base the X pointers of the tile at (i_tap, i_c0); called when a tap or a concat source begins
        auto rebase_x = [&]() {
            const SrcSel s = src_select(p, i_c0);
            if (MODE == 0) {
#pragma unroll
                for (int i = 0; i < XI; ++i) {
                    xsrc[i] = (const char*)(s.base + (s.second ? xrow_off1[i] : xrow_off0[i]) + s.cc + (xks[i] << 3));
                    xadv[i] = 128;
                }
            } else {
                const int ky = i_tap / 3, kx = i_tap - ky * 3;
#pragma unroll
                for (int i = 0; i < XI; ++i) {
                    const ConvTap t = conv_tap(p, xb[i], xoy[i], xox[i], ky, kx);
                    xsrc[i] = t.ok ? (const char*)(s.base + t.pix * s.ld + s.cc + (xks[i] << 3)) : (const char*)slh_zero_page;
                    xadv[i] = t.ok ? 128 : 0;
                }
            }
        };
        // LDS-DMA piece j (order: X, W, LoRA) of K tile i_kt into ring slot `slot`
        auto piece = [&](const int j, const int slot) {
            if (j < XI) {
                glds16_hidden(xsrc[j], lds0 + slot * (BM * 128) + (wave + NW * j) * 1024);
                xsrc[j] += xadv[j];
            } else if (j < XI + WI) {
                const int i = j - XI;
                glds16_hidden(wsrc[i], lds0 + STAGES * BM * 128 + slot * (BN * 128) + (wave + NW * i) * 1024);
                wsrc[i] += wkbytes;
            } else {
                glds16_hidden(lsrc, lds0 + STAGES * (BM + BN) * 128 + slot * (32 * 128) + (wave & 3) * 1024);
                lsrc += ladv;
            }
        };
        auto tile_begin = [&]() {
            if (i_first || i_c0 == 0 || i_c0 == p.ca0) rebase_x();
            i_first = false;
        };
        auto tile_end = [&]() {
            ++i_kt;
            i_c0 += BK;
            if (MODE == 1 && i_c0 == cin) { i_c0 = 0; ++i_tap; }
        };
        auto issue_all = [&](const int slot) {
            tile_begin();
#pragma unroll
            for (int j = 0; j < L; ++j) piece(j, slot);
            tile_end();
        };

        bf16x8 xf[2][MI], wf[2][NI], lf[2];
        auto load_frags = [&](const int set, const int slot, const int ks) {
            const char* cX = sX + slot * (BM * 128);
            const char* cW = sW + slot * (BN * 128);
            if (LORA && set == wn) lf[set] = *(const bf16x8*)(sL + slot * (32 * 128) + lds_off(lrow, ks * 2 + lhi));   // set == ks & 1
#pragma unroll
            for (int i = 0; i < MI; ++i)
                xf[set][i] = *(const bf16x8*)(cX + lds_off(wm * (32 * MI) + i * 32 + lrow, ks * 2 + lhi));
#pragma unroll
            for (int j = 0; j < NI; ++j)
                wf[set][j] = *(const bf16x8*)(cW + lds_off(wn * (32 * NI) + j * 32 + lrow, ks * 2 + lhi));
        };
        // the MFMAs of one k-step; with ISSUE, the LDS-DMA pieces [p0, p1) of the tile being staged are dealt out behind
        // them one at a time, so each piece's ~7 scalar/vector instructions issue in the shadow of a 32-cycle MFMA
        constexpr int NMF = MI * NI + (LORA ? MI : 0);
        auto mfmas = [&](const int set, const bool with_pieces, const int p0, const int p1, const int slot) {
            const int per = with_pieces ? (p1 - p0 + NMF - 1) / NMF : 0;
            int m = 0;
#pragma unroll
            for (int i = 0; i < MI; ++i) {
#pragma unroll
                for (int j = 0; j < NI + (LORA ? 1 : 0); ++j) {
                    if (j < NI) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[set][j], xf[set][i], acc[i][j], 0, 0, 0);
                    else if (set == wn) accl[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lf[set], xf[set][i], accl[i], 0, 0, 0);
                    if (with_pieces) {
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int q = 0; q < per; ++q)
                            if (p0 + m * per + q < p1) piece(p0 + m * per + q, slot);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    ++m;
                }
            }
        };

        // prologue: tiles 0 .. S-2 in flight, tile 0 landed, its first fragments requested
        for (int t = 0; t < S - 1; ++t) {
            if (t < nk) issue_all(t);
        }
        ln_finish();
        if (nk >= S - 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((S - 2) * L) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        load_frags(0, 0, 0);
        __builtin_amdgcn_s_waitcnt(0xC07F);            // lgkmcnt(0): nothing pending when the loop is entered
        int cur = 0;
        // one K tile; MORE: a next tile exists, ISSUE: tile g+S-1 exists, KEEP: tile g+2 exists (its LDS-DMA may stay in
        // flight across the barrier).  The flags are compile-time so that the steady-state body is straight-line code:
        // hipcc's waitcnt insertion falls back to lgkmcnt(0) at control-flow joins, which would expose the latency of
        // the fragment reads it was asked to keep in flight.
        auto body = [&](auto more_c, auto issue_c, auto keep_c) {
            constexpr bool MORE = decltype(more_c)::value, ISSUE = decltype(issue_c)::value, KEEP = decltype(keep_c)::value;
            const int nxt = cur == S - 1 ? 0 : cur + 1;
            const int prv = cur == 0 ? S - 1 : cur - 1;
            __builtin_amdgcn_sched_barrier(0);
            load_frags(1, cur, 1);
            __builtin_amdgcn_sched_barrier(0);
            mfmas(0, false, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            load_frags(0, cur, 2);
            __builtin_amdgcn_sched_barrier(0);
            mfmas(1, false, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (MORE) {
                if constexpr (S >= 4 && KEEP) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((S - 3) * L) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
            }
            __builtin_amdgcn_sched_barrier(0);
            load_frags(1, cur, 3);
            if constexpr (ISSUE) tile_begin();
            __builtin_amdgcn_sched_barrier(0);
            mfmas(0, ISSUE, 0, H0, prv);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (MORE) load_frags(0, nxt, 0);
            __builtin_amdgcn_sched_barrier(0);
            mfmas(1, ISSUE, H0, L, prv);
            if constexpr (ISSUE) tile_end();
            __builtin_amdgcn_sched_barrier(0);
            // the fragments requested before the last four MFMAs have landed long before those MFMAs have issued; saying
            // so here leaves nothing pending across the loop edge (where the compiler would otherwise wait lgkmcnt(0)
            // AFTER the next k-step's reads have been issued)
            __builtin_amdgcn_s_waitcnt(0xC07F);
            cur = nxt;
        };
        using T_ = std::true_type;
        using F_ = std::false_type;
        int g = 0;
        for (; g + S - 1 < nk; ++g) body(T_{}, T_{}, T_{});
        if constexpr (S >= 4) {
            if (g + 2 < nk) { body(T_{}, F_{}, T_{}); ++g; }
        }
        if (g + 1 < nk) { body(T_{}, F_{}, F_{}); ++g; }
        if (g < nk) body(F_{}, F_{}, F_{});
    }

    // XA: the instantiation that carries the fused cross-attention (FEAT bit 8, gemm_common.h)
    gemm_epilogue<MI, NI, MODE, LORA, NW, 2, XA ? 15 : 7>(p, smem, acc, accl, ln_mean, ln_rstd, ln_on, tile_m, tile_n, ks_id, wave, wm, wn);
}

template <int MI, int NI, int MODE, bool LORA, int WM>
int launch_gemm3(const GemmArgs& a, int stages, hipStream_t s) {
    const int grid = a.tiles_m * a.tiles_n * (a.splitk > 1 ? a.splitk : 1) + a.pf_blocks;
    constexpr int stage_bytes = (32 * MI * WM + 64 * NI + (LORA ? 32 : 0)) * 128;
    constexpr bool can3 = 3 * stage_bytes <= 160 * 1024;
    constexpr bool can4 = 4 * stage_bytes <= 160 * 1024;
#define SLH_LAUNCH_RING(ST_)                                                                                                  \
    slh_launch<gemm_kernel<MI, NI, MODE, ST_, LORA, WM>>(grid, 128 * WM, s, a, "gemm_kernel<%d, %d, %d, %d, %s, %d, false>", MI, NI, \
                                                         MODE, (int)(ST_), slh_tf(LORA), WM)
    if (stages == 4 && !can4) stages = 3;          // the deepest ring that fits the 160 KB of LDS
    if (stages == 3 && !can3) stages = 2;
    if (stages == 4)
        SLH_LAUNCH_RING((can4 ? 4 : 2));
    else if (stages == 3)
        SLH_LAUNCH_RING((can3 ? 3 : 2));
    else
        SLH_LAUNCH_RING(2);
#undef SLH_LAUNCH_RING
    SLH_LAUNCH_CHECK("slh_gemm");
    return 0;
}

// query projection + cross-attention (slh_gemm_desc.xa_k): the 128 x 128 8-wave ring tile (256 registers per lane to work with;
// the double-buffered loop's 128 would spill the scores)
int launch_gemm_xa(const GemmArgs& a, hipStream_t s) {
    const int grid = a.tiles_m * a.tiles_n + a.pf_blocks;
    slh_launch<gemm_kernel<1, 2, 0, 4, false, 4, true>>(grid, 512, s, a, "gemm_kernel<1, 2, 0, 4, false, 4, true>");
    SLH_LAUNCH_CHECK("slh_gemm (query projection + cross-attention)");
    return 0;
}

template <int MI, int NI, int WM>
int launch_gemm(const GemmArgs& a, int mode, int stages, hipStream_t s) {
    const bool lora = a.lora_down != nullptr;
    if (mode == 0) return lora ? launch_gemm3<MI, NI, 0, true, WM>(a, stages, s) : launch_gemm3<MI, NI, 0, false, WM>(a, stages, s);
    return lora ? launch_gemm3<MI, NI, 1, true, WM>(a, stages, s) : launch_gemm3<MI, NI, 1, false, WM>(a, stages, s);
}

}  // namespace

// CUs behind the weight touch; a query (slh_gemm_launch_query) answers for the MI355X's 256 on any machine
static int slh_ncu() {
    if (slh_name_mode()) return 256;
    static const int ncu = [] {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
        return prop.multiProcessorCount;
    }();
    return ncu;
}

// The tile d names - explicit (set by the planner from the tuned table) or, for an all-zero code, a fill-the-chip heuristic - or the
// refusal of a code that names no kernel: every nibble of bits 0-15 is either read by the dispatch or must be zero.
int gemm_tile_decode(const slh_gemm_desc* d, GemmTile* t) {
    const int tile = d->tile, fam = (tile >> 12) & 15, st = (tile >> 8) & 15, hi = (tile >> 4) & 15, lo = tile & 15;
    SLH_CHECK((tile >> 20) == 0, "slh_gemm: tile 0x%x uses reserved bits (20 and up must be zero)", tile);
    t->splitk = (tile >> 16) & 15;
    t->slots = st; t->mi = hi; t->ni = lo; t->wm = 0;
    if ((tile & 0xffff) == 0) {
        // untuned shape: the pattern of the measured table (sliders_amd/tuning/gfx950_sdxl_128.json) - the 8-wave 128x128
        // tile once it yields enough workgroups (or fewer, but with a long K loop to amortise them), 64x64 otherwise
        const long t128 = (long)((d->M + 127) / 128) * ((d->N + 127) / 128);
        t->family = GEMM_RING;
        t->mi = 1;
        if (d->geglu == 1) {
            t->ni = 2; t->wm = t128 >= 192 ? 4 : 2;
        } else if (t128 >= 256 || (t128 >= 160 && d->K >= 5760)) {
            t->ni = 2; t->wm = 4;
        } else {
            t->ni = 1; t->wm = 2;
        }
    } else if (fam == 5) {                                      // gemm5.hip: 4 waves of 32 x 80
        SLH_CHECK((tile & 0xfff) == 0x425 || (tile & 0xfff) == 0x525,
                  "slh_gemm: the 64 x 160 tile is 0x5425 (4 ring slots) or 0x5525 (5 ring slots), not 0x%x", tile & 0xffff);
        t->family = GEMM_64X160;
        t->bm = 64; t->bn = 160; t->threads = 256;
        return 0;
    } else if (fam == 7) {                                      // gemm7.hip: 0x7<S><XB><WB>
        // (a 128 x 320 four-wave instantiation, 0x754a, was measured and removed: it lost to the ping-pong tile in the pass and is
        // superseded by the 256 x 320 tile - profiles/r06_gemm7_insitu_ab.txt, r06_tile_256x320.txt)
        SLH_CHECK((tile & 0xfff) == 0x648 || (tile & 0xfff) == 0x645 || (tile & 0xfff) == 0x48a,
                  "slh_gemm: the tiles of gemm7.hip are 0x7648 (128 x 256), 0x7645 (128 x 160) and 0x748a (256 x 320), not 0x%x", tile & 0xffff);
        t->family = GEMM_FOURWAVE;
        t->bm = 32 * hi; t->bn = 32 * lo; t->threads = 512;
        return 0;
    } else {
        SLH_CHECK(fam == 0 || fam == 2 || fam == 4 || fam == 8,
                  "slh_gemm: tile 0x%x: bits 12-15 are 0 | 2 (4 waves), 4 (8 waves), 8 (ping-pong), 5 (64 x 160) or 7 (gemm7.hip)", tile);
        SLH_CHECK(hi != 0, "slh_gemm: tile 0x%x names no block tile (MI = 0): bits 0-15 are all zero (heuristic) or a complete tile code", tile);
        if (fam == 8) {                                         // gemm8p.hip: one 8-wave workgroup per CU
            SLH_CHECK(st == 0, "slh_gemm: tile 0x%x: bits 8-11 of a ping-pong tile (0x8042, 0x801<NI>) must be zero", tile);
            SLH_CHECK((hi == 4 && lo == 2) || (hi == 1 && lo >= 3 && lo <= 5),
                      "slh_gemm: tile 0x%x: ping-pong tiles are 256 x 256 (0x8042) or 128 x 64*NI (0x801<NI>, NI = 3..5)", tile);
            t->family = GEMM_PINGPONG; t->wm = 8;
            t->bm = hi == 1 ? 128 : 256; t->bn = hi == 1 ? 64 * lo : 256; t->threads = 512;
            return 0;
        }
        SLH_CHECK(st == 0 || st == 2 || st == 3 || st == 4, "slh_gemm: tile 0x%x: bits 8-11 (ring slots) are 0 | 2 (double buffer), 3 or 4", tile);
        t->family = GEMM_RING; t->wm = fam == 4 ? 4 : 2;
        SLH_CHECK((hi == 1 || hi == 2) && (lo == 1 || lo == 2), "slh_gemm: bad tile 0x%x: MI and NI are 1 or 2", tile);
        SLH_CHECK(t->wm == 2 || lo == 2 || hi == 1, "slh_gemm: tile 0x%x: 8-wave tiles are 128x64, 128x128 or 256x128", tile);
    }
    t->bm = 32 * t->mi * t->wm; t->bn = 64 * t->ni; t->threads = 128 * t->wm;
    return 0;
}

// L2 blocking: number of m-tile groups G (see the kernel's tile mapping).  An XCD's chunk of the grouped sequence reads
// its groups' X rows once if a group fits the L2 budget, and sweeps W once per group it touches, so the fabric
// traffic is about  X * max(1, 8/G) + G * W ; pick the power of two that minimises it.
static int pick_group_m(const slh_gemm_desc* d, int tiles_m) {
    static const char* env = getenv("SLIDERS_GEMM_GROUPS");   // measurement aid: force G (1 = ungrouped order)
    if (tiles_m <= 1) return 1;
    int G = 1;
    if (env && atoi(env) > 0) {
        G = atoi(env);
    } else {
        const int cin = d->ca0 + d->ca1;
        double xb = 2.0 * d->M * cin;
        if (d->mode == 1) xb = 2.0 * d->batch * d->hs * d->ws * cin;     // unique source pixels of the implicit GEMM
        const double wb = 2.0 * d->N * d->K;
        const double budget = 2.75e6;                                    // of the 4 MB L2: the rest holds W panels + C
        double best = -1.0;
        for (int g = 1; g <= tiles_m; g *= 2) {
            if (xb / g > budget && 2 * g <= tiles_m) continue;
            const double cost = xb * (g < 8 ? 8.0 / g : 1.0) + g * wb;
            if (best < 0.0 || cost < best) { best = cost; G = g; }
        }
    }
    if (G > tiles_m) G = tiles_m;
    return (tiles_m + G - 1) / G;
}

// gemm5.hip / gemm7.hip: an XCD's run of tiles_m * tiles_n / 8 tiles is gm row tiles x (run / gm) column tiles; pick the gm (power
// of two) that minimises the operand rows it pulls through its L2 (bm * gm of X + bn * run / gm of W)
int gemm_group_m(int tiles_m, int tiles_n, int bm, int bn) {
    const int run = (tiles_m * tiles_n + 7) / 8;
    int best = 1;
    long best_cost = -1;
    for (int gm = 1; gm <= tiles_m; gm *= 2) {
        const int gn = (run + gm - 1) / gm;
        const long cost = (long)bm * gm + (long)bn * (gn < tiles_n ? gn : tiles_n);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = gm; }
    }
    return best;
}

// the name of the kernel instantiation slh_gemm would launch for d, as rocprofv3 prints it ("gemm8pb_kernel<1, 5, 0, false>"): the
// whole of slh_gemm runs - descriptor checks, tile choice, ring-depth fallback - with the launch itself replaced by a record of the
// selected template (common.h: slh_launch).  No device needed, nothing launched.  0 / the descriptor's error.
extern "C" int slh_gemm_kernel_name(const slh_gemm_desc* d, char* buf, int cap) {
    SLH_CHECK(buf && cap >= 16, "slh_gemm_kernel_name: buffer");
    slh_name_sink_set(buf, cap);
    const int rc = slh_gemm(d, nullptr);
    slh_name_sink_set(nullptr, 0);
    if (rc == 0 && !buf[0]) { slh_set_error("slh_gemm_kernel_name: internal: no launch site recorded a name"); return -3; }
    return rc;
}

// slh_gemm_kernel_name plus the launch itself: grid, block size and the FNV-1a hash of the argument struct the kernel would receive
extern "C" int slh_gemm_launch_query(const slh_gemm_desc* d, char* name, int cap, int32_t* grid, int32_t* block, uint64_t* args_hash) {
    SLH_CHECK(grid && block && args_hash, "slh_gemm_launch_query: null pointer");
    const int rc = slh_gemm_kernel_name(d, name, cap);
    if (rc) return rc;
    int g, b;
    unsigned long long h;
    slh_launch_recorded(&g, &b, &h);
    *grid = g; *block = b; *args_hash = h;
    return 0;
}

// K slices a launch of d runs (1: no split-K): the tile's factor, cut so that every slice is non-empty - each publishes its whole
// partial tile, the last one to arrive reads them all; per = K tiles per slice
static int gemm_splitk(const slh_gemm_desc* d, const GemmTile& t, int& per) {
    const int nk = d->K / 64, s = t.splitk;
    per = nk;
    if (s <= 1) return 1;
    per = (nk + s - 1) / s;
    return (nk + per - 1) / per;
}

// vt_out: the columns from vt_col0 on leave head-transposed; whole heads, whole col_align-column blocks and token_align-row blocks
int gemm_check_vt(const slh_gemm_desc* d, const GemmTile& t, int col_align, int token_align) {
    GEMM_CHECK(d->vt_D > 0 && d->vt_D % 64 == 0 && d->vt_col0 % col_align == 0 && d->vt_col0 < d->N && d->vt_heads > 0 &&
                   (d->N - d->vt_col0) == d->vt_heads * d->vt_D && d->vt_tokens > 0 && d->vt_tokens % token_align == 0 &&
                   d->M % d->vt_tokens == 0 && d->vt_ld % 8 == 0 && d->vt_ld == d->vt_tokens && !d->geglu && ((uintptr_t)d->vt_out & 15) == 0,
               "vt_out constraints (vt_D %% 64, vt_col0 %% %d, vt_tokens %% %d, M %% vt_tokens, vt_ld == vt_tokens: the padding columns "
               "slh_transpose_heads zero-fills are not written here, so there must be none; 16-byte aligned; no GEGLU)", col_align, token_align);
    return 0;
}

// What the 64 x 160 tile and the tiles of gemm7.hip both are: whole tiles of a dense single-source product with packed weights, results
// stored in 16-byte row segments, operands read in aligned quads; an adapter only fused in, in the forward form
int gemm_check_whole_tiles(const slh_gemm_desc* d, const GemmTile& t, int w_align) {
    GEMM_CHECK(d->mode == 0 && !d->a1 && !d->ca1 && d->w_layout == 1, "this tile runs dense single-source products with packed weights (w_layout = 1) only");
    GEMM_CHECK(d->M % t.bm == 0 && d->N % t.bn == 0, "this tile needs M %% %d == 0 and N %% %d == 0 (M=%d N=%d)", t.bm, t.bn, d->M, d->N);
    GEMM_CHECK(!d->lora_t && !d->rowbias && !d->xa_k && !d->geglu_pre && d->geglu != 1 && d->geglu != 2,
               "this tile takes no row bias, external T, geglu = 1 / 2, geglu_pre or cross-attention");
    GEMM_CHECK(d->ldc % 8 == 0 && ((uintptr_t)d->c & 15) == 0 && ((uintptr_t)d->a0 & 15) == 0 && ((uintptr_t)d->w & (w_align - 1)) == 0 &&
                   ((uintptr_t)d->residual & 7) == 0 && ((uintptr_t)d->bias & 7) == 0,
               "this tile needs ldc %% 8 == 0, 16-byte aligned a0 / c, %d-byte aligned w, 8-byte aligned bias / residual", w_align);
    if (d->lora_down)
        GEMM_CHECK(!d->lora_up_rmajor && ((uintptr_t)d->lora_down & 15) == 0 && ((uintptr_t)d->lora_up & 7) == 0 && ((uintptr_t)d->lora_t_out & 15) == 0,
                   "this tile takes a fused adapter in the forward form only; 16-byte aligned lora_down / lora_t_out, 8-byte aligned lora_up");
    else
        GEMM_CHECK(!d->lora_t_out, "lora_t_out without lora_down");
    return 0;
}

// gemm.hip / gemm8p.hip: every option exists; which tiles take which
static int gemm_ring_check(const slh_gemm_desc* d, const GemmTile& t) {
    const bool pp = t.family == GEMM_PINGPONG;
    GEMM_CHECK(d->w_layout == 0 || d->w_layout == 1, "bad w_layout");
    GEMM_CHECK(!pp || !d->lora_down || t.mi == 1, "the 256 x 256 tile does not take a fused adapter (lora_down)");
    GEMM_CHECK(!pp || !d->vt_out || t.mi == 4 || (t.ni == 4 && d->mode == 0),
               "vt_out on the ping-pong tiles needs 256 x 256 (0x8042) or the dense 128 x 256 tile (0x8014)");
    GEMM_CHECK(!pp || d->geglu != 2 || t.mi == 4, "the 128 x 64*NI ping-pong tiles have no GEGLU backward epilogue (geglu = 2)");
    GEMM_CHECK(d->geglu != 1 || t.ni == 2, "geglu needs NI=2");
    GEMM_CHECK(!d->ln_out || (t.ni == 2 && d->N % 64 == 0 && !d->vt_out), "ln_out needs a 128-column tile (NI = 2), N %% 64 == 0, no vt_out");
    GEMM_CHECK(!(d->ln_in && d->lora_down) ||
                   (pp && t.mi == 1 && t.ni <= 4 && !d->lora_up_rmajor && !d->lora_t_out && !d->ln_mr_out && t.splitk <= 1),
               "ln_in with a fused adapter runs on the ping-pong 128 x 192 / 128 x 256 tiles (0x8013, 0x8014); forward form, no split-K");
    return d->vt_out ? gemm_check_vt(d, t, 128, 8) : 0;
}

// Every check of slh_gemm except what the caller provisions once the tile is chosen (the split-K slab / ticket workspace and its slab
// count, ln_lora_s / ln_lora_c): 0 and the decoded tile, or the status slh_gemm returns for d with slh_last_error saying why.
// Each contract stands here once; a family's own part says which options it has and on which tiles.
static int gemm_check(const slh_gemm_desc* d, GemmTile& t) {
    // ---- the product
    SLH_CHECK(d && d->a0 && d->w && d->c, "slh_gemm: null pointer");
    SLH_CHECK(d->M > 0 && d->N > 0 && d->K > 0, "slh_gemm: bad shape M=%d N=%d K=%d", d->M, d->N, d->K);
    SLH_CHECK(d->K % 64 == 0, "slh_gemm: K=%d must be a multiple of 64", d->K);
    SLH_CHECK(d->N % 4 == 0, "slh_gemm: N=%d must be a multiple of 4", d->N);
    SLH_CHECK(d->ca0 % 64 == 0 && d->ca1 % 64 == 0, "slh_gemm: channel counts must be multiples of 64");
    SLH_CHECK((d->a1 != nullptr) == (d->ca1 > 0), "slh_gemm: a1/ca1 mismatch");
    SLH_CHECK(d->lda0 % 8 == 0 && d->lda1 % 8 == 0 && d->ldw % 8 == 0 && d->ldc % 4 == 0,
              "slh_gemm: leading dimensions must keep 16-byte loads / 8-byte stores aligned");
    SLH_CHECK(wt_span_ok(d->M, d->ldc, d->geglu == 2 ? 2 * d->N : d->geglu ? d->N / 2 : d->N),
              "slh_gemm: the result tensor (M=%d rows of ldc=%d) reaches past 2 GiB from its base: the write-through row stores address it "
              "with 32-bit offsets - split the batch", d->M, d->ldc);
    const int cin = d->ca0 + d->ca1;
    if (d->mode == 0) {
        SLH_CHECK(cin == d->K, "slh_gemm: dense K=%d != ca0+ca1=%d", d->K, cin);
    } else {
        SLH_CHECK(d->mode == 1, "slh_gemm: bad mode %d", d->mode);
        SLH_CHECK(d->K == 9 * cin, "slh_gemm: conv K=%d != 9*Cin=%d", d->K, 9 * cin);
        SLH_CHECK(d->stride == 1 || d->stride == 2, "slh_gemm: bad stride");
        SLH_CHECK(d->src_xform >= 0 && d->src_xform <= 2, "slh_gemm: bad src_xform");
        SLH_CHECK(d->M == d->batch * d->ho * d->wo, "slh_gemm: conv M mismatch");
    }
    SLH_CHECK(d->geglu >= 0 && d->geglu <= 3, "slh_gemm: geglu is 0, 1 / 3 (forward epilogue, 32 | 32 or 16 | 16 weight blocks) or 2 (backward form)");
    // ---- the tile, and its family's part
    if (gemm_tile_decode(d, &t)) return -1;
    const int rc = t.family == GEMM_FOURWAVE ? gemm7_check(d, t) : t.family == GEMM_64X160 ? gemm5_check(d, t) : gemm_ring_check(d, t);
    if (rc) return rc;
    // ---- adapters
    if (d->lora_down) {
        GEMM_CHECK(!d->lora_t && d->lora_up && d->lora_scale && !d->geglu, "fused lora_down excludes an external T / geglu");
        if (d->lora_up_rmajor) {
            // backward-data form: lora_down = the k-major copy of the up matrices ([rank][K], block-diagonal over a fused
            // q|k|v group), lora_up = the down matrices as stored ([rank][N]); U = dY . B leaves through lora_t_out
            GEMM_CHECK(d->lora_groups == 1 && (d->lora_rank == 4 || d->lora_rank == 8 || d->lora_rank == 12),
                       "fused r-major lora needs groups = 1, rank in {4, 8, 12}");
        } else {
            GEMM_CHECK(d->lora_groups >= 1 && d->lora_groups <= 3 && d->lora_rank == 4 * d->lora_groups &&
                           d->N % d->lora_groups == 0 && (d->N / d->lora_groups) % 4 == 0,
                       "fused lora needs rank = 4 * groups");
        }
        if (d->lora_t_out) GEMM_CHECK(d->ld_t >= d->lora_rank && d->ld_t % 4 == 0, "ld_t for lora_t_out");
    }
    if (d->lora_t) {
        GEMM_CHECK(d->lora_up && d->lora_scale, "lora pointers");
        GEMM_CHECK(d->lora_groups >= 1 && d->lora_groups <= 3 && d->N % d->lora_groups == 0 &&
                       d->ld_t >= 4 * d->lora_groups && d->ld_t % 4 == 0,
                   "bad lora grouping");
        if (d->lora_up_rmajor)
            GEMM_CHECK(d->lora_groups == 1 && (d->lora_rank == 4 || d->lora_rank == 8 || d->lora_rank == 12) &&
                           d->ld_t >= d->lora_rank,
                       "r-major lora_up needs groups=1 and rank in {4,8,12}");
        GEMM_CHECK((d->N / d->lora_groups) % 4 == 0, "lora group width");
    }
    // ---- epilogue options
    if (d->rowbias) GEMM_CHECK(d->rows_per_sample > 0 && d->ld_rowbias % 4 == 0, "rowbias");
    if (d->residual) GEMM_CHECK(d->ld_res % 4 == 0, "ld_res");
    if (d->geglu == 1) GEMM_CHECK(d->N % 64 == 0 && !d->lora_t && !d->residual && !d->rowbias, "geglu constraints");
    if (d->geglu == 3)
        GEMM_CHECK(d->N % 32 == 0 && !d->lora_t && !d->lora_down && !d->residual && !d->rowbias && !d->geglu_pre && !d->vt_out && !d->ln_out,
                   "geglu = 3 (16 | 16 weight blocks) needs N %% 32 == 0 and excludes adapters, residual, row bias, geglu_pre, vt_out, ln_out");
    GEMM_CHECK(!d->geglu_pre || (d->geglu && d->ld_pre >= (d->geglu == 2 ? 2 * d->N : d->N) && d->ld_pre % 4 == 0 &&
                                 ((uintptr_t)d->geglu_pre & 7) == 0),
               "geglu_pre needs the GEGLU epilogue, ld_pre >= N (2N in the backward form), 8-byte alignment");
    if (d->geglu == 2)
        GEMM_CHECK(d->geglu_pre && d->N % 32 == 0 && d->ldc >= 2 * d->N && d->ldc % 4 == 0 && !d->bias && !d->rowbias && !d->residual &&
                       !d->lora_t && !d->lora_down && !d->vt_out && !d->ln_in && !d->ln_out,
                   "geglu = 2 (backward form) needs geglu_pre, N %% 32 == 0, ldc >= 2N and a bare product");
    GEMM_CHECK(!d->vt_also_c || d->vt_out, "vt_also_c without vt_out");
    // ---- LayerNorm fold: producer side, consumer side
    if (d->ln_out) GEMM_CHECK(!d->geglu && ((uintptr_t)d->ln_out & 7) == 0, "ln_out needs 8-byte alignment and no GEGLU");
    if (d->ln_in) {
        GEMM_CHECK(d->mode == 0 && !d->a1 && d->ln_s && d->ln_b && !d->bias && !d->lora_t,
                   "ln_in needs a dense single-source product, ln_s / ln_b, no bias (folded into ln_b), no external T");
        GEMM_CHECK(d->ln_in_chunks >= 1 && d->ln_in_chunks <= 20 && (d->K == 64 * d->ln_in_chunks || d->K == 80 * d->ln_in_chunks),
                   "ln_in_chunks must be K / 64 (producer on a 64 / 128-column tile) or K / 80 (producer on the 64 x 160 tile), <= 20");
        GEMM_CHECK(((uintptr_t)d->ln_in & 7) == 0 && ((uintptr_t)d->ln_s & 15) == 0 && ((uintptr_t)d->ln_b & 15) == 0,
                   "ln_in / ln_s / ln_b alignment");
    }
    GEMM_CHECK(!d->ln_mr_out || d->ln_in, "ln_mr_out without ln_in");
    // ---- split-K
    int per;
    const int splitk = gemm_splitk(d, t, per);
    if (splitk > 1) {
        GEMM_CHECK((long)splitk * ((d->M + 255) / 256 * 256L) * ((d->N + 255) / 256 * 256L) * 4 < (1L << 31), "split-K slabs beyond 2 GB");
        // the slab workspace is sized by contract (include/sliders_hip.h: roundup(M, 256) x roundup(N, 128) floats per slice)
        GEMM_CHECK((long)((d->M + t.bm - 1) / t.bm) * t.bm * ((d->N + t.bn - 1) / t.bn) * t.bn <= ((d->M + 255) / 256 * 256L) * ((d->N + 127) / 128 * 128L),
                   "split-K slabs of %d x %d tiles exceed the workspace contract for M=%d N=%d", t.bm, t.bn, d->M, d->N);
    }
    // ---- cross-attention behind the query projection
    if (d->xa_k) {
        GEMM_CHECK(t.family == GEMM_RING && t.wm == 4 && t.mi == 1 && t.ni == 2 && t.slots == 4 && splitk == 1,
                   "the fused cross-attention runs on the 128 x 128 8-wave ring tile (0x4412), no split-K");
        GEMM_CHECK(d->mode == 0 && !d->lora_down && !d->lora_t && !d->residual && !d->rowbias && !d->geglu && !d->ln_out && !d->vt_out,
                   "xa_k excludes adapters, residual, row bias, GEGLU, ln_out, vt_out");
        GEMM_CHECK(d->xa_vt && d->N % 64 == 0 && d->xa_tk >= 1 && d->xa_tk <= 96 && d->xa_tq > 0 && d->xa_tq % 128 == 0 &&
                       d->M % d->xa_tq == 0 && d->xa_ldvt >= 128 && d->xa_ldvt % 8 == 0 && d->xa_ldk % 8 == 0 &&
                       d->xa_vt_heads >= d->N / 64 && ((uintptr_t)d->xa_k & 15) == 0 && ((uintptr_t)d->xa_vt & 15) == 0,
                   "xa_* need head dim 64 (N %% 64 == 0), 1 <= xa_tk <= 96, xa_tq %% 128 == 0, M %% xa_tq == 0, "
                   "xa_ldvt >= 128 (two 64-key tiles are staged), 16-byte aligned keys / values");
    }
    return 0;
}

extern "C" int slh_gemm_tile_ok(const slh_gemm_desc* d) {
    GemmTile t;
    return gemm_check(d, t) == 0;
}

extern "C" int slh_gemm_ln_chunk_cols(const slh_gemm_desc* d) {
    GemmTile t;
    if (!d || !d->ln_out || gemm_check(d, t) != 0) return 0;
    return t.bn == 160 ? 80 : 64;      // a wave of the 64 x 160 tile and of 0x7645 owns 80 columns; every other tile's chunks are 64 wide
}

extern "C" int slh_gemm(const slh_gemm_desc* d, slh_stream_t stream) {
    GemmTile t;
    const int rc = gemm_check(d, t);
    if (rc) return rc;
    SLH_CHECK(!(d->ln_in && d->lora_down) || (d->ln_lora_s && d->ln_lora_c),
              "slh_gemm: ln_in with a fused adapter needs ln_lora_s / ln_lora_c (lora_down = A . gamma)");
    if (t.family == GEMM_FOURWAVE) return slh_gemm7_launch(d, t, stream);
    if (t.family == GEMM_64X160) return slh_gemm5_launch(d, t, stream);
    GemmArgs a;
    memset(&a, 0, sizeof(a));      // padding included: a field this function forgets is zero in the kernel, and the query hashes these bytes
    a.a0 = (const __bf16*)d->a0; a.a1 = (const __bf16*)d->a1; a.w = (const __bf16*)d->w;
    a.bias = (const __bf16*)d->bias; a.rowbias = (const __bf16*)d->rowbias; a.lora_t = d->lora_t;
    a.lora_up = (const __bf16*)d->lora_up; a.lora_scale = d->lora_scale;
    a.residual = (const __bf16*)d->residual; a.c = (__bf16*)d->c;
    a.lora_down = (const __bf16*)d->lora_down; a.lora_t_out = d->lora_t_out;
    a.lda0 = d->lda0; a.lda1 = d->lda1; a.ca0 = d->ca0; a.ca1 = d->ca1;
    a.hs = d->hs; a.ws = d->ws; a.src_xform = d->src_xform; a.stride = d->stride; a.ho = d->ho; a.wo = d->wo;
    a.ldw = d->ldw; a.M = d->M; a.N = d->N; a.K = d->K;
    a.ld_rowbias = d->ld_rowbias; a.rows_per_sample = d->rows_per_sample > 0 ? d->rows_per_sample : 1;
    a.ld_t = d->ld_t; a.lora_cols_per_group = (d->lora_t || d->lora_down) ? d->N / d->lora_groups : 1;
    a.ld_res = d->ld_res; a.ldc = d->ldc; a.geglu = d->geglu;
    a.lora_rank = d->lora_rank > 0 ? d->lora_rank : 4; a.lora_up_rmajor = d->lora_up_rmajor;
    a.w_packed = d->w_layout;
    a.vt = (__bf16*)d->vt_out; a.vt_col0 = d->vt_col0; a.vt_D = d->vt_D; a.vt_heads = d->vt_heads;
    a.vt_tokens = d->vt_tokens; a.vt_ld = d->vt_ld;
    a.ln_out = d->ln_out; a.ln_in = d->ln_in; a.ln_s = d->ln_s; a.ln_b = d->ln_b;
    a.ln_in_chunks = d->ln_in_chunks; a.ln_eps = d->ln_eps;
    a.c32 = d->splitk_c32;
    a.t32 = d->splitk_t32;
    a.ticket = (unsigned long long*)d->splitk_ticket;
    a.ln_mr_out = d->ln_mr_out;
    a.geglu_pre = (__bf16*)d->geglu_pre; a.ld_pre = d->ld_pre;
    a.vt_also_c = d->vt_also_c;
    // same-XCD slab reads (gemm_common.h, split-K epilogue): gfx950 only, SLIDERS_SPLITK_LOCAL=0 turns them off (a query answers 1)
    static const int splitk_local_ok = [] {
        const char* e = getenv("SLIDERS_SPLITK_LOCAL");
        if (e && atoi(e) == 0) return 0;
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
        return strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
    }();
    a.splitk_local = slh_name_mode() ? 1 : splitk_local_ok;
    a.splitk = gemm_splitk(d, t, a.kper);
    if (a.splitk > 1) {
        SLH_CHECK(d->splitk_c32, "slh_gemm: split-K needs the fp32 slab workspace splitk_c32");
        SLH_CHECK(d->splitk_slabs >= a.splitk, "slh_gemm: split-K into %d slices but the workspace holds %d slabs", a.splitk,
                  d->splitk_slabs);
        SLH_CHECK(d->splitk_ticket, "slh_gemm: split-K needs the arrival tickets splitk_ticket (zeroed once)");
        SLH_CHECK(((uintptr_t)d->splitk_ticket & 7) == 0 && d->N % 4 == 0, "slh_gemm: split-K needs N %% 4 == 0 and 8-byte aligned tickets");
        SLH_CHECK(!d->lora_down || a.t32, "slh_gemm: split-K with a fused adapter needs the slab workspace splitk_t32");
        SLH_CHECK(((uintptr_t)d->splitk_c32 & 15) == 0 && ((uintptr_t)d->splitk_t32 & 15) == 0, "slh_gemm: slab alignment");
    }
    a.store16 = (d->ldc % 8 == 0) && (((uintptr_t)d->c & 15) == 0);
    a.ln_lora_s = d->ln_lora_s; a.ln_lora_c = d->ln_lora_c;
    a.xa_k = (const __bf16*)d->xa_k; a.xa_vt = (const __bf16*)d->xa_vt;
    a.xa_tk = d->xa_tk; a.xa_tq = d->xa_tq; a.xa_ldk = d->xa_ldk; a.xa_ldvt = d->xa_ldvt; a.xa_vt_heads = d->xa_vt_heads;
    a.xa_scale = d->xa_scale;
    a.tiles_m = (d->M + t.bm - 1) / t.bm;
    a.tiles_n = (d->N + t.bn - 1) / t.bn;
    a.group_m = pick_group_m(d, a.tiles_m);
    hipStream_t s = (hipStream_t)stream;
    if (t.family == GEMM_PINGPONG) return launch_gemm8p(a, d->mode, t.mi == 4 ? 0 : t.ni, s);
    if (d->pf_ptr && d->pf_bytes >= 16 && t.wm == 4 && t.mi == 1 && t.ni == 2 && t.slots == 4) {
        // the weight touch is a hint: taken only on the 128 x 128 ring tile (0x4412: one workgroup per CU) and only when the launch
        // leaves CUs idle
        SLH_CHECK(((uintptr_t)d->pf_ptr & 15) == 0, "slh_gemm: pf_ptr must be 16-byte aligned");
        const int idle = slh_ncu() - a.tiles_m * a.tiles_n * (a.splitk > 1 ? a.splitk : 1);
        if (idle >= 16) { a.pf_ptr = d->pf_ptr; a.pf_bytes = (long)d->pf_bytes; a.pf_blocks = idle < 64 ? idle : 64; }
    }
    if (d->xa_k) return launch_gemm_xa(a, s);
    if (t.wm == 4) {
        if (t.mi == 2) return launch_gemm<2, 2, 4>(a, d->mode, t.slots, s);   // 256 x 128, 8 waves
        if (t.ni == 1) return launch_gemm<1, 1, 4>(a, d->mode, t.slots, s);   // 128 x 64, 8 waves
        return launch_gemm<1, 2, 4>(a, d->mode, t.slots, s);                  // 128 x 128, 8 waves
    }
    if (t.mi == 2 && t.ni == 2) return launch_gemm<2, 2, 2>(a, d->mode, t.slots, s);
    if (t.mi == 2 && t.ni == 1) return launch_gemm<2, 1, 2>(a, d->mode, t.slots, s);
    if (t.mi == 1 && t.ni == 2) return launch_gemm<1, 2, 2>(a, d->mode, t.slots, s);
    return launch_gemm<1, 1, 2>(a, d->mode, t.slots, s);
}
