/*
 * sliders_hip.h - C ABI of libsliders_hip.so, the MI355X (gfx950) UNet-denoise hot path for
 * concept-slider LoRA training.
 *
 * What this boundary replaces in the reference (rohitgandikota/sliders):
 *   the model call  unet(latent_model_input, timestep, encoder_hidden_states=..., added_cond_kwargs=...)
 *   at trainscripts/textsliders/train_util.py:159-163 and :242-247 (diffusers-0.20.2
 *   UNet2DConditionModel.forward, a third-party dependency), the per-layer LoRA patch
 *   LoRAModule.forward at trainscripts/textsliders/lora.py:108-112, the CFG combine at
 *   train_util.py:166-169 / 250-253, scheduler.step at train_util.py:193 / 291, the guidance loss at
 *   trainscripts/textsliders/prompt_util.py:108-148, loss.backward()/optimizer.step() at
 *   trainscripts/textsliders/train_lora_xl.py:345-346.
 *
 * Conventions
 *   - every entry point is asynchronous on the caller-supplied hipStream_t, takes raw device pointers,
 *     never allocates, returns 0 on success and a negative code on a bad descriptor / launch failure
 *     (message via slh_last_error()).
 *   - activations are bf16, "pixel-major": a (B,C,H,W) tensor of the reference is stored as the row-major
 *     matrix [B*H*W][C] with an explicit row stride (ld, in elements).  Latents at the model boundary stay
 *     in the reference's (B,4,H,W) layout.
 *   - fp32 accumulation everywhere; bf16 is rounded once per op output.
 *   - one host thread per GPU/process; no global mutable state besides the last-error string.
 */
#ifndef SLIDERS_HIP_H
#define SLIDERS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* slh_stream_t; /* hipStream_t */

int slh_version(void);   /* 2: slh_op_info (keyed by opcode) replaced the positional list of descriptor sizes; SLH_OP_MEMSET has an entry point, slh_memset */
const char* slh_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * slh_gemm: C[M][N] = epilogue( A[M][K] . W[N][K]^T )   bf16 MFMA (32x32x16), fp32 accumulate.
 * Replaces every nn.Linear / 1x1 Conv2d / 3x3 Conv2d of the diffusers UNet together
 * with the LoRA up-projection of LoRAModule.forward (lora.py:108-112): the rank-r product
 * lora_scale * T[M][r] . Bup[N][r]^T is added in the epilogue (T comes from slh_skinny).
 * mode 1 gathers A on the fly from a pixel-major image (implicit-GEMM 3x3 conv, pad 1, stride 1|2,
 * optional nearest-2x upsample read (Upsample2D) or zero-dilated read (dgrad of the stride-2 conv),
 * optional two-source channel concat (up-block skip cat)); K index = tap*Cin + c.
 * ---------------------------------------------------------------------------------------------- */
typedef struct slh_gemm_desc {
    const void* a0;          /* source 0 (bf16) */
    const void* a1;          /* source 1 or NULL: channels [ca0, ca0+ca1) */
    const void* w;           /* bf16 weights: [N][ldw] row-major (w_layout 0) or tile-packed (w_layout 1) */
    const void* bias;        /* [N] bf16 or NULL */
    const void* rowbias;     /* [batch][ld_rowbias] bf16 or NULL: per-sample per-channel add (time embedding) */
    const float* lora_t;     /* [M][ld_t] fp32 or NULL */
    const void* lora_up;     /* [N][4] bf16 */
    const float* lora_scale; /* device scalar: multiplier * alpha / rank */
    const void* residual;    /* [M][ld_res] bf16 or NULL (may alias c) */
    void* c;                 /* [M][ldc] bf16 (N/2 columns when geglu) */
    const void* lora_down;   /* [rank][K] bf16 or NULL: FUSED down-projection, T = A.lora_down^T is computed inside
                                the same kernel (rank = 4*lora_groups <= 12); excludes lora_t.  In the forward form (lora_up [N][4])
                                lora_scale * T is ROUNDED TO bf16 ahead of the up-projection, which runs as one more MFMA (the
                                reference's lora_down output is a bf16 tensor too); lora_t_out receives the unrounded fp32 T.  The
                                backward-data form (lora_up_rmajor) and an external lora_t keep T in fp32 */
    float* lora_t_out;       /* optional [M][ld_t] fp32: the fused T, kept for the backward pass */
    int32_t lda0, lda1, ca0, ca1;
    int32_t mode;            /* 0 dense, 1 conv3x3 */
    int32_t batch, hs, ws;   /* conv: source image dims */
    int32_t src_xform;       /* conv: 0 none, 1 nearest upsample x2, 2 zero-dilate x2 */
    int32_t stride;          /* conv: 1 or 2 */
    int32_t ho, wo;          /* conv: output dims */
    int32_t ldw;
    int32_t M, N, K;
    int32_t ld_rowbias, rows_per_sample;
    int32_t ld_t, lora_groups; /* N/lora_groups columns share one rank-4 slice of T */
    int32_t ld_res, ldc;
    int32_t geglu;           /* 1: out[:, j] = a_j * gelu(g_j); W rows pre-permuted in 64-row blocks [32 a | 32 g].
                                2: backward form, for the backward-data product of the Linear BEHIND a GEGLU: the result d(ff)
                                [M][N] leaves as d(proj) [M][2N] in proj's blocked column order, computed with the forward's
                                pre-activation geglu_pre (slh_elementwise GEGLU_BWD fused; bare product only).
                                3: as 1 with W rows pre-permuted in 32-row blocks [16 a | 16 g] (any tile; no geglu_pre) */
    int32_t tile;            /* bits 0-15 all zero: auto (the heuristic picks one of the ring codes below; S may still be set).  Any other
                                code must be complete: every nibble of bits 0-15 is read by the dispatch or must be zero, and a code
                                that names no kernel is refused (unknown WM or stages, MI = 0, stages bits on a WM = 8 code, a
                                0x5xxx / 0x7xxx code other than those listed below).
                                Else (S<<16)|(WM<<12)|(stages<<8)|(MI<<4)|NI, MI,NI in {1,2}, WM in {0|2, 4}: WM*2 waves per
                                workgroup, block tile (32*MI*WM) x (64*NI); stages 0|2: double buffer, 3|4: deep LDS ring;
                                S: split-K factor (0|1 none), needs splitk_c32.
                                WM = 8: ping-pong K loops, one 8-wave workgroup per CU (csrc/gemm8p.hip): 0x8042 = 256 x 256
                                (no fused adapter), 0x801<NI> = 128 x 64*NI, NI = 3..5 (geglu 0 | 3 only, no ln_out / vt_out).
                                Bits 20 and up must be zero.  (Round 4 carried a stream-K form under bit 20 whose finishing
                                workgroups waited on flags of other workgroups; it was slower than the plain launch on every
                                shape and could hang two concurrent launches - removed: no kernel of this library waits on
                                another workgroup, profiles/r04_streamk.txt keeps the measurement.) */
    int32_t lora_rank;       /* 0 = 4.  With lora_up_rmajor: total rank 4 | 8 | 12 (T has that many columns) */
    int32_t lora_up_rmajor;  /* 1: lora_up is [rank][N] (= lora_down as stored): backward-data LoRA term */
    int32_t w_layout;        /* 0: w is [N][ldw].  1: frozen weights repacked once at load time into the order the kernel
                                streams them: [ceil(N/64)][K/64] blocks of 64 rows x 64 k (8 KB contiguous, rows past N
                                zero), 16-byte slot s of row r stored at slot s ^ ((r>>1)&7) (the LDS swizzle applied
                                in memory, so every LDS-DMA instruction reads 1 KB of consecutive addresses); ldw unused */
    int32_t reserved_;       /* 0 (ignored; rounds 2-5 read ablation bits from it in probe builds - those builds are gone) */
    float* splitk_c32;       /* split-K workspace or NULL: splitk_slabs slabs of roundup(M, 256) * roundup(N, 128) floats each (the
                                partial tiles are kept whole, in accumulator order), any contents.  With tile bits 16-19 =
                                S > 1 the K range is cut into S slices; each slice's workgroups publish their partial tiles in
                                slab number <slice> (write-through stores - no fp32 atomics, whose arrival-order sums make a
                                pass differ from run to run), take a ticket of their tile (splitk_ticket), and the slice that
                                arrives LAST adds the slabs IN SLICE ORDER and runs the ordinary epilogue - one launch, every
                                epilogue option available, bit-reproducible.  For the few-tile, long-K products (1280-channel
                                3x3 convolutions at 8x8 / 16x16: 10-40 output tiles on 256 CUs, 29 MB of weights each) this
                                is what fills the chip. */
    float* splitk_t32;       /* with lora_down and S > 1: [ceil(N / (64*NI))][2*S][M][ld_t] fp32 - per column tile, two slabs
                                per slice of the adapter's T (size it for NI = 1: ceil(N/64) * 2 * splitk_slabs * M * ld_t) */
    void* vt_out;            /* optional: the columns >= vt_col0 of the result (the V third of a fused q|k|v projection,
                                diffusers Attention.to_v) are written HEAD-TRANSPOSED for slh_attn_fwd instead of into c:
                                vt_out[((b*vt_heads + h)*Dp + d)*vt_ld + t] = C[b*vt_tokens + t][vt_col0 + h*vt_D + d],
                                Dp = 64*ceil(vt_D/64) - exactly what slh_transpose_heads would produce from c, without
                                the extra launch and the round trip of V through HBM.  Needs vt_D % 64 == 0 (no padded
                                rows), vt_col0 % 128 == 0, vt_tokens % 8 == 0, M % 8 == 0; not with geglu; vt_ld == vt_tokens
                                (slh_transpose_heads zero-fills padding columns up to its ldt; this epilogue writes the vt_tokens
                                columns only, so a padded row is refused rather than left half-initialised) */
    int32_t vt_col0, vt_D, vt_heads, vt_tokens, vt_ld;
    int32_t splitk_slabs;    /* slabs splitk_c32 holds (>= the S of tile) */
    /* LayerNorm folded into the products around it (BasicTransformerBlock.norm1/2/3 of the no-grad passes: no LayerNorm
     * launch, no round trip of the normalised tensor through HBM).
     *   producer (the GEMM that writes the tensor LayerNorm reads): ln_out [N/64][M][2] fp32 (chunk-major: a wave's 32 rows
     *     are contiguous for both sides) receives (mean, M2) of every 64-column chunk of every row of the bf16 result;
     *     needs a 128-column tile, no GEGLU / vt_out.
     *   consumer (dense, single source, K = LayerNorm width <= 1280): ln_in = the producer's ln_out, ln_in_chunks = K/64 (K/80
     *     behind a producer on the 64 x 160 tile: equal-sized chunks of either width merge the same way);
     *     w must hold W * gamma, ln_s [N] fp32 its row sums, ln_b [N] fp32 = bias + W . beta (bias must be NULL):
     *     c = rstd_m * (a . w^T - mean_m * ln_s) + ln_b, the row's mean / rstd merged from the chunks in a fixed order. */
    float* ln_out;
    const float* ln_in; const float* ln_s; const float* ln_b;
    int32_t ln_in_chunks;
    float ln_eps;
    void* splitk_ticket;     /* with S > 1: one 64-bit arrival ticket per output tile ([ceil(M/64) * ceil(N/64)] is enough for
                                every tile shape), zero before the first launch, left zero by every launch */
    float* ln_mr_out;        /* with ln_in, optional: [M][2] fp32 receives the merged (mean, rstd) of every row - what
                                slh_layernorm would have left in mean_rstd for slh_layernorm_bwd (training passes) */
    void* geglu_pre;         /* geglu = 1, optional: [M][ld_pre] bf16 RECEIVES proj(x) itself (bf16-rounded, this product's column
                                order = what the same call without geglu writes to c).  geglu = 2: the same array, READ */
    int32_t ld_pre;
    int32_t vt_also_c;       /* with vt_out: 1 = the head-transposed columns are ALSO written row-major into c (training passes
                                keep V, and the backward dO, in both layouts: no separate transpose launch) */
    /* Cross-attention fused behind the query projection (diffusers Attention.to_q of attn2 + the xformers call behind it, no-grad
     * passes, head dim 64): with xa_k the product is Q = a . w^T (bf16-rounded, LayerNorm fold / bias applied first) and c receives
     *   softmax(Q_h K_h^T * xa_scale) V_h   per (sample, head h = columns [64h, 64h + 64))
     * for the xa_tk <= 96 keys of the row's sample (text tokens): every wave of the 128 x 128 ring tile (tile 0x4412, required) owns
     * 32 rows x one head, so scores, softmax and P.V stay in its registers (24 MFMAs behind the K loop; K / V^T of the workgroup's
     * two heads staged once through LDS) and neither Q nor a second launch exists.  xa_k: this layer's keys, [B][xa_tk][xa_ldk]
     * with head h in columns [64h, 64h + 64); xa_vt: this layer's first head inside a head-transposed V
     * [B][xa_vt_heads][64][xa_ldvt >= 128] (slh_transpose_heads layout, key columns >= xa_tk zero); both 16-byte aligned;
     * xa_tq = rows per sample (a multiple of 128).  Excludes residual, row bias, adapters, GEGLU, ln_out, vt_out, split-K. */
    const void* xa_k; const void* xa_vt;
    int32_t xa_tk, xa_tq, xa_ldk, xa_ldvt, xa_vt_heads;
    float xa_scale;
    /* ln_in together with a fused adapter (lora_down; ping-pong tiles 0x8013 / 0x8014 only): lora_down must hold A . gamma (bf16, what
     * slh_lora_ln_fold writes) and the down-projection is normalised like the main product,
     *   T = rstd_m * (a . (A gamma)^T - mean_m * ln_lora_s) + ln_lora_c,   ln_lora_s = row sums of the rounded A gamma, ln_lora_c = A . beta
     * (fp32 [rank] each), ahead of the up-projection - Linear(LayerNorm(x)) + LoRA(LayerNorm(x)) without the LayerNorm launch. */
    const float* ln_lora_s; const float* ln_lora_c;
    /* Optional hint: pf_bytes of frozen weights at pf_ptr (16-byte aligned) that a LATER launch will stream are touched by up to 64
     * extra workgroups of THIS launch when its grid leaves that many CUs idle (the 160-tile products of the M = 2048 level: the
     * touch rides on CUs that have nothing to do and costs no launch, no second stream, no graph edge).  A UNet pass reads every
     * matrix once, so the big ones are HBM-cold at first touch (2048 x 1280 x 5120: 56 us cold, 47 us after a touch).  Ignored
     * when the grid fills the chip or the tile is a ping-pong one. */
    const void* pf_ptr; int64_t pf_bytes;
} slh_gemm_desc;
int slh_gemm(const slh_gemm_desc* d, slh_stream_t stream);
/* Name of the kernel instantiation slh_gemm would launch for d, as rocprofv3 --kernel-trace prints it without namespace and parameter
 * list (e.g. "gemm8pb_kernel<1, 5, 0, false>", "gemm5_kernel<false, 4>"), written to buf (cap >= 16 bytes, NUL-terminated).  All of
 * slh_gemm's checks and its dispatch run; the launch is replaced by a record of the selected template, so the name is exact for
 * every present and future tile.  Needs no device and launches nothing.  0, or the status slh_gemm would return for d.
 * (bench.py / scripts/make_pmc_traffic.py pair in-situ event times and PMC rows by this name.) */
int slh_gemm_kernel_name(const slh_gemm_desc* d, char* buf, int cap);
/* slh_gemm_kernel_name plus the launch: the grid (workgroups), the block size (threads) and a 64-bit FNV-1a hash of the bytes of the
 * argument struct the kernel would receive (zeroed before it is filled, padding included).  A function of the descriptor alone: the two
 * inputs slh_gemm takes from the machine are fixed in a query - 256 CUs behind the weight touch, same-XCD split-K slab reads on - so
 * the answer is the same without a device and on an MI355X (tests/data/gemm_dispatch.json pins it: a change of the dispatch that keeps
 * every result but moves a grid, a group_m or a split-K cut shows there).  0, or the status slh_gemm would return for d. */
int slh_gemm_launch_query(const slh_gemm_desc* d, char* name, int cap, int32_t* grid, int32_t* block, uint64_t* args_hash);
/* The 64 x 160 tile (tile codes 0x5425: 4-slot LDS ring, 0x5525: 5 slots - no other 0x5xxx code is accepted; csrc/gemm5.hip): 4 waves
 * of 32 x 80 on the 16 x 16 x 32 MFMA - the M = 2048, N = 1280 products as 256 workgroups = one full round of the chip.  Dense single-source products with packed
 * weights (w_layout = 1), M % 64 == 0, N % 160 == 0; epilogue: bias, residual, ln_out - whose chunks are then 80 COLUMNS wide:
 * ln_out [N/80][M][2], and the consumer's ln_in_chunks = K / 80. */
/* The tiles of csrc/gemm7.hip (tile code bits 12-15 = 7: 0x7<S><XB><WB>): 128 x 256 (0x7648) and 128 x 160 (0x7645) - four loader waves
 * that issue the ring's LDS-DMA + four compute waves, one per SIMD, each a 64 x (16 WB) register tile of 16 x 16 x 32 MFMAs - and 256 x 320
 * (0x748a) on eight compute waves that stage the ring themselves (GEGLU.proj as one round of 256 workgroups); ring of S half K tiles (32
 * deep).  Dense single-source products with packed weights (w_layout = 1, w 128-byte aligned), M % (32 XB) == 0, N % (32 WB) == 0,
 * K % 64 == 0, K >= 32 S.  Epilogue: bias, residual, ln_in, geglu = 3 on all three; on the 128-row tiles also ln_out (64-column chunks;
 * 80-column chunks on 0x7645), ln_mr_out, vt_out / vt_also_c (vt_col0 % (16 WB) == 0, vt_tokens % 128 == 0, vt_ld == vt_tokens) and - 0x7648 only - one fused
 * adapter of 1-3 column groups (forward form, every tile inside one group; with ln_in also its own fold: ln_lora_s / ln_lora_c) and
 * lora_t_out.  No split-K, row bias, external T, geglu 1 / 2, cross-attention. */
/* 1 where the tile named by d->tile (0: the one slh_gemm's own heuristic picks) can run d's shape and features: every check of
 * slh_gemm except what a caller provisions once the tile is chosen - the split-K slab / ticket workspace and its slab count, and
 * ln_lora_s / ln_lora_c.  slh_gemm runs this check first and returns its status, so a query and a launch cannot disagree.  Needs
 * no device.  The tile code is taken apart in one place (csrc/gemm_dispatch.h: GemmTile) and every contract is stated once, for all
 * families; a refusal names the condition and, once the code is decoded, the tile ("... (64 x 160 tile, 0x5425)"). */
int slh_gemm_tile_ok(const slh_gemm_desc* d);
/* Width of the LayerNorm chunks (ln_out) d's tile writes: 80 columns on the 64 x 160 tile and on 0x7645, 64 on the other tiles
 * that take ln_out (128-column ring tiles, 0x8042, 0x7648) - the producer's ln_out is [N / width][M][2] and its consumers'
 * ln_in_chunks = K / width.  0 when d carries no ln_out or slh_gemm_tile_ok(d) is 0. */
int slh_gemm_ln_chunk_cols(const slh_gemm_desc* d);

/* ------------------------------------------------------------------------------------------------
 * slh_skinny: T[M][R] = A[M][K] . Wd[R][K]^T (+bias), R <= 16, same A addressing as slh_gemm.
 * LoRA down-projection lora_down(x) of lora.py:108-112 (Linear: (r,in); Conv: (r,Cin,k,k) repacked
 * [r][tap][Cin]) and the UNet's conv_out (320 -> 4).  Output fp32 [M][ldo] or bf16 NCHW (conv_out).
 * ---------------------------------------------------------------------------------------------- */
typedef struct slh_skinny_desc {
    const void* a0; const void* a1;
    const void* w;           /* [R][K] bf16 */
    const void* bias;        /* [R] bf16 or NULL */
    void* out;
    int32_t lda0, lda1, ca0, ca1;
    int32_t mode, batch, hs, ws, src_xform, stride, ho, wo;
    int32_t M, R, K;
    int32_t ldo;
    int32_t out_kind;        /* 0: fp32 [M][ldo]; 1: bf16 NCHW [batch][R][ho][wo] */
    int32_t w_kmajor;        /* 1: w is [K][4] (R must be 4): U = dY . B with B = lora_up [out][r] as stored */
} slh_skinny_desc;
int slh_skinny(const slh_skinny_desc* d, slh_stream_t stream);
/* The kernel instantiation slh_skinny would launch for d, written to buf (cap >= 32): "skinny<RMAX,LPR>" with RMAX in {4, 12, 16} the
 * accumulator rows compiled in (rows past R are masked) and LPR in {64, 16} the lanes that share one output row.  Answered by the
 * selection function slh_skinny itself launches through; no device needed, nothing launched.  0, or the error slh_skinny would give. */
int slh_skinny_kernel_name(const slh_skinny_desc* d, char* buf, int cap);

/* ------------------------------------------------------------------------------------------------
 * slh_gemv: y[b][n] = x'[b][:] . W[n][:] + bias[n] + addend[b][n] + lora,  b < nb <= 8 (weight-streaming).
 * TimestepEmbedding MLPs, add_embedding, and all ResnetBlock2D.time_emb_proj layers batched into one
 * launch (they only depend on emb).  in_act 1 applies SiLU to x first.
 * ---------------------------------------------------------------------------------------------- */
typedef struct slh_gemv_desc {
    const void* x;           /* [nb][ldx] bf16 */
    const void* w;           /* bf16 weights: [N][ldw] row-major (w_layout 0) or tile-packed (w_layout 1) */
    const void* bias;        /* [N] bf16 or NULL */
    const void* addend;      /* [nb][ld_add] bf16 or NULL */
    const float* lora_t;     /* [nb][ld_t] fp32 or NULL */
    const int32_t* lora_tcol;/* [N] first T column of row n (NULL: 0) */
    const void* lora_up;     /* [N][4] bf16 */
    const float* lora_scale;
    void* y;                 /* [nb][ldy] bf16 (out_f32: fp32) */
    int32_t nb, N, K, ldx, ld_add, ld_t, ldy;
    int32_t in_act, out_f32;
} slh_gemv_desc;
int slh_gemv(const slh_gemv_desc* d, slh_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GroupNorm (+SiLU) on pixel-major images; x may be a two-source channel concat.
 * slh_gn_stats leaves (sum, sum of squares) pairs per cluster of row blocks; slh_gn_apply (same descriptor, next on the
 * stream) adds a sample's cluster pairs in index order in every workgroup's prologue, writes stats[b][G] = (mean, rstd) and
 * y = act((x-mean)*rstd*gamma+beta).  No fp32 atomics anywhere: bit-reproducible.
 * diffusers ResnetBlock2D.norm1/norm2 (+nonlinearity), Transformer2DModel.norm, conv_norm_out.
 * ---------------------------------------------------------------------------------------------- */
typedef struct slh_gn_desc {
    const void* x0; const void* x1;
    const void* gamma; const void* beta; /* [C] bf16 */
    float* stats;            /* [batch][groups][2] fp32: (mean, rstd), written by slh_gn_apply (and slh_gn_fused) */
    void* y;                 /* [batch*hw][ldy] bf16 */
    int32_t ldx0, ldx1, c0, c1;
    int32_t batch, hw, groups, ldy;
    float eps;
    int32_t act;             /* 0 none, 1 SiLU */
    /* The statistics are reduced in a fixed order: every workgroup of slh_gn_stats (one row block) writes one shifted (sum, sum of
     * squares) pair per group; the LAST workgroup of a cluster of 16 row blocks to arrive (one ticket level) adds the cluster's
     * pairs in row-block order and leaves the cluster pair; slh_gn_apply adds the cluster pairs (double accumulation).
     * With R = slh_gn_row_blocks(c0+c1, hw, groups) and L = slh_gn_clusters(R): */
    float* partial;          /* [batch][R + L][groups][2] fp32 scratch, any contents; must stay untouched between the two launches */
    /* No aliasing: slh_gn_apply re-reads the statistics' pivot (the first element of every group) from x0 / x1 in every workgroup,
     * so y must be a different buffer (checked) and x must be unchanged between slh_gn_stats and slh_gn_apply. */
    uint32_t* ticket;        /* [batch][1 + L] arrival counters, ZERO before the launch (left zero by it) */
} slh_gn_desc;
int slh_gn_stats(const slh_gn_desc* d, slh_stream_t stream);
int slh_gn_apply(const slh_gn_desc* d, slh_stream_t stream);
/* workgroups per sample of slh_gn_stats / slh_gn_bwd_stats, and the clusters they form; -1 for an unsupported shape */
int slh_gn_row_blocks(int channels, int hw, int groups);
int slh_gn_clusters(int row_blocks);
/* Statistics AND normalisation in one launch; also writes stats for the backward.  partial / ticket unused; y must not alias x.
 * slh_gn_fused_ok(channels, hw, groups) = 0 where it does not apply (use the two launches above),
 *   1: tiny tensors (8x8 latents: a sample's group slab is a few KB) - one workgroup per group set keeps the slab in registers;
 *   2: cache-resident slabs (hw <= 4096, hw * channels / groups <= 81920: the 32x32 level and the 640-channel tensors of the 64x64 level of SDXL at 1024^2) -
 *      S = 1..8 sibling workgroups per (sample, group), each of which reduces the WHOLE slab in the same fixed order (identical
 *      statistics, nothing exchanged, nothing waited for) and normalises its own 1/S of it. */
int slh_gn_fused_ok(int channels, int hw, int groups);
int slh_gn_fused(const slh_gn_desc* d, slh_stream_t stream);

/* GroupNorm backward (dx only: gamma/beta are frozen).  Two launches like the forward:
 * bwd_stats reduces per (b,g) sum(dyhat) and sum(dyhat*xhat) into bstats (fixed order, see slh_gn_desc),
 * bwd_apply writes dx (+= into dx if accumulate).  dy is the gradient of the post-activation output. */
typedef struct slh_gn_bwd_desc {
    const void* x0; const void* x1;
    const void* gamma; const void* beta;
    const float* stats;      /* forward stats (mean, rstd) */
    float* bstats;           /* [batch][groups][2] fp32: (sum dxhat, sum dxhat*xhat), written by slh_gn_bwd_stats */
    const void* dy;          /* [batch*hw][lddy] bf16 */
    void* dx0; void* dx1;    /* gradient w.r.t. source 0 / 1 */
    int32_t ldx0, ldx1, c0, c1;
    int32_t batch, hw, groups, lddy, lddx0, lddx1;
    float eps;
    int32_t act;
    int32_t accumulate0, accumulate1; /* dx += instead of = */
    float* bpartial;         /* slh_gn_bwd_stats: scratch like slh_gn_desc.partial */
    uint32_t* bticket;       /* slh_gn_bwd_stats: zeroed arrival counters like slh_gn_desc.ticket */
} slh_gn_bwd_desc;
int slh_gn_bwd_stats(const slh_gn_bwd_desc* d, slh_stream_t stream);
int slh_gn_bwd_apply(const slh_gn_bwd_desc* d, slh_stream_t stream);

/* LayerNorm over the last dim (BasicTransformerBlock.norm1/2/3), one wave per row. */
typedef struct slh_ln_desc {
    const void* x; const void* gamma; const void* beta;
    void* y;
    float* mean_rstd;        /* [M][2] fp32 or NULL (saved for backward) */
    int32_t M, C, ldx, ldy;
    float eps;
} slh_ln_desc;
int slh_layernorm(const slh_ln_desc* d, slh_stream_t stream);

typedef struct slh_ln_bwd_desc {
    const void* x; const void* gamma; const void* dy;
    const float* mean_rstd;
    void* dx;                /* dx (+)= LN-backward(dy) */
    int32_t M, C, ldx, lddy, lddx;
    int32_t accumulate;
} slh_ln_bwd_desc;
int slh_layernorm_bwd(const slh_ln_bwd_desc* d, slh_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Attention: O = softmax(Q K^T * scale) V per (sample, head); head dims 64 (SDXL), 40/80/160 (SD-1.x).
 * Q [B][Tq][ldq] (head h at columns h*D..), K [B][Tk][ldk], VT [B][H][Dp][ldvt] (V transposed by
 * slh_transpose_heads, Dp = 64*ceil(D/64)), O [B][Tq][ldo]; lse [B][H][Tq] fp32 (log2 domain) or NULL.
 * Replaces Attention + XFormersAttnProcessor (train_lora.py:68).
 * ---------------------------------------------------------------------------------------------- */
typedef struct slh_attn_desc {
    const void* q; const void* k; const void* vt;
    void* o;
    float* lse;
    int32_t B, H, Tq, Tk, ldq, ldk, ldvt, ldo;
    float scale;
    int32_t D;               /* head dim: 0/64 (SDXL) or 40 / 80 / 160 (SD-1.x); head h = columns [h*D, (h+1)*D);
                                VT is [B][H][64*ceil(D/64)][ldvt] with zero rows for d >= D */
    int32_t vt_batch_heads;  /* 0 = H.  Otherwise vt points into a wider [B][vt_batch_heads][..][ldvt] array (one transposed
                                V for the cross-attention of every transformer block) at this layer's first head */
    int32_t reserved_;
    /* Optional weight touch (as slh_gemm_desc.pf_*): pf_bytes bytes at pf_ptr (16-byte aligned) - the packed weights of a product a
     * few launches later - are streamed through the memory-side cache by up to 64 extra workgroups dispatched behind the launch's own.
     * A hint: taken only by the key-split form (the self-attention of the 32 x 32 level, whose workgroups all fit the chip at once, so
     * the touch runs beside them); slh_attn_fwd_carries_touch(d) = 1 where it would be.  NULL / 0 = none. */
    const void* pf_ptr; int64_t pf_bytes;
} slh_attn_desc;
int slh_attn_fwd(const slh_attn_desc* d, slh_stream_t stream);
int slh_attn_fwd_carries_touch(const slh_attn_desc* d);
/* The kernel instantiation slh_attn_fwd would launch for d, as a profiler prints it ("attn_fwd_kernel<4, 1, true>": workgroup waves,
 * d-tiles, masked tail tile; "attn_fwd_ks_kernel": the key-split form), written to buf (cap >= 32).  Answered by the dispatch code
 * itself, environment knobs included; no device needed, nothing launched.  0, or the error slh_attn_fwd would give. */
int slh_attn_fwd_kernel_name(const slh_attn_desc* d, char* buf, int cap);

/* src [B][T][ld] columns [h*64,(h+1)*64) -> dst [B][H][64][ldt] (columns >= T zero-filled up to ldt) */
typedef struct slh_transpose_desc {
    const void* src; void* dst;
    int32_t B, H, T, ld, ldt;
    int32_t D;               /* head dim (0 = 64); dst is [B][H][64*ceil(D/64)][ldt] */
} slh_transpose_desc;
int slh_transpose_heads(const slh_transpose_desc* d, slh_stream_t stream);

/* Attention backward.  dQ (and dK/dV when self-attention) given dO, Q, K, V, O, lse.
 * All operands [B][T][ld] pixel-major with heads in columns; transposed copies are built internally
 * in the caller-provided workspace.  need_dkv = 0 for cross-attention (text K/V carry no gradient). */
typedef struct slh_attn_bwd_desc {
    const void* q; const void* k; const void* v; const void* o; const void* d_o;
    const void* kt;          /* [B][H][64][ldkt] K transposed (slh_transpose_heads) */
    const void* qt;          /* [B][H][64][ldqt] Q transposed   (need_dkv only) */
    const void* dot;         /* [B][H][64][ldqt] dO transposed  (need_dkv only) */
    const float* lse;        /* [B][H][Tq] from the forward, padded by 64 floats: the dK/dV kernel reads up to 63 floats past the end. */
    float* delta;            /* [B][H][Tq] fp32 workspace, padded by 64 floats.  The padding of both may hold ANYTHING (NaN, Inf,
                                recycled memory): it is read, never used, and never written */
    void* dq; void* dk; void* dv;
    int32_t B, H, Tq, Tk, ldq, ldk, ldv, ldo, lddo, ldkt, ldqt, lddq, lddk, lddv;
    float scale;
    int32_t need_dkv;
    int32_t D;               /* head dim (0 = 64); kt / qt / dot use the padded [B][H][64*ceil(D/64)][ld] layout */
    int32_t pad_;
} slh_attn_bwd_desc;
int slh_attn_bwd(const slh_attn_bwd_desc* d, slh_stream_t stream);
/* The dq and dkv instantiations slh_attn_bwd would launch for d ("attn_bwd_dq_kernel<2>", "attn_bwd_dkv_kernel<2, 2>": d-tiles, query
 * tile buffers; dkv = "" with need_dkv = 0), each written to a buffer of cap >= 32 bytes.  No device needed, nothing launched. */
int slh_attn_bwd_kernel_names(const slh_attn_bwd_desc* d, char* dq, char* dkv, int cap);

/* ------------------------------------------------------------------------------------------------
 * small ops
 * ---------------------------------------------------------------------------------------------- */
/* sinusoidal timestep embedding (Timesteps(dim, flip_sin_to_cos=True, freq_shift=0)), fp32 math -> bf16.
 * out[b][col0 + j*dim + 0..dim) for each of the n_vals values vals[b][j] (fp32). */
typedef struct slh_tembed_desc {
    const float* vals; void* out;
    int32_t nb, n_vals, dim, ldo, col0;
} slh_tembed_desc;
int slh_timestep_embed(const slh_tembed_desc* d, slh_stream_t stream);

/* conv_in: (B,Cin<=8,H,W) bf16 NCHW -> pixel-major [B*H*W][Cout], 3x3 pad 1, w [Cout][9*Cin] (tap-major) */
typedef struct slh_convin_desc {
    const void* x; const void* w; const void* bias; void* y;
    int32_t batch, cin, h, wd, cout, ldy;
} slh_convin_desc;
int slh_conv_in(const slh_convin_desc* d, slh_stream_t stream);

/* generic elementwise helpers on bf16 matrices [M][C] (8 channels per thread) */
typedef struct slh_ew_desc {
    const void* a; const void* b; void* out;
    int32_t M, C, lda, ldb, ldo;
    int32_t op;              /* see SLH_EW_* */
    int32_t iarg, iarg2;
    float alpha;
    int32_t pad_;
} slh_ew_desc;
enum {
    SLH_EW_COPY = 0,         /* out = a */
    SLH_EW_ADD = 1,          /* out = a + b */
    SLH_EW_GEGLU_FWD = 2,    /* a = GEGLU.proj output [M][2C] in 64-column blocks [32 values | 32 gates] ->
                                out[M][C] = value * gelu(gate)  (training forward keeps the pre-activation) */
    SLH_EW_GEGLU_BWD = 3,    /* a as above, b = d(out) [M][C] -> out = d(proj) [M][2C], same blocked layout */
    SLH_EW_UPSAMPLE_BWD = 4, /* a = d(upsampled) (2h x 2w image) -> out = 2x2 block sums; M = B*h*w, iarg = w, iarg2 = h*w */
    SLH_EW_COLSUM = 5        /* out (fp32 [B][ldo], +=) = per-sample column sums of a; iarg2 = rows per sample */
};
int slh_elementwise(const slh_ew_desc* d, slh_stream_t stream);

/* CFG combine + DDIM step (train_util.py:166-169 + scheduler.step, eta = 0), bf16 rounding points as the
 * reference's tensor ops.  eps [2*nb][chw] (uncond half first), x [nb][chw] -> x_prev; also used with
 * do_step = 0 to produce only the guided epsilon (predict_noise). */
typedef struct slh_cfg_ddim_desc {
    const void* eps; const void* x; void* out;
    void* out2;              /* optional second copy of the result (the CFG pair's duplicated latent input) */
    const void* eps_text;    /* optional: text-half epsilon [nb][chw] when it is not stored right after the uncond half */
    int32_t nb, chw;
    float guidance;
    float c_sqrt_beta_t, c_inv_sqrt_alpha_t, c_sqrt_alpha_prev, c_dir;
    int32_t do_step;
    int32_t v_prediction;    /* 1: the network predicts v (SD-2.x 768-v; model_util.py:126 prediction_type="v_prediction"):
                                x0 = sqrt(a_t) x - sqrt(1-a_t) v, eps = sqrt(a_t) v + sqrt(1-a_t) x, same rounding points
                                as the DDIMScheduler.step tensor ops */
    float c_sqrt_alpha_t;    /* v_prediction only: alpha_prod_t ** 0.5 (fp32) */
    int32_t pad_;
} slh_cfg_ddim_desc;
int slh_cfg_ddim(const slh_cfg_ddim_desc* d, slh_stream_t stream);

/* One step of the residual DDPM noise space that edits a given image (sliders_amd/edit.py, docs/EDIT.md): CFG combine, the DDIM
 * mean mu of x_{t-1} (the formulas of slh_cfg_ddim, but fp32 throughout on an fp32 master latent, one rounding per operation, no
 * contraction), then
 *   mode 0 (invert): resid = target - mu is written;   mode 1 (edit): resid is read;   both: out = mu + resid.
 * mu is computed ahead of the mode branch, so an edit over the same epsilon and the inversion's residuals reproduces the
 * inversion's `out` bit for bit.  The bf16 copies are the round-to-nearest-even of out. */
typedef struct slh_ddpm_edit_desc {
    const void* eps;         /* bf16 [2*nb][chw], uncond half first */
    const void* eps_text;    /* optional, as slh_cfg_ddim_desc */
    const float* x;          /* fp32 [nb][chw] master latent x_t */
    const float* target;     /* mode 0: x_{t-1} of the constructed path (x0 on the last step); mode 1: unused, may be NULL */
    float* resid;            /* fp32 [nb][chw]; mode 0: written, mode 1: read */
    float* out;              /* fp32 x_{t-1}; may alias x */
    void* out_bf16; void* out2_bf16;   /* optional bf16 copies of out: the two halves of the CFG pair's sample input */
    int32_t nb, chw;
    float guidance;
    float c_sqrt_beta_t, c_inv_sqrt_alpha_t, c_sqrt_alpha_t, c_sqrt_alpha_prev;
    float c_dir;             /* sqrt(1 - alpha_prev - sigma^2): the noise sigma z of a DDPM step is part of resid */
    int32_t mode;            /* 0 invert, 1 edit */
    int32_t v_prediction;    /* as slh_cfg_ddim_desc (c_sqrt_alpha_t is read only then) */
} slh_ddpm_edit_desc;
int slh_ddpm_edit_step(const slh_ddpm_edit_desc* d, slh_stream_t stream);

/* The step between two UNet passes of the samplers euler, euler_a, lms, ddpm and dpmpp_2m on an fp32 master latent: CFG combine,
 * predicted clean sample, multistep update, and the next pass's scaled bf16 input, in one launch (csrc/sigma_step.hip,
 * docs/SAMPLING.md).  Never recorded in a program: it has no opcode and no descriptor struct; it takes three host arrays.  Per
 * element, with u, t the bf16 unconditional and text model outputs and x the master latent, fp32 throughout, one rounding per
 * operation, nothing contracted:
 *   m   = u + g (t - u)                          single branch: m = u, g is not read
 *   x0  = p x + q m
 *   H0  = kind == 0 ? (x - x0) / sigma : x0      0: the derivative (euler, euler_a, lms); 1: the denoised sample (ddpm, dpmpp_2m)
 *   acc = a x;  acc += c[0] H0;  acc += c[k] H[k] for k = 1 .. n_hist ascending;  acc += c_n noise (if noise)
 *   out = acc;  hist_out = H0;  in_bf16 = in2_bf16 = round-to-nearest-even(out * s_next)
 * The rows (p, q, sigma, a, c, c_n, s_next) of every scheduler: sliders_amd/schedulers.py, step_row.
 * ptrs[11]: 0 eps       bf16 [2*nb][chw], unconditional half first ([nb][chw] for the single branch)
 *           1 eps_text  optional, as slh_cfg_ddim_desc (not with the single branch)
 *           2 x         fp32 [nb][chw]
 *           3..5 H[1..3] fp32 [nb][chw], the first n_hist are read (H[1] the newest); the others may be NULL
 *           6 noise     fp32 [nb][chw] or NULL
 *           7 out       fp32 [nb][chw]; may alias x
 *           8 hist_out  optional fp32 [nb][chw]; may alias the oldest history slot that is read, or any slot that is not
 *           9, 10 in_bf16, in2_bf16   optional bf16 [nb][chw]: the two halves of the CFG pair's sample input
 * dims[5]:  0 nb, 1 chw (any value >= 1), 2 n_hist (0..3), 3 kind (0, 1), 4 single (1: the single branch)
 * coef[11]: 0 p, 1 q, 2 sigma (kind 0 only), 3 a, 4..7 c[0..3], 8 c_n, 9 s_next, 10 g
 * Refused before the launch (slh_last_error): a null eps / x / out or a null H[k], k <= n_hist; an fp32 pointer that is not 4-byte
 * or a bf16 pointer that is not 2-byte aligned; nb < 1, chw < 1; n_hist, kind or single out of range; sigma == 0 with kind 0.
 * Apart from the two aliases named above, no output may overlap an input. */
int slh_sigma_step(const void* const* ptrs, const int32_t* dims, const float* coef, slh_stream_t stream);

/* The blend behind every step of a localised sampling run (csrc/latent_blend.hip, docs/SAMPLING.md, "Localised sampling"): the latent
 * a step just produced against the latent the scale-0 chain of the same seed had after the same step, under a mask with one value per
 * latent pixel.  Never recorded in a program: no opcode, no descriptor struct; three host arrays, as slh_sigma_step.  Per element,
 * with k = keep, m = mask, fp32 throughout (bf16 inputs widen exactly), one rounding per operation, nothing contracted:
 *   out = m == 0 ? k : m == 1 ? e : k + m * (e - k)          the select-then-lerp of slh_ddpm_edit_blend (csrc/step_common.h)
 * A NaN in e does not reach a pixel with m = 0, nor a NaN in keep a pixel with m = 1.  Mask values outside [0, 1] are the caller's error.
 * ptrs[6]: 0 e        the latent the step just produced   [nb][chw]
 *          1 keep     the base chain's latent after the same step   [nb][chw]
 *          2 mask     fp32 [nb][hw] in [0,1], one value per latent pixel, shared by the channels (index b*hw + i % hw)
 *          3 out      [nb][chw]; may alias e
 *          4, 5 in_bf16, in2_bf16   optional bf16 [nb][chw]: the two halves of the CFG pair's sample input
 * dims[4]: 0 nb, 1 chw, 2 hw (chw % hw == 0), 3 dtype (0: e/keep/out bf16; 1: fp32)
 * coef[1]: 0 s_next (dtype 1 only; not read for dtype 0)
 * dtype 1: out is fp32 and the bf16 copies are round-to-nearest-even(out * s_next), as slh_sigma_step writes them.
 * dtype 0: out is the round-to-nearest-even bf16 of the fp32 result (m = 0: keep's bits, m = 1: e's bits); the copies are out's bits.
 * Every thread reads all it needs before it writes, so out may alias e.  16-byte accesses where every pointer, chw and hw allow them
 * (a multiple of 4 elements for dtype 1, of 8 for dtype 0), one element per thread otherwise; any chw >= 1 works.
 * Refused before the launch (slh_last_error): a null e / keep / mask / out; an fp32 pointer that is not 4-byte or a bf16 pointer that
 * is not 2-byte aligned; nb < 1, chw < 1, hw < 1, chw % hw != 0; dtype out of range; a non-finite s_next with dtype 1; keep or mask
 * overlapping an output. */
int slh_latent_blend(const void* const* ptrs, const int32_t* dims, const float* coef, slh_stream_t stream);

/* Prompt-direction sampling (csrc/eps_direction.hip, docs/SAMPLING.md, "Prompt-direction sampling"): one UNet pass has produced, next
 * to the text row t, the rows e+_k, e-_k of K <= 3 prompt pairs on the same latent.  With d_k = e+_k - e-_k (one fp32 subtraction of
 * the widened bf16 values) and key(d) = the upper 16 bits of the fp32 bit pattern of |d|, an integer:
 *
 * slh_direction_threshold: thr[b][k][ch] = tau, the n_keep[k]-th largest key(d_k) among the hw pixels of channel ch of sample b, counted
 * with multiplicity.  One workgroup per (b, k, ch), a radix select in two 8-bit passes with integer LDS counters: exact, the same in
 * every run.  Any hw >= 1.
 * ptrs[7]: 0..2 pos[k], 3..5 neg[k]   bf16 [nb][chw], the first K of each are read
 *          6 thr                       int32 [nb][K][chw / hw], written
 * dims[7]: 0 nb, 1 chw, 2 hw (chw % hw == 0), 3 K (1..3), 4..6 n_keep[k] (1..hw)
 * coef:    not read (may be NULL)
 *
 * slh_eps_direction: the guided text row, per element in fp32, one rounding per operation, nothing contracted:
 *   acc = t;   for k ascending with c[k] != 0:  d = e+_k - e-_k;  if thr is given and key(d) < thr[b][k][ch] the term is skipped;
 *   otherwise p = c[k] * d, acc = acc + p;   out = round-to-nearest-even bf16 of acc.
 * A term with c[k] == 0 is skipped, not multiplied: its rows are not read and may hold NaN.  With every c[k] == 0 out has t's bits.
 * Every element with key(d) == tau is kept, so at least n_keep elements of a group are; without thr every element is, which is what
 * n_keep = hw gives bit for bit.
 * ptrs[9]: 0 t      bf16 [nb][chw]
 *          1 out    bf16 [nb][chw]; must not overlap any input
 *          2..4 pos[k], 5..7 neg[k]   bf16 [nb][chw], the first K of each
 *          8 thr    optional int32 [nb][K][chw / hw], as slh_direction_threshold writes it
 * dims[4]: 0 nb, 1 chw, 2 hw (chw % hw == 0), 3 K (1..3)
 * coef[3]: c[k]
 * 16-byte accesses where every pointer, chw and hw allow them (multiples of 8 elements), one element per thread otherwise.
 * Both are never recorded in a program: no opcode, no descriptor struct; three host arrays, as slh_sigma_step.  Refused before the
 * launch (slh_last_error): a null required pointer; a bf16 pointer that is not 2-byte or an int32 pointer that is not 4-byte aligned;
 * nb < 1, chw < 1, hw < 1, chw % hw != 0; K outside 1..3; n_keep[k] outside 1..hw; a non-finite c[k]; an output overlapping an input. */
int slh_direction_threshold(const void* const* ptrs, const int32_t* dims, const float* coef, slh_stream_t stream);
int slh_eps_direction(const void* const* ptrs, const int32_t* dims, const float* coef, slh_stream_t stream);

/* slh_eps_direction with SEGA's momentum term (docs/SAMPLING.md, "Prompt-direction sampling"): nu, an fp32 state per element, carries
 * the guidance the directions gave on the earlier passes into this one, and is updated from what they give now.  Per element, fp32,
 * one rounding per operation, nothing contracted; keep is slh_eps_direction's rule (key(d) >= thr[b][k][ch], every tie kept, all kept
 * without thr):
 *   acc = t;  g = +0
 *   for k ascending with c[k] != 0, where kept:   d = e+_k - e-_k;  p = c[k] * d;  acc = acc + p;  g = g + p
 *   q = s_m * nu;   acc = acc + q;   gm = g + q
 *   a = beta * nu;  b = omb * gm;    nu' = a + b
 *   out = round-to-nearest-even bf16 of acc;   mom_out = nu'
 * A term with c[k] == 0 is skipped as in slh_eps_direction: its rows are not read.  s_m == 0 is refused: momentum off is
 * slh_eps_direction, whose acc keeps the sign of a -0 that an added +0 would lose.
 * ptrs[11]: 0..8 as slh_eps_direction (t, out, pos[3], neg[3], optional thr)
 *           9  mom_in   fp32 [nb][chw], nu
 *           10 mom_out  fp32 [nb][chw], nu'; may be mom_in itself (every thread reads all it needs before it writes)
 * dims[4]:  as slh_eps_direction
 * coef[6]:  0..2 c[k], 3 s_m, 4 beta, 5 omb (the caller's 1 - beta, formed in double and rounded once)
 * 16-byte accesses where every pointer, chw and hw allow them (eight elements per thread: one bf16 vector, two fp32 ones), one element
 * per thread otherwise; any chw >= 1.  Never recorded in a program.  Refused before the launch: everything slh_eps_direction refuses; a
 * null mom_in / mom_out, or one that is not 4-byte aligned; a non-finite s_m, beta or omb; s_m == 0; mom_out or out overlapping any
 * input (mom_out == mom_in excepted); out overlapping mom_out. */
int slh_eps_direction_momentum(const void* const* ptrs, const int32_t* dims, const float* coef, slh_stream_t stream);

/* The edit step of a localised edit: e = mu + resid exactly as slh_ddpm_edit_step mode 1 forms it (one piece of code), then, with
 * k = keep[i] and m = mask[b*hw + i % hw] (one mask value per latent pixel, shared by the channels),
 *   out = m == 0 ? k : m == 1 ? e : k + m * (e - k)          fp32, one rounding per operation, no contraction.
 * keep is the latent the inversion's own chain had after this step: where the mask is 0 the edit stays on the inversion's latents
 * bit for bit, and where e == keep (an edit at scale 0) out == keep under any mask.  Mask values outside [0, 1] are the caller's
 * error.  keep and mask must not overlap out. */
typedef struct slh_ddpm_edit_blend_desc {
    const void* eps;         /* bf16 [2*nb][chw], uncond half first */
    const void* eps_text;    /* optional, as slh_cfg_ddim_desc */
    const float* x;          /* fp32 [nb][chw] master latent x_t */
    const float* resid;      /* fp32 [nb][chw], read */
    const float* keep;       /* fp32 [nb][chw]: the inversion's latent after this step */
    const float* mask;       /* fp32 [nb][hw] in [0, 1]; 1 = edit */
    float* out;              /* fp32 x_{t-1}; may alias x */
    void* out_bf16; void* out2_bf16;   /* optional bf16 copies of out */
    int32_t nb, chw, hw;     /* chw % hw == 0 */
    float guidance;
    float c_sqrt_beta_t, c_inv_sqrt_alpha_t, c_sqrt_alpha_t, c_sqrt_alpha_prev, c_dir;   /* as slh_ddpm_edit_desc */
    int32_t v_prediction;
} slh_ddpm_edit_blend_desc;
int slh_ddpm_edit_blend(const slh_ddpm_edit_blend_desc* d, slh_stream_t stream);

/* One step of the second-order residual noise space (csrc/edit_step2.hip, docs/EDIT.md, "Second-order noise space"): the mean of
 * slh_ddpm_edit_step with the multistep correction of SDE-DPM-Solver++ 2M added, its mode branch, and with keep / mask the blend of
 * slh_ddpm_edit_blend, in one launch.  Never recorded in a program: no opcode, no descriptor struct; three host arrays, as
 * slh_sigma_step.  Per element, with u, t the bf16 epsilon halves and x the master latent, fp32 throughout, one rounding per
 * operation, nothing contracted:
 *   e    = u + g (t - u)
 *   x0h, mu_1                            the predicted clean sample and the mean, by the device code slh_ddpm_edit_step forms them with
 *   with x0_prev:  d = x0h - x0_prev;  p = c_corr * d;  mu = mu_1 + p        without: mu = mu_1 (the term is skipped, not multiplied)
 *   mode 0 (invert): resid = target - mu is written;   mode 1 (edit): resid is read;   both: o = mu + resid
 *   with keep / mask (k, m = mask[b*hw + i % hw]):  o = m == 0 ? k : m == 1 ? o : k + m * (o - k)
 *   out = o;  x0_out = x0h;  out_bf16 = out2_bf16 = round-to-nearest-even(o)
 * Without x0_prev, out, resid and the bf16 copies are those of slh_ddpm_edit_step (with keep / mask: slh_ddpm_edit_blend) bit for bit.
 * ptrs[12]: 0 eps       bf16 [2*nb][chw], unconditional half first
 *           1 eps_text  optional, as slh_cfg_ddim_desc
 *           2 x         fp32 [nb][chw]
 *           3 x0_prev   optional fp32 [nb][chw]: x0h of the same chain's step before; NULL: first order
 *           4 target    fp32 [nb][chw], mode 0 only (mode 1: not read, may be NULL)
 *           5 resid     fp32 [nb][chw]; mode 0: written, mode 1: read
 *           6 keep      optional fp32 [nb][chw]: the inversion's latent after this step (with mask)
 *           7 mask      optional fp32 [nb][hw] in [0, 1], one value per latent pixel (with keep; mode 1 only)
 *           8 out       fp32 [nb][chw]; may be x itself
 *           9 x0_out    optional fp32 [nb][chw]; may be x0_prev itself
 *           10, 11 out_bf16, out2_bf16   optional bf16 [nb][chw]: the two halves of the CFG pair's sample input
 * dims[5]:  0 nb, 1 chw, 2 hw (chw % hw == 0), 3 mode (0 invert, 1 edit), 4 v_prediction (0, 1)
 * coef[7]:  0 guidance, 1 c_sqrt_beta_t, 2 c_inv_sqrt_alpha_t, 3 c_sqrt_alpha_t, 4 c_sqrt_alpha_prev, 5 c_dir (as slh_ddpm_edit_desc),
 *           6 c_corr = B h / (2 h_old), B = c_sqrt_alpha_prev - c_dir c_sqrt_alpha_t / c_sqrt_beta_t (read only with x0_prev)
 * Every thread reads all it needs before it writes, which is what makes the two aliases legal.  16-byte fp32 / 8-byte bf16 accesses
 * (four elements per thread) where every pointer, chw and hw allow them, one element per thread otherwise; any chw >= 1 works.
 * Refused before the launch (slh_last_error): a null ptrs / dims / coef, eps, x, resid or out; an fp32 pointer that is not 4-byte or a
 * bf16 pointer that is not 2-byte aligned; nb < 1, chw < 1, hw < 1, chw % hw != 0; mode or v_prediction out of range; keep without
 * mask or mask without keep; mode 0 without target, or with a mask; x0_prev with a c_corr that is zero or not finite; an output
 * overlapping an input (keep and mask included) other than out == x and x0_out == x0_prev; two outputs overlapping. */
int slh_edit_step2(const void* const* ptrs, const int32_t* dims, const float* coef, slh_stream_t stream);

/* Where two epsilon predictions differ, per latent pixel: with e = u + guidance * (t - u) of each pair (fp32, no contraction),
 *   out[b][p] = sum over c = 0 .. chw/hw - 1, ascending, of |e_a - e_b| at (b, c, p).
 * One thread per pixel, a fixed order and no atomics: bit-reproducible. */
typedef struct slh_eps_absdiff_desc {
    const void* eps_a;       /* bf16 [2*nb][chw], uncond half first */
    const void* eps_a_text;  /* optional: the text half [nb][chw] where it is not stored right after the uncond half */
    const void* eps_b; const void* eps_b_text;   /* likewise */
    float* out;              /* fp32 [nb][hw] */
    int32_t nb, chw, hw;     /* chw % hw == 0 */
    float guidance;
} slh_eps_absdiff_desc;
int slh_eps_absdiff(const slh_eps_absdiff_desc* d, slh_stream_t stream);

/* One attention map per sample from a cross-attention layer's q and k and a weight per key (SliderEditor.word_map):
 *   term[b][i] = coef * sum_{h < H} sum_{j < Tk} wt[b][j] * P[b0 + b, h, i, j],   P = softmax_j(scale * q_i . k_j) over the Tk keys,
 *   out = term (accumulate 0) or out + term (accumulate 1).
 * bf16 inputs, fp32 everywhere else; the softmax keeps a running maximum, no probability, logit or per-head share goes to global
 * memory; the heads are added in ascending order by the one workgroup that owns the query row, with no atomics and no wait on
 * another workgroup: bit-reproducible.  Several layers accumulate into one map by stream order.
 * D % 8 == 0 and 8 <= D <= 192, 1 <= Tk <= 128, Tq >= 1, H >= 1, b0 + nb <= B, ldq and ldk multiples of 8 and >= H * D, q and k
 * 16-byte aligned; anything else is refused before the launch. */
typedef struct slh_xattn_map_desc {
    const void* q;        /* [B][Tq][ldq] bf16, head h at columns [h*D, (h+1)*D) */
    const void* k;        /* [B][Tk][ldk] bf16, same head layout (a column view of attn2_kv_all is the normal case: ldk >> H*D) */
    const float* wt;      /* [nb][Tk] fp32 key weights, one row per collected sample */
    float* out;           /* [nb][Tq] fp32 */
    int32_t B, b0, nb;    /* samples b0 .. b0+nb-1 of the batch are collected (the text half of a CFG pair: b0 = nb = B/2) */
    int32_t H, D, Tq, Tk, ldq, ldk;
    float scale;          /* D^-0.5 */
    float coef;           /* 1 / (H * layers of this level): the last launch of a level leaves the mean */
    int32_t accumulate;   /* 0: out = term; 1: out = out + term */
} slh_xattn_map_desc;
int slh_xattn_map(const slh_xattn_map_desc* d, slh_stream_t stream);

/* guidance loss (prompt_util.py:108-148): loss = mean((target - (neutral +- gs*(positive-uncond)))^2);
 * writes loss (fp32 scalar, atomically accumulated: zero it first) and d(loss)/d(target) (bf16). */
typedef struct slh_loss_desc {
    const void* target; const void* positive; const void* neutral; const void* uncond;
    float* loss; void* dtarget;
    float* dtarget_pix;      /* optional: the same gradient as fp32 pixel-major [nb*hw][nch] (backward input) */
    int32_t n; float guidance; int32_t erase;
    int32_t hw, nch;         /* n = nb * nch * hw, NCHW order */
} slh_loss_desc;
int slh_guidance_loss(const slh_loss_desc* d, slh_stream_t stream);

/* LoRA weight gradients: out (fp32, +=) = scale * sum_m Z[m][c] * V[m][r]; Z bf16 with the same addressing
 * as slh_gemm's A (mode 1: column index = tap*Cin + c), V fp32 [M][ldv].  R is 4 or 12. */
typedef struct slh_wgrad_desc {
    const void* z0; const void* z1;
    const float* v;
    float* out;              /* dense: [C][ldo]; conv: [9][C][ldo] */
    const float* scale;      /* device scalar */
    int32_t ldz0, ldz1, c0, c1;
    int32_t mode, batch, hs, ws, src_xform, stride, ho, wo;
    int32_t M, R, ldv, ldo;
    int32_t out_rmajor;      /* 1: out is [R][ldo] (down-weight layout), 0: [C][ldo] (up-weight layout) */
    int32_t vgroup_cols;     /* >0: channel c uses V columns 4*(c/vgroup_cols).. (fused q/k/v up grads).  Contract (refused otherwise): a
                                multiple of 8 (the offset is taken once per 8-channel chunk) that divides c0 + c1, and R == 4 */
    float* slabs;            /* fixed-order reduction over the M splits (bit-reproducible gradients): slh_lora_wgrad_single_blocks(d)
                                slabs of 256 * R floats (contents irrelevant) ... */
    void* tickets;           /* ... and as many uint32 arrival tickets, zeroed once (the last arriver re-arms them).  Both NULL:
                                fp32 atomics (commit in arrival order).  Inside a batch: any non-NULL slabs selects the slab
                                geometry for slh_lora_wgrad_blocks; the workspace itself is the batch's */
} slh_wgrad_desc;
int slh_lora_wgrad(const slh_wgrad_desc* d, slh_stream_t stream);
int slh_lora_wgrad_single_blocks(const slh_wgrad_desc* d);
/* Launch geometry of d's problem as the library's one geometry function gives it, out4 = {gx (column blocks of 256 channels), splits
 * (of M), taps (9 in conv mode), rows_per_block}, for kind 0 (fp32 atomics, single or batched), 1 (single launch with slabs) or 2 (a
 * problem of a batch with slabs).  Shape fields only, no device needed.  gx * splits * taps is what slh_lora_wgrad_blocks (kind 2 / 0) and
 * slh_lora_wgrad_single_blocks (kind 1) return.  0, or -1 + slh_last_error(). */
int slh_lora_wgrad_geometry(const slh_wgrad_desc* d, int kind, int32_t* out4);

/* Batched launches: n independent problems of one kind in ONE launch (the backward of a UNet pass has ~380 rank-4
 * weight-gradient reductions and ~210 head transposes of forward activations, each far too small to fill the chip).
 * table is a DEVICE array of n descriptors of the kind's own type, prefix a DEVICE int32[n + 1] running sum of the
 * workgroups each problem needs (slh_*_blocks(descriptor), which also validates the descriptor: -1 + slh_last_error()),
 * total = prefix[n].  A workgroup finds its problem by bisection of prefix. */
typedef struct slh_batch_desc {
    const void* table; const int32_t* prefix;
    int32_t n, total;
    int32_t arg;             /* slh_lora_wgrad_batch: R (4 or 12), the same for every problem of the batch */
    int32_t pad_;
    void* slabs;             /* slh_lora_wgrad_batch: `total` slabs of 256 * R floats + ... */
    void* tickets;           /* ... `total` uint32 tickets (zeroed once): fixed-order reduction, every problem's descriptor built
                                with a non-NULL slabs; both NULL: fp32 atomics.  Contract: prefix takes each problem's geometry
                                from its descriptor's slabs (slh_lora_wgrad_blocks), the kernel takes it from the batch's, and the
                                table is device memory the launch cannot read back: ALL descriptors of a batch are built with
                                slabs, or none, and the batch carries slabs exactly when they are - workgroups index past their
                                problem otherwise.  lib.batch_table refuses a mixed table and lib.call / Program.add a batch whose
                                slabs disagree with its table */
} slh_batch_desc;
int slh_lora_wgrad_blocks(const slh_wgrad_desc* d);
int slh_lora_wgrad_batch(const slh_batch_desc* d, slh_stream_t stream);
int slh_transpose_heads_blocks(const slh_transpose_desc* d);
int slh_transpose_heads_batch(const slh_batch_desc* d, slh_stream_t stream);

/* out[i] = idx[i] < 0 ? 0 : src[idx[i]] on 16-bit elements (the k-major copies of the adapters' up matrices that the fused
 * backward-data products stream as their third operand: rebuilt from the live parameters at the head of every backward). */
typedef struct slh_gather16_desc { const void* src; const int32_t* idx; void* out; int64_t n; } slh_gather16_desc;
int slh_gather16(const slh_gather16_desc* d, slh_stream_t stream);

/* The adapter side of a LayerNorm folded into an adapter-carrying product (slh_gemm_desc.ln_lora_*): for every item
 *   a_out[r][k] = bf16(a[r][k] * gamma[k]),  s_out[r] = sum_k float(a_out[r][k]),  c_out[r] = sum_k a[r][k] * beta[k]
 * from the LIVE adapter parameters; one launch at the head of a pass covers every folded module (items = a device array). */
typedef struct slh_lora_lnfold_item {
    const void* a; const void* gamma; const void* beta;   /* bf16 [rows][K], [K], [K] */
    void* a_out; float* s_out; float* c_out;               /* bf16 [rows][K], fp32 [rows], fp32 [rows] */
    int32_t rows, K;                                       /* K % 8 == 0.  Contract: rows <= 16 - the grid is 16 rows per item, further
                                                              rows would be silently left out; the items live in device memory, so
                                                              whoever builds them checks (lib.lnfold_item) */
} slh_lora_lnfold_item;
typedef struct slh_lora_lnfold_desc { const slh_lora_lnfold_item* items; int32_t n; int32_t pad_; } slh_lora_lnfold_desc;
int slh_lora_ln_fold(const slh_lora_lnfold_desc* d, slh_stream_t stream);

/* Adapters folded into the frozen weights (inference: the adapters are constants of a denoise loop, so any number of sliders of
 * any rank become W' = W + sum_i s_i (alpha_i / r_i) B_i A_i once, and the adapter-free programs run on W').  For every item
 *   out[n][k] = bf16( float(base[n][k]) + sum_{r < R} (c[r] * u[n - n0][r]) * d[r][k] ),   n0 <= n < n0 + rows,
 * on a STORED matrix: base is a pristine copy in the layout of out (w_layout as slh_gemm_desc.w_layout: 1 tile-packed, rows past N
 * are never written; 0 row-major with row stride ld).  The sum is one fp32 fma chain per element, r ascending from 0.  The host
 * concatenates all sliders' factors along R and keeps scale * alpha / rank in c: new scales rewrite R floats.  R is any value >= 1.
 * gamma != NULL: the item writes the LayerNorm-folded copy instead (weights.py fold_layernorm, on the merged matrix):
 *   out[n][k] = bf16( (base + delta)[n][k] * gamma[k] ),  lns[n] = sum_k float(out[n][k]),
 *   lnb[n] = bias[n] + sum_k float(bf16((base + delta)[n][k])) * beta[k]      (fp32, fixed order; bias may be NULL)
 * One workgroup owns 64 rows of an item and walks K: no atomics, bit-reproducible.  items is a DEVICE array, prefix a DEVICE
 * int32[n + 1] running sum of slh_lora_merge_blocks(item) (which validates a HOST copy of the item: -1 + slh_last_error()),
 * total = prefix[n]; one launch covers every item.  Items of one launch must not write the same rows of the same tensor. */
typedef struct slh_lora_merge_item {
    const void* base; void* out;                              /* bf16 stored matrices (first element of the whole matrix) */
    const float* u; const float* d; const float* c;           /* fp32 [rows][ldu], [R][ldd], [R] */
    const void* gamma; const void* beta; const void* bias;    /* bf16 [K], [K], [N]; gamma NULL: plain merge */
    float* lns; float* lnb;                                   /* fp32 [N], written at rows n0 .. n0 + rows (folded copy only) */
    int32_t n0, rows, N, K;                                   /* K % 8 == 0 (tile-packed: % 64) */
    int32_t R, ldu, ldd, ld;                                  /* ldu >= R; ldd >= K, % 4 == 0; ld: row-major only, >= K, % 8 == 0 */
    int32_t w_layout, pad_;
} slh_lora_merge_item;
typedef struct slh_lora_merge_desc { const slh_lora_merge_item* items; const int32_t* prefix; int32_t n, total; } slh_lora_merge_desc;
int slh_lora_merge_blocks(const slh_lora_merge_item* item);
int slh_lora_merge(const slh_lora_merge_desc* d, slh_stream_t stream);

/* Backward-data term of a 3x3 LoRA down conv (lora.py:82-87): gx[i][c] (+)= scale * sum_{tap,r} U[o][r] *
 * A[r][tap][c] for the output pixels o with o*stride + tap - 1 = i.  U fp32 [batch*ho*wo][ldu], A = lora_down
 * as stored [4][9*cin], gx bf16 pixel-major image of hl x wl. */
typedef struct slh_lora_cdgrad_desc {
    const float* u; const void* a_down; const float* scale; void* gx;
    int32_t batch, hl, wl, ho, wo, stride, cin, ldu, ldgx, accumulate;
} slh_lora_cdgrad_desc;
int slh_lora_conv_dgrad(const slh_lora_cdgrad_desc* d, slh_stream_t stream);

/* LoRA gradients of one ResnetBlock2D.time_emb_proj for one sample: g = d(loss)/d(temb projection) [C] fp32
 * (column sums of the conv1 output gradient), t = that layer's lora_down(silu(emb)) [4], up [C][4], emb [ted]
 * bf16; accumulates d_up [C][4] and d_down [4][ted] (fp32). */
typedef struct slh_temb_lora_bwd_desc {
    const float* g; const float* t; const void* up; const void* emb; float* d_up; float* d_down;
    const float* scale;
    int32_t C, ted;
} slh_temb_lora_bwd_desc;
int slh_temb_lora_bwd(const slh_temb_lora_bwd_desc* d, slh_stream_t stream);

/* flat AdamW over the packed LoRA parameter buffer (bf16 params and moments, torch.optim.AdamW op order
 * and bf16 rounding points; train_util.py:362-363, train_lora_xl.py:346). grads fp32.
 * f32_state = 1 (train.precision: float32 - the reference's weight_dtype applied to the network, train_lora_xl.py:60-61, 84-90): param,
 * exp_avg and exp_avg_sq are fp32 arrays updated with the op order of torch.optim.AdamW on fp32 CUDA tensors (one fp32 rounding per
 * foreach op), the gradient is used unrounded, and param_lo - the bf16 copy every kernel of the UNet pass reads - receives the
 * rounded new parameters in the same launch. */
typedef struct slh_adamw_desc {
    void* param; void* exp_avg; void* exp_avg_sq; const float* grad;
    int64_t n;
    double lr, beta1, beta2, eps, weight_decay;  /* python floats of torch.optim.AdamW */
    int32_t step;            /* 1-based */
    float grad_scale;        /* multiply grads first (1/world_size after all-reduce) */
    void* param_lo;          /* f32_state only: bf16 [n], written */
    int32_t f32_state;       /* 0: bf16 state (default), 1: fp32 state + param_lo */
    int32_t pad_;
} slh_adamw_desc;
int slh_adamw(const slh_adamw_desc* d, slh_stream_t stream);

/* flat Lion over the packed LoRA parameter buffer (train.optimizer "lion": train_util.py:365-368 -> lion_pytorch==0.1.2,
 * requirements.txt:5).  One bf16 moment; op order and bf16 rounding points of that package's update_fn:
 *   p.mul_(1 - lr*wd); update = sign(exp_avg*b1 + (1-b1)*g); p.add_(update, alpha=-lr); exp_avg = exp_avg*b2 + (1-b2)*g */
typedef struct slh_lion_desc {
    void* param; void* exp_avg; const float* grad;
    int64_t n;
    double lr, beta1, beta2, weight_decay;
    float grad_scale;        /* multiply grads first (1/world_size after all-reduce) */
    int32_t pad_;
} slh_lion_desc;
int slh_lion(const slh_lion_desc* d, slh_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Image sliders: AutoencoderKL encoder + posterior sample + add_noise in fp32 on the GPU.
 * Replaces trainscripts/imagesliders/train_util.py:200-235 `get_noisy_image` (vae.encode(...).latent_dist.sample()
 * * scaling_factor -> scheduler.add_noise); the VAE arithmetic itself is diffusers' AutoencoderKL.encode.
 * Activations are pixel-major fp32 [B*H*W][C]; 3x3 weights are [Cout][ky][kx][Cin] fp32.
 * ---------------------------------------------------------------------------------------------- */
typedef struct slh_sgemm_desc {
    const void* x;          /* [M][ldx] fp32 (mode 0) or the [batch*hs*ws][ldx] source image of an implicit 3x3 GEMM (mode 1) */
    const void* w;          /* [N][ldw] fp32 */
    const void* bias;       /* [N] (or [M] if bias_per_row) fp32, may be NULL */
    const void* residual;   /* [M][ldr] fp32, may be NULL */
    void* c;                /* [M][ldc] fp32 */
    int32_t ldx, ldw, ldr, ldc;
    int32_t M, N, K;
    int32_t mode;           /* 0 dense, 1 implicit 3x3 (K = 9*cin) */
    int32_t cin, batch, hs, ws, ho, wo, stride, pad;   /* stride 1 | 2; pad 1: one zero row / column on every side; pad 0: one below
                               and to the right only (Downsample2D(padding=0) with stride 2).  The output size is checked:
                               ho = (he + pad - 2) / stride + 1 with he = hs (2*hs with upsample), wo likewise; M = batch*ho*wo */
    int32_t bias_per_row;
    float alpha;            /* C = alpha * (X W^T) + bias + residual */
    int32_t upsample;       /* conv, stride 1 only: 1 = the source is read through a nearest-2x upsample (Upsample2D), ho = 2*hs
                               with pad 1.  Must be 0 in mode 0 */
    int32_t split_bf16;     /* 0: exact fp32 products (v_mfma_f32_32x32x2_f32).  1: every operand split into two bf16 halves,
                               x.w ~= hi.hi + hi.lo + lo.hi on the bf16 matrix pipe with fp32 accumulation (16 mantissa bits per
                               operand, ~5x fewer matrix cycles); needs K % 32 == 0 (and Cin % 32 == 0), else exact.  Any other
                               value is refused */
} slh_sgemm_desc;
int slh_sgemm(const slh_sgemm_desc* d, slh_stream_t stream);
/* the kernel form slh_sgemm would launch for d (its own selection runs, nothing is launched, no device needed); negative, with
 * slh_last_error set, for a descriptor slh_sgemm refuses */
enum { SLH_SGEMM_EXACT = 0, SLH_SGEMM_SPLIT64 = 1, SLH_SGEMM_SPLIT128 = 2 };   /* sgemm_kernel, sgemm_bf16x3_kernel<64>, <128> */
int slh_sgemm_form(const slh_sgemm_desc* d);

typedef struct slh_gn32_desc {
    const void* x; const void* gamma; const void* beta;   /* fp32 */
    float* stats;           /* [batch][groups][2] fp32: (mean, rstd), written by slh_gn32_stats */
    void* y;                /* [batch*hw][ldy] fp32 */
    int32_t ldx, ldy, C, batch, hw, groups;
    float eps;
    int32_t act;            /* 0 none, 1 SiLU */
    float* partial;         /* slh_gn32_stats: [batch][R + L][groups][2] fp32 scratch, R = slh_gn32_row_blocks(hw),
                               L = slh_gn_clusters(R) (see slh_gn_desc) */
    uint32_t* ticket;       /* slh_gn32_stats: [batch][1 + L] arrival counters, zero before the launch */
} slh_gn32_desc;
int slh_gn32_stats(const slh_gn32_desc* d, slh_stream_t stream);
int slh_gn32_apply(const slh_gn32_desc* d, slh_stream_t stream);
int slh_gn32_row_blocks(int hw);

typedef struct slh_softmax32_desc { float* x; int64_t ld; int32_t rows, cols; } slh_softmax32_desc;   /* in place */
int slh_softmax32(const slh_softmax32_desc* d, slh_stream_t stream);

typedef struct slh_vae_conv_desc {
    const void* x;          /* conv_in: image [batch][h*wd][3] fp32; moments: [batch*h*wd][cin] fp32 */
    const void* w; const void* bias;      /* conv_in: [cout][3][3][3]; moments: conv_out [8][3][3][cin], [8] */
    const void* qw; const void* qb;       /* moments only: quant_conv [8][8], [8] */
    void* y;                /* conv_in: [batch*h*wd][cout]; moments: [batch*h*wd][8] = mean | logvar */
    int32_t batch, h, wd, cin, cout;
    float inv_scaling;      /* post_quant only: 1 / vae.config.scaling_factor */
} slh_vae_conv_desc;
int slh_vae_conv_in(const slh_vae_conv_desc* d, slh_stream_t stream);    /* cin 3 (encoder) or 4 (decoder conv_in) */
int slh_vae_moments(const slh_vae_conv_desc* d, slh_stream_t stream);
/* decoder input: x = latents NCHW [batch][4][h*wd] (fp32, or bf16 if cin == 1) -> * inv_scaling -> post_quant_conv (qw [4][4],
 * qb [4]) -> y pixel-major [batch*h*wd][4] fp32.  eval-scripts/generate_images_sd1.py:166-168. */
int slh_vae_post_quant(const slh_vae_conv_desc* d, slh_stream_t stream);

typedef struct slh_vae_sample_desc {
    const float* moments;       /* [batch*hw][8] */
    const float* post_noise;    /* [batch][4][hw] NCHW: the draw of DiagonalGaussianDistribution.sample */
    const float* noise;         /* [batch][4][hw] NCHW: the diffusion noise of add_noise */
    float* latent_f32;          /* optional: scaling_factor * sample, NCHW */
    float* noisy_f32;           /* optional: add_noise result, NCHW fp32 */
    void* noisy_bf16;           /* optional: the same in bf16 (the UNet's input dtype) */
    int32_t batch, hw;
    float scaling, sqrt_alpha, sqrt_one_minus_alpha;
    int32_t pad_;
} slh_vae_sample_desc;
int slh_vae_sample(const slh_vae_sample_desc* d, slh_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * program executor: a whole UNet forward / backward is a flat command buffer built once by the host
 * planner (sliders_amd/plan.py) and replayed with ONE call.  Record layout: {int32 opcode; int32
 * nbytes; desc bytes (8-byte aligned)}.
 * ---------------------------------------------------------------------------------------------- */
enum {
    SLH_OP_GEMM = 1, SLH_OP_SKINNY = 2, SLH_OP_GEMV = 3, SLH_OP_GN_STATS = 4, SLH_OP_GN_APPLY = 5,
    SLH_OP_LAYERNORM = 6, SLH_OP_ATTN_FWD = 7, SLH_OP_TRANSPOSE_HEADS = 8, SLH_OP_TEMBED = 9,
    SLH_OP_CONV_IN = 10, SLH_OP_ELEMENTWISE = 11, SLH_OP_CFG_DDIM = 12, SLH_OP_LOSS = 13,
    SLH_OP_WGRAD = 14, SLH_OP_ADAMW = 15, SLH_OP_GN_BWD_STATS = 16, SLH_OP_GN_BWD_APPLY = 17,
    SLH_OP_LAYERNORM_BWD = 18, SLH_OP_ATTN_BWD = 19, SLH_OP_MEMSET = 20, SLH_OP_LORA_CONV_DGRAD = 21,
    SLH_OP_TEMB_LORA_BWD = 22, SLH_OP_SGEMM = 23, SLH_OP_GN32_STATS = 24, SLH_OP_GN32_APPLY = 25, SLH_OP_SOFTMAX32 = 26,
    SLH_OP_VAE_CONV_IN = 27, SLH_OP_VAE_MOMENTS = 28, SLH_OP_VAE_SAMPLE = 29, SLH_OP_VAE_POST_QUANT = 30, SLH_OP_LION = 31,
    SLH_OP_WGRAD_BATCH = 32, SLH_OP_TRANSPOSE_BATCH = 33, SLH_OP_GATHER16 = 34, SLH_OP_GN_FUSED = 35,
    SLH_OP_LORA_LN_FOLD = 36,     /* 37 was SLH_OP_PREFETCH (side-stream weight touch: measured slower, removed in round 5) */
    SLH_OP_LORA_MERGE = 38, SLH_OP_DDPM_EDIT = 39, SLH_OP_DDPM_EDIT_BLEND = 40, SLH_OP_EPS_ABSDIFF = 41,
    SLH_OP_XATTN_MAP = 42
};
/* SLH_OP_MEMSET: byte fill by a kernel of this library (not hipMemsetAsync: a captured memset node is a runtime blit whose
 * replays were observed to go wrong on the legacy default stream - see the executor's comment) */
typedef struct slh_memset_desc { void* ptr; int64_t nbytes; int32_t value; int32_t pad; } slh_memset_desc;
int slh_memset(const slh_memset_desc* d, slh_stream_t stream);   /* nbytes <= 0: nothing is launched, 0 */
int slh_run_program(const void* program, int64_t nbytes, slh_stream_t stream);
/* hipGraph replay of a command buffer: capture records the launches slh_run_program would issue (on a private stream;
 * nothing executes), launch re-submits them as one graph.  The buffer must be static between replays (descriptors are baked
 * into the kernel arguments); everything the reference's loop changes per step (latents, timestep, adapter scale and
 * weights - train_util.py:220-260) is read through device pointers and may change freely.  Replaces the ~1.2k Python
 * op dispatches of one diffusers UNet forward with one submission. */
int slh_graph_capture(const void* program, int64_t nbytes, void** out_graph);
int slh_graph_launch(void* graph, slh_stream_t stream);
int slh_graph_destroy(void* graph);
/* The executor's op table, one row per SLH_OP_*, for binding self-checks: row `index` gives the opcode, the name of its entry point
 * and the sizeof() of the descriptor that entry point takes (any out pointer may be NULL).  Returns the number of rows; an index
 * outside [0, rows) writes nothing.  The order of the rows carries no meaning: a binding keys its check by opcode. */
int slh_op_info(int index, int32_t* opcode, const char** entry, int32_t* desc_size);

#ifdef __cplusplus
}
#endif
#endif
