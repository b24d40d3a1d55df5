// Host side of the slh_gemm dispatch: the decoded tile, and what gemm.hip (decoder, the rule, ring / ping-pong launch), gemm5.hip and
// gemm7.hip (their families' parts of the rule, their launches) share.  No device code.
#pragma once
#include "common.h"
#include "../../include/sliders_hip.h"

enum GemmFamily { GEMM_RING, GEMM_PINGPONG, GEMM_64X160, GEMM_FOURWAVE };      // gemm.hip, gemm8p.hip, gemm5.hip, gemm7.hip

// slh_gemm_desc.tile taken apart (gemm_tile_decode, gemm.hip: the one place that reads the code's bits and knows which codes exist).
// For an all-zero code it holds the heuristic's pick.
struct GemmTile {
    GemmFamily family;
    int slots;             // bits 8-11 as coded: ring 0 | 2 (double buffer), 3, 4; 64 x 160: 4 | 5; gemm7.hip: S half K tiles
    int mi, ni, wm;        // ring / ping-pong: MI, NI, WM (waves along M / 2).  gemm7.hip: mi = XB, ni = WB.  64 x 160: 2, 5
    int splitk;            // bits 16-19 as coded (0 | 1: none)
    int bm, bn;            // block tile
    int threads;           // per workgroup
};
int gemm_tile_decode(const slh_gemm_desc* d, GemmTile* t);      // 0, or -1 with slh_last_error naming the code's fault

// every refusal behind the decoder says which tile it is about
#define GEMM_CHECK(cond, fmt, ...) SLH_CHECK(cond, "slh_gemm: " fmt " (%d x %d tile, 0x%x)", ##__VA_ARGS__, t.bm, t.bn, d->tile)

// contracts that more than one family applies with its own parameters (gemm.hip)
int gemm_check_vt(const slh_gemm_desc* d, const GemmTile& t, int col_align, int token_align);      // vt_out
int gemm_check_whole_tiles(const slh_gemm_desc* d, const GemmTile& t, int w_align);                // gemm5.hip / gemm7.hip: what both are
// group_m of the grouped tile order of gemm5.hip / gemm7.hip: the power of two that minimises the operand rows an XCD pulls through its L2
int gemm_group_m(int tiles_m, int tiles_n, int bm, int bn);

// the families' own parts of the rule (options they have at all, divisibility, stricter alignments, which tiles take which option)
// and their launches; slh_gemm has checked d before it launches
int gemm5_check(const slh_gemm_desc* d, const GemmTile& t);
int gemm7_check(const slh_gemm_desc* d, const GemmTile& t);
int slh_gemm5_launch(const slh_gemm_desc* d, const GemmTile& t, slh_stream_t stream);
int slh_gemm7_launch(const slh_gemm_desc* d, const GemmTile& t, slh_stream_t stream);
