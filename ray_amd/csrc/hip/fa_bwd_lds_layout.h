// LDS tile image and address helpers shared by the key-on-lane dK/dV
// kernel (fa_bwd_dkv_v6.hip), dq v5 (fa_bwd_dq_v5.hip) and gemm_wgrad.hip.
#pragma once
#include "common.h"

// element offset of 16-byte chunk ch (0..15) of row `row` in a
// [rows][128 x bf16] image (8 rows x 128 columns stay one 2 KB group)
DEV_INLINE int fb6_off(int row, int ch) {
  return 1024 * (row >> 3) + 256 * (ch >> 2) + 32 * (row & 7) +
         8 * ((ch & 3) ^ ((row >> 2) & 3));
}
// Row read (A/B fragment of the S / dP chains): lane r = lane&31 reads
// chunk 2c+hi of row 32n + r at fb6_rbase(lane, c&1) + 4096n + 256(c>>1).
DEV_INLINE int fb6_rbase(int lane, int e) {
  const int r = lane & 31;
  return 1024 * (r >> 3) + 32 * (r & 7) +
         8 * ((2 * e + (lane >> 5)) ^ ((r >> 2) & 3));
}
// Transposed read (ds_read_tr16_b64) of the 4 rows 8m + 4hi .. +3, columns
// 32dt + 16grp16 .. +15: at fb6_tbase(lane, m&1) + 1024m + 256dt.
DEV_INLINE int fb6_tbase(int lane, int m1) {
  const int gl = lane & 15;
  const int grp16 = (lane >> 4) & 1;
  const int hi = lane >> 5;
  return 32 * (4 * hi + (gl >> 2)) +
         8 * ((2 * grp16 + ((gl & 3) >> 1)) ^ ((hi + 2 * m1) & 3)) +
         4 * (gl & 1);
}

// Lane id read afresh (two VALU ops): an address used once per tile or
// only in the epilogue then holds no register across the MFMA loop.
DEV_INLINE int fb6_lane_fresh() {
  int l;
  asm volatile(
      "v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0"
      : "=v"(l));
  return l;
}
