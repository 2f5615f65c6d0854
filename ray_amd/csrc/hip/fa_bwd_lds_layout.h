// LDS tile image, address helpers and small conversions shared by the
// key-on-lane dK/dV kernel (fa_bwd_dkv_v6.hip) and dq v5 (fa_bwd_dq_v5.hip).
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

// Two f32 -> packed bf16 (round to nearest even) as a plain cast, which
// hipcc lowers to v_cvt_pk_bf16_f32 and schedules like any VALU write.
// The inline-asm fb3_cvt_pk of fa_bwd_v3.hip is not used here: with its
// result as the A operand of the very next MFMA, dQ came out wrong in the 32
// columns of that first MFMA (measured; PERFORMANCE.md, backward ladder,
// "cvt_pk"), which is what a missing VALU-write -> MFMA-read wait state
// looks like. dq v3 is unaffected: a permlane32_swap sits in between.
typedef __attribute__((ext_vector_type(2))) __bf16 fb6_bf16x2;
DEV_INLINE unsigned int fb6_cvt_pk(float lo, float hi) {
  fb6_bf16x2 v{(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned int, v);
}

typedef __attribute__((ext_vector_type(4))) unsigned int fb6_u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int fb6_u32x2;
