// Head dimension, staged tile height and the 32x32x16 bf16 MFMA fragment
// types shared by the attention backward kernels (fa_bwd_prep.hip,
// fa_bwd_v3.hip, fa_bwd_dq_v5.hip, fa_bwd_dkv_v6.hip).
#pragma once
#include "common.h"

#define FB3_D 128
#define FB3_QT 64           // q rows per staged tile (2 sub-tiles of 32)

typedef __attribute__((ext_vector_type(8))) __bf16 fb3_bf16x8;
typedef __attribute__((ext_vector_type(16))) float fb3_f32x16;

DEV_INLINE fb3_bf16x8 fb3_ld8(const short* p) {
  short8 s = *reinterpret_cast<const short8*>(p);
  return __builtin_bit_cast(fb3_bf16x8, s);
}
