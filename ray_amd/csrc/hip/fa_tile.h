// Tile math shared by the attention kernels: fragment types, the two
// cvt_pk forms, the K swizzle, S' = K·Q^T, the online-softmax step and
// P·V. flash_attn_v5.hip and paged_attn_prefill.hip call s_tile,
// softmax_step and pv_tile; flash_attn_v7.hip calls the two-phase form of
// the same arithmetic at the end of this file. The backward kernels take
// the types and conversions and the pieces that are the same in either
// direction: c_row, the packed exchange of a C-layout tile (pack_swap),
// the two-read transposed gather (ld_tr8) and the C-layout store of an
// output tile (c_store). Staging, base-address prologues and the kernels'
// own epilogues stay with the kernels: that is where they differ.
//
// Swapped-operand form: S' = K·Q^T puts S'[k][q] in C layout with
// q = lane&31, so a lane owns ONE query column. The softmax max/sum over
// k is in-register plus one exchange with the partner lane (l ^ 32, which
// holds the other half of the k rows), P feeds P·V's B operand without an
// LDS round trip, and O accumulates as O'[d][q], whose rescale is a
// lane-local scalar multiply.
//
// Lane layouts of mfma_f32_32x32x16_bf16 (verified by fa_probe32.hip):
//   A (32x16) row-major: lane l holds A[l&31][8*(l>>5)+i], i = 0..7
//   B (16x32):           lane l holds B[8*(l>>5)+i][l&31]
//   C (32x32):           col = l&31, row = (reg&3) + 8*(reg>>2) + 4*(l>>5)
// ds_read_tr16_b64 (verified by tr_probe.hip), per 16-lane group, on a
// 4-row x 16-column block of 16-bit elements: supplier lane 4q+p gives
// the address of row q, columns 4p..4p+3; consumer lane i receives column
// i of the four rows, row q in element q. pv_tile's two reads hand lane l
// V[8*(l>>5) + j][32*dt + (l&31)], j = 0..7, of a 16-row chunk: the A
// fragment of V^T.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

DEV_INLINE bf16x8 ld8(const short* p) {
  short8 s = *reinterpret_cast<const short8*>(p);
  return __builtin_bit_cast(bf16x8, s);
}

// Two f32 -> packed bf16 (round to nearest even), in two forms.
//
// cvt_pk, the default, is a plain cast, which hipcc lowers to
// v_cvt_pk_bf16_f32 and schedules like any VALU write.
//
// cvt_pk_asm issues the same instruction from inline asm, which the
// compiler's hazard tracking does not see. It is safe only where another
// VALU or permlane instruction sits between it and the MFMA that reads
// the result, as the permlane32_swap of pv_tile and of dq v3 does
// (pack_swap<true>). With its result as the A operand of the very next
// MFMA, dq v5's dQ came out wrong in the 32 columns of that first MFMA
// (measured; PERFORMANCE.md, backward ladder, "cvt_pk"), which is what a
// missing VALU-write -> MFMA-read wait state looks like: dq v5 calls
// pack_swap<false>. Moving a kernel from one form to the other changes its
// code generation: measure it.
DEV_INLINE unsigned int cvt_pk(float lo, float hi) {
  bf16x2 v{(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned int, v);
}
DEV_INLINE unsigned int cvt_pk_asm(float lo, float hi) {
  unsigned int r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// Row of C-layout register r; here and below, hi = lane >> 5.
//
// A shared function is simplified on its own before it is inlined, so a
// call is not always the code of the same lines written in place. Where
// c_row, ld_tr8 or c_store changed a backward kernel's tile loop (the mask
// compares of every backward kernel, the K gathers of dq v3 and dq v5,
// dq v3's epilogue, dkv v6's paired reads) the kernel keeps the lines and
// says so; tools/kernel_isa_diff.py shows what a call site does.
DEV_INLINE int c_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// Registers 8kc .. 8kc+7 of a C-layout tile (8 of the lane's 16 rows, one
// column) as the A/B fragment of k-step kc: packed to bf16 and exchanged
// with the partner lane (guide T12: one permlane32_swap fills two fragment
// words, no divergent hi/lo branch). ASM chooses the cvt_pk form, see above.
template <bool ASM>
DEV_INLINE bf16x8 pack_swap(const f32x16& p, int kc) {
  auto pk = [](float lo, float hi) {
    return ASM ? cvt_pk_asm(lo, hi) : cvt_pk(lo, hi);
  };
  unsigned int a0 = pk(p[8 * kc + 0], p[8 * kc + 1]);
  unsigned int a1 = pk(p[8 * kc + 2], p[8 * kc + 3]);
  unsigned int b0 = pk(p[8 * kc + 4], p[8 * kc + 5]);
  unsigned int b1 = pk(p[8 * kc + 6], p[8 * kc + 7]);
  auto sw0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
  auto sw1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
  u32x4 pw{(unsigned)sw0[0], (unsigned)sw1[0], (unsigned)sw0[1],
           (unsigned)sw1[1]};
  return __builtin_bit_cast(bf16x8, pw);
}

// Two ds_read_tr16_b64 at the LDS addresses p0 and p1 as one fragment:
// elements 0..3 from p0's 4-row block, 4..7 from p1's.
DEV_INLINE bf16x8 ld_tr8(const short* p0, const short* p1) {
  typedef __attribute__((address_space(3))) short4v* lds4;
  short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)p0);
  short4v hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)p1);
  short tmp[8] = {lo[0], lo[1], lo[2], lo[3], hi4[0], hi4[1], hi4[2], hi4[3]};
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<short8*>(tmp));
}

// A wave's 32-row x 128-column C-layout tile to bf16 rows at `out`, row
// stride rs elements.
DEV_INLINE void c_store(const f32x16 (&acc)[4], short* out, long long rs,
                        int lane, int hi) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      out[(long long)c_row(r, hi) * rs + 32 * dt + (lane & 31)] =
          f2bf(acc[dt][r]);
}

// K LDS XOR-swizzle (guide T2): element column c (a multiple of 8) of
// row r of a [rows][D] tile sits at column k_swz(r, c), so the S'-phase
// ds_read_b128 of 32 different rows at one column range spreads over the
// banks. Writer and reader both go through this.
DEV_INLINE int k_swz(int r, int c) { return c ^ ((r & 7) << 3); }

// S' = K·Q^T for the 32-row sub-tile kt of a swizzled [rows][D] LDS tile;
// q_frag is the lane's own query row as B fragments.
template <int D, int ROWS>
DEV_INLINE f32x16 s_tile(const short (&k_tile)[ROWS][D], int kt, int lane,
                         int hi, const bf16x8 (&q_frag)[D / 16]) {
  f32x16 acc{};
  const int rr = 32 * kt + (lane & 31);
  const short* krow = &k_tile[rr][0];
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    bf16x8 kf = ld8(krow + k_swz(rr, 16 * c + 8 * hi));
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, q_frag[c], acc, 0, 0,
                                                  0);
  }
  return acc;
}

// One online-softmax step over the 32-key sub-tile starting at key k0s:
// s_acc (C layout) -> the lane's 16 unnormalised probabilities (same
// layout), with m_run / l_run updated and the DT output tiles rescaled
// when the running max moves. Keys at or past k_lim, and under `causal`
// keys above the lane's global query index gq, are masked; gq0 is the
// wave's smallest gq, which decides the unmasked fast path.
// Defer-max (guide T13): the old running max is kept while the tile max
// stays within THR of it. P is then bounded by e^THR, which the fp32
// accumulators tolerate, and the O rescale pass is skipped entirely.
template <int DT>
DEV_INLINE f32x16 softmax_step(f32x16 s_acc, f32x16 (&o_acc)[DT],
                               float& m_run, float& l_run, int k0s, int k_lim,
                               int causal, int gq, int gq0, float scale,
                               int hi) {
  const float THR = 8.f;
  const float L2E = 1.4426950408889634f;
  const bool full_tile =
      (k0s + 32 <= k_lim) && (!causal || (k0s + 31 <= gq0));
  // one vector multiply in front of the branch, not a scalar one in each
  // arm: that form costs every kernel registers (PERFORMANCE.md, "forward
  // tile math shared")
  f32x16 p = s_acc * scale;
  float rmax = -INFINITY;
  if (full_tile) {
#pragma unroll
    for (int r = 0; r < 16; ++r) rmax = fmaxf(rmax, p[r]);
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int gk = k0s + c_row(r, hi);
      bool masked = (gk >= k_lim) || (causal && gk > gq);
      p[r] = masked ? -INFINITY : p[r];
      rmax = fmaxf(rmax, p[r]);
    }
  }
  rmax = fmaxf(rmax, __shfl_xor(rmax, 32, 64));
  bool need_rescale = (m_run == -INFINITY) || (rmax - m_run > THR);
  float m_new = need_rescale ? fmaxf(m_run, rmax) : m_run;
  float sc = 1.f;
  if (need_rescale)
    sc = (m_run == -INFINITY) ? 0.f : __expf(m_run - m_new);
  if (m_new == -INFINITY) sc = 0.f;
  float mb = m_new * L2E;
  float psum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    p[r] = (m_new == -INFINITY)
               ? 0.f
               : __builtin_amdgcn_exp2f(__builtin_fmaf(p[r], L2E, -mb));
    psum += p[r];
  }
  psum += __shfl_xor(psum, 32, 64);
  l_run = l_run * sc + psum;
  m_run = m_new;

  if (need_rescale) {
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) o_acc[d][r] *= sc;
  }
  return p;
}

// O' += V^T·P for the 32-row sub-tile kt of an unswizzled [rows][D] LDS
// tile. P -> B fragments by pack_swap; V^T A fragments by ld_tr8 (guide
// T10): two reads replace 32 u16 gathers per (16-key chunk, 32-column
// tile).
template <int D, int ROWS>
DEV_INLINE void pv_tile(f32x16 p, const short (&v_tile)[ROWS][D], int kt,
                        int lane, int hi, f32x16 (&o_acc)[D / 32]) {
  const int gl = lane & 15;
  const int grp16 = (lane >> 4) & 1;
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) {
    bf16x8 pb = pack_swap<true>(p, kc);
    const int vrow0 = 32 * kt + kc * 16 + 8 * hi + (gl >> 2);
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) {
      const int vcol = dt * 32 + 16 * grp16 + 4 * (gl & 3);
      bf16x8 va = ld_tr8(&v_tile[vrow0][vcol], &v_tile[vrow0 + 4][vcol]);
      o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, pb, o_acc[dt],
                                                          0, 0, 0);
    }
  }
}

// ---- Two-phase form of the same tile math (flash_attn_v7.hip) ----
//
// The pieces above run S, softmax and P·V of a sub-tile back to back. The
// pieces below cut the same arithmetic, operation for operation, into a
// VALU phase (softmax_pack: scores -> packed P, no LDS access) and a
// matrix phase (pv_sub, s_sub: every MFMA and every LDS read), so that the
// two waves of a SIMD can run the two phases against each other. K and V
// are read from the [64][128] image of fa_bwd_lds_layout.h (fb6_off).

// Transposed-read base of pv_sub: the 4 rows 16kc + 8hi + 4h .. +3 of a
// 32-row sub-tile, columns 32dt + 16grp16 .. +15, sit at
// fa_pv_tbase(lane, h) + 2048kc + 256dt of the sub-tile's image. The lane
// halves take rows 8hi .. 8hi+7 of each 16-key chunk, as pv_tile does, so
// the MFMA sees the same operands in the same k slots; fb6_tbase's row
// assignment (4hi and 8 + 4hi) belongs to the backward kernels' permuted
// fragments.
DEV_INLINE int fa_pv_tbase(int lane, int h) {
  const int gl = lane & 15;
  const int grp16 = (lane >> 4) & 1;
  const int hi = lane >> 5;
  return 1024 * hi + 32 * (4 * h + (gl >> 2)) +
         8 * ((2 * grp16 + ((gl & 3) >> 1)) ^ ((2 * hi + h) & 3)) +
         4 * (gl & 1);
}

// S' = K·Q^T of one 32-key sub-tile whose image starts at k_img; rb0 and
// rb1 are fb6_rbase(lane, 0 / 1). All 8 fragments are read before the
// chain, so no MFMA waits on the read issued just in front of it.
DEV_INLINE f32x16 s_sub(const short* k_img, int rb0, int rb1,
                        const bf16x8 (&q_frag)[8]) {
  bf16x8 kf[8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
    kf[c] = ld8(k_img + ((c & 1) ? rb1 : rb0) + 256 * (c >> 1));
  f32x16 acc{};
#pragma unroll
  for (int c = 0; c < 8; ++c)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[c], q_frag[c], acc, 0,
                                                  0, 0);
  return acc;
}

// x of the partner lane (l ^ 32) combined with the lane's own by max / by
// sum, through one v_permlane32_swap instead of a ds_bpermute round trip
// through the LDS pipe. a keeps the low half's x in both halves, b the
// high half's; max and + are commutative, so the result has the bits of
// fmaxf(x, __shfl_xor(x, 32)) and of x + __shfl_xor(x, 32).
DEV_INLINE void halves32(float x, float& a, float& b) {
  const unsigned u = __builtin_bit_cast(unsigned, x);
  auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  a = __builtin_bit_cast(float, (unsigned)sw[0]);
  b = __builtin_bit_cast(float, (unsigned)sw[1]);
}

// softmax_step without the O rescale, followed by pv_tile's packing:
// s_acc -> the two B fragments of P (16 keys each). m_run and l_run are
// updated; `need` and `sc` tell the caller to multiply O by sc before this
// sub-tile's P·V (and after the previous one's). MASKED = false is
// softmax_step's full_tile arm; MASKED = true applies the k_lim and causal
// masks by select, which leaves an unmasked score as it is.
template <bool MASKED>
DEV_INLINE void softmax_pack(f32x16 s_acc, float& m_run, float& l_run,
                             int k0s, int k_lim, int causal, int gq,
                             float scale, int hi, bf16x8 (&pb)[2],
                             bool& need, float& sc_out) {
  const float THR = 8.f;
  const float L2E = 1.4426950408889634f;
  f32x16 p = s_acc * scale;
  float rmax = -INFINITY;
  if (!MASKED) {
#pragma unroll
    for (int r = 0; r < 16; ++r) rmax = fmaxf(rmax, p[r]);
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int gk = k0s + c_row(r, hi);
      bool masked = (gk >= k_lim) || (causal && gk > gq);
      p[r] = masked ? -INFINITY : p[r];
      rmax = fmaxf(rmax, p[r]);
    }
  }
  {
    float a, b;
    halves32(rmax, a, b);
    rmax = fmaxf(a, b);
  }
  bool need_rescale = (m_run == -INFINITY) || (rmax - m_run > THR);
  float m_new = need_rescale ? fmaxf(m_run, rmax) : m_run;
  float sc = 1.f;
  if (need_rescale)
    sc = (m_run == -INFINITY) ? 0.f : __expf(m_run - m_new);
  if (m_new == -INFINITY) sc = 0.f;
  float mb = m_new * L2E;
  float psum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    p[r] = (m_new == -INFINITY)
               ? 0.f
               : __builtin_amdgcn_exp2f(__builtin_fmaf(p[r], L2E, -mb));
    psum += p[r];
  }
  {
    float a, b;
    halves32(psum, a, b);
    psum = a + b;
  }
  l_run = l_run * sc + psum;
  m_run = m_new;
  need = need_rescale;
  sc_out = sc;
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) pb[kc] = pack_swap<true>(p, kc);
}

// O' *= sc on the lanes whose running max moved (softmax_step's tail).
DEV_INLINE void o_rescale(f32x16 (&o_acc)[4], bool need, float sc) {
  if (need) {
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) o_acc[d][r] *= sc;
  }
}

// O' += V^T·P of one 32-key sub-tile whose image starts at v_img; tb0 and
// tb1 are fa_pv_tbase(lane, 0 / 1). Sums kc then dt, as pv_tile does.
DEV_INLINE void pv_sub(const bf16x8 (&pb)[2], const short* v_img, int tb0,
                       int tb1, f32x16 (&o_acc)[4]) {
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const int o = 2048 * kc + 256 * dt;
      bf16x8 va = ld_tr8(v_img + tb0 + o, v_img + tb1 + o);
      o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, pb[kc],
                                                          o_acc[dt], 0, 0, 0);
    }
  }
}
