// Paged-KV prefill attention: a chunk of Tq query tokens per sequence
// attends causally to K/V that already sit in the paged cache.
//
// q [B, Tq, Hq, D] bf16 (the model's post-RoPE layout), k_cache /
// v_cache [num_pages, Hkv, PAGE, D] as in paged_attn.hip. The chunk's
// own K/V are appended to the pages before the launch; query row i of
// sequence b sits at position ctx_lens[b] + i and sees cache rows
// j <= ctx_lens[b] + i. Rows i >= q_lens[b] are written as zeros.
//
// paged_attn_prefill_kernel<D, WAVES, FP8>: grid (ceil(Tq/(32*WAVES)), Hq, B),
// WAVES x 32 query rows per block. The binding launches 4 waves
// (128-row tiles) until those make PP_WIDE_TILE_BLOCKS blocks, then 8
// (256-row tiles, which stage each K/V tile half as often per query
// row). The math is flash_attn_v6's swapped-operand form on
// mfma_f32_32x32x16_bf16 (S' = K.Q^T so a lane owns one query column,
// lane-local fp32 online softmax in exp2 form with defer-max, P to
// B-fragments by cvt_pk + permlane32_swap, V^T by ds_read_tr16_b64),
// with the same fragment layouts and K XOR-swizzle. What differs is the
// staging: a KV tile is 64 tokens = 4 pages; each 16-row slab of a tile
// is the contiguous PAGE*D block of one (page, kv head), found through
// the block table, clamped into the pool, and copied in 8-element
// chunks into double-buffered LDS while the previous tile computes.
//
// Cache rows at or beyond ctx + q_len (tail slots of the last page,
// unused table entries, the null page) are never loaded: they are
// staged as zeros and masked to -inf, so uninitialised pool memory
// cannot reach the result through 0 x NaN. KV tiles wholly above a
// query tile's causal diagonal are not visited. One plain launch, no
// split over KV: the query-tile grid is the parallelism at prefill
// sizes. Query tiles are issued last-first so the longest ones start
// first.
//
// FP8 caches (FP8 = true) hold OCP e4m3fn bytes, value = byte * scale.
// Only the staging differs: a chunk is 8 bytes instead of 16, and the
// LDS write converts fp8 -> f32 -> bf16 in registers (exact: e4m3 has 3
// mantissa bits), so LDS holds the same bf16 image, swizzle included,
// and everything after it is the bf16 code. k_scale is folded into
// `scale` by the binding, v_scale (oscale) into the final 1/l.
#include <type_traits>

#include "common.h"

#define PP_PAGE 16
#define PP_QW 32                      // query rows per wave
#define PP_BN 64                      // staged K/V rows per tile (4 pages)
// 128-row query tiles at or past which the binding picks 256-row tiles
#define PP_WIDE_TILE_BLOCKS 512

typedef __attribute__((ext_vector_type(8))) __bf16 pp_bf16x8;
typedef __attribute__((ext_vector_type(16))) float pp_f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int pp_u32x4;

DEV_INLINE pp_bf16x8 pp_ld8(const short* p) {
  short8 s = *reinterpret_cast<const short8*>(p);
  return __builtin_bit_cast(pp_bf16x8, s);
}

// v_cvt_pk_bf16_f32: 2 f32 -> packed 2x bf16
DEV_INLINE unsigned int pp_cvt_pk(float lo, float hi) {
  unsigned int r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

typedef __attribute__((ext_vector_type(2))) int pp_int2;

// a staged 8-element chunk as bf16: bf16 chunks as they are
DEV_INLINE short8 pp_stage_bf16(const short8 x) { return x; }

DEV_INLINE short8 pp_stage_bf16(const pp_int2 x) {
  typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
  u32x4 w;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float2v lo = __builtin_amdgcn_cvt_pk_f32_fp8(x[i], false);
    const float2v hi = __builtin_amdgcn_cvt_pk_f32_fp8(x[i], true);
    w[2 * i] = pp_cvt_pk(lo[0], lo[1]);
    w[2 * i + 1] = pp_cvt_pk(hi[0], hi[1]);
  }
  return __builtin_bit_cast(short8, w);
}

// WAVES x 32 query rows per block, two waves per SIMD (256 registers a
// lane): two blocks per CU at 4 waves, one at 8 (64 KB of LDS a block
// at D = 128), so one wave's staging and softmax overlap another's
// MFMAs.
template <int D, int WAVES, bool FP8>
__global__ __launch_bounds__(WAVES * 64, 2) void
paged_attn_prefill_kernel(
    const short* __restrict__ Q,          // [B, Tq, Hq, D]
    const void* __restrict__ Kc_,         // [num_pages, Hkv, PAGE, D]
    const void* __restrict__ Vc_,
    const int* __restrict__ block_table,  // [B, max_pages]
    const int* __restrict__ ctx_lens,     // [B]
    const int* __restrict__ q_lens,       // [B]
    short* __restrict__ Out,              // [B, Tq, Hq, D]
    int Tq, int Hq, int Hkv, int num_pages, int max_pages, float scale,
    float oscale) {
  // cache element and the 8-element chunk a thread stages
  typedef std::conditional_t<FP8, unsigned char, short> elem_t;
  typedef std::conditional_t<FP8, pp_int2, short8> stage_t;
  const elem_t* Kc = static_cast<const elem_t*>(Kc_);
  const elem_t* Vc = static_cast<const elem_t*>(Vc_);
  static_assert(D == 64 || D == 128, "head_dim is 64 or 128");
  static_assert(WAVES == 4 || WAVES == 8, "4 or 8 waves per block");
  constexpr int PP_BM = PP_QW * WAVES;   // query rows per block
  constexpr int PP_THREADS = WAVES * 64;
  constexpr int QC = D / 16;   // k-chunks of the S' product
  constexpr int DT = D / 32;   // 32-column tiles of the output
  constexpr int CPR = D / 8;   // 8-element chunks per row
  constexpr int NST = PP_BN * CPR / PP_THREADS;  // staged chunks per thread
  static_assert(PP_BN * CPR % PP_THREADS == 0, "staging must divide evenly");

  __shared__ short k_lds[2][PP_BN][D];
  __shared__ short v_lds[2][PP_BN][D];

  const int q0 = (gridDim.x - 1 - blockIdx.x) * PP_BM;  // long tiles first
  const int hq = blockIdx.y;
  const int b = blockIdx.z;
  const int hkv = hq / (Hq / Hkv);
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int qcol = lane & 31;
  const int hi = lane >> 5;
  const int a_off = 8 * hi;

  // never leave the block table: lengths are clamped to its capacity
  const int cap = max_pages * PP_PAGE;
  const int ctx = min(max(ctx_lens[b], 0), cap);
  const int qlen = min(max(q_lens[b], 0), Tq);
  const int kv_len = min(ctx + qlen, cap);

  const int my_q = q0 + wave * PP_QW + qcol;   // row within the chunk
  const int gq = ctx + my_q;                   // its cache position
  const int wave_gq_min = ctx + q0 + wave * PP_QW;
  const int wave_gq_max = wave_gq_min + PP_QW - 1;
  const long long q_rs = (long long)Hq * D;
  const long long my_row = (((long long)b * Tq + my_q) * Hq + hq) * D;

  // a query tile with no valid row (block-uniform): zeros, no KV read
  if (q0 >= qlen) {
    if (my_q < Tq) {
      const short8 zero = short8{0, 0, 0, 0, 0, 0, 0, 0};
      for (int c = hi; c < CPR; c += 2)
        *reinterpret_cast<short8*>(Out + my_row + c * 8) = zero;
    }
    return;
  }

  // Q fragments (B operand): a lane reads its own query row; rows past
  // q_len (and so any row past Tq) are zeros and are never dereferenced
  pp_bf16x8 q_frag[QC];
  {
    const bool q_ok = my_q < qlen;
    const short8 zero = short8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < QC; ++c)
      q_frag[c] = q_ok ? pp_ld8(Q + my_row + 16 * c + a_off)
                       : __builtin_bit_cast(pp_bf16x8, zero);
  }

  pp_f32x16 o_acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) o_acc[t] = pp_f32x16{};
  float m_run = -INFINITY, l_run = 0.f;

  // KV rows this query tile can see; tiles above the diagonal are skipped
  const int k_end = min(kv_len, ctx + min(q0 + PP_BM, qlen));
  const int n_tiles = (k_end + PP_BN - 1) / PP_BN;

  const int* bt = block_table + (long long)b * max_pages;
  stage_t k_stage[NST], v_stage[NST];
  int pg_stage[NST];  // page ids of this thread's rows, one tile ahead

  // Page ids of the rows a thread stages in tile t_idx, clamped into the
  // pool. With 4 waves they are fetched a whole tile before the K/V
  // loads that depend on them, so a wave does not wait on the table in
  // the middle of a tile (measured: 7-9% faster). With 8 waves the same
  // prefetch measured 3% slower, so there the table is read in place.
  constexpr bool PREFETCH = WAVES == 4;
#define PP_LOAD_PAGES(t_idx)                                              \
  do {                                                                    \
    const int kt0 = (t_idx)*PP_BN;                                        \
    _Pragma("unroll") for (int j = 0; PREFETCH && j < NST; ++j) {         \
      const int krow = kt0 + (threadIdx.x + PP_THREADS * j) / CPR;        \
      int page = 0;                                                       \
      if (krow < k_end) page = bt[krow / PP_PAGE];                        \
      pg_stage[j] = min(max(page, 0), num_pages - 1);                     \
    }                                                                     \
  } while (0)

  // Stage rows [kt0, kt0 + 64) from the pages in pg_stage. Chunk i ->
  // row i / CPR: the 16 rows of a page/kv-head slab are PAGE*D
  // contiguous elements.
#define PP_LOAD_TILE(t_idx)                                               \
  do {                                                                    \
    const int kt0 = (t_idx)*PP_BN;                                        \
    _Pragma("unroll") for (int j = 0; j < NST; ++j) {                     \
      const int i = threadIdx.x + PP_THREADS * j;                         \
      const int r = i / CPR;                                              \
      const int c = (i % CPR) * 8;                                        \
      const int krow = kt0 + r;                                           \
      stage_t kv{}, vv{};                                                 \
      if (krow < k_end) {                                                 \
        const int page =                                                  \
            PREFETCH ? pg_stage[j]                                        \
                     : min(max(bt[krow / PP_PAGE], 0), num_pages - 1);    \
        const long long off =                                             \
            (((long long)page * Hkv + hkv) * PP_PAGE + (krow % PP_PAGE)) * \
                D + c;                                                    \
        kv = *reinterpret_cast<const stage_t*>(Kc + off);                 \
        vv = *reinterpret_cast<const stage_t*>(Vc + off);                 \
      }                                                                   \
      k_stage[j] = kv;                                                    \
      v_stage[j] = vv;                                                    \
    }                                                                     \
  } while (0)

#define PP_WRITE_TILE(buf)                                                \
  do {                                                                    \
    _Pragma("unroll") for (int j = 0; j < NST; ++j) {                     \
      const int i = threadIdx.x + PP_THREADS * j;                         \
      const int r = i / CPR;                                              \
      const int c = (i % CPR) * 8;                                        \
      /* K swizzled: col_shorts ^= (row&7)<<3 */                          \
      *reinterpret_cast<short8*>(&k_lds[buf][r][c ^ ((r & 7) << 3)]) =    \
          pp_stage_bf16(k_stage[j]);                                      \
      *reinterpret_cast<short8*>(&v_lds[buf][r][c]) =                     \
          pp_stage_bf16(v_stage[j]);                                      \
    }                                                                     \
  } while (0)

  // prologue: stage tile 0 (n_tiles >= 1 here: q0 < qlen so k_end > 0,
  // unless the table has no room, and then every row stages as zero)
  PP_LOAD_PAGES(0);
  PP_LOAD_TILE(0);
  PP_LOAD_PAGES(1);
  PP_WRITE_TILE(0);
  __syncthreads();

  const float THR = 8.f;  // defer-max threshold
  const float L2E = 1.4426950408889634f;

  for (int t = 0; t < n_tiles; ++t) {
    const int cur = t & 1;
    const int k0 = t * PP_BN;
    if (t + 1 < n_tiles) {
      PP_LOAD_TILE(t + 1);
      PP_LOAD_PAGES(t + 2);
    }

    if (k0 <= wave_gq_max) {
      const bool do0 = (k0 < k_end);
      const bool do1 = (k0 + 32 < k_end) && (k0 + 32 <= wave_gq_max);

      auto s_mfma = [&](int kt) {
        pp_f32x16 acc{};
        const int rr = 32 * kt + (lane & 31);
        const short* krow = &k_lds[cur][rr][0];
        const int sw = (rr & 7) << 3;
#pragma unroll
        for (int c = 0; c < QC; ++c) {
          pp_bf16x8 kf = pp_ld8(krow + ((16 * c + a_off) ^ sw));
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, q_frag[c], acc,
                                                        0, 0, 0);
        }
        return acc;
      };

      auto softmax_pv = [&](int kt, pp_f32x16 s_acc) {
        const int k0s = k0 + 32 * kt;
        const bool full_tile =
            (k0s + 32 <= k_end) && (k0s + 31 <= wave_gq_min);
        float p_reg[16];
        float rmax = -INFINITY;
        if (full_tile) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            p_reg[r] = s_acc[r] * scale;
            rmax = fmaxf(rmax, p_reg[r]);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int krow = (r & 3) + 8 * (r >> 2) + 4 * hi;
            const int gk = k0s + krow;
            const float sv = s_acc[r] * scale;
            const bool masked = (gk >= k_end) || (gk > gq);
            p_reg[r] = masked ? -INFINITY : sv;
            rmax = fmaxf(rmax, p_reg[r]);
          }
        }
        rmax = fmaxf(rmax, __shfl_xor(rmax, 32, 64));
        const bool need_rescale =
            (m_run == -INFINITY) || (rmax - m_run > THR);
        const float m_new = need_rescale ? fmaxf(m_run, rmax) : m_run;
        float sc = 1.f;
        if (need_rescale)
          sc = (m_run == -INFINITY) ? 0.f : __expf(m_run - m_new);
        if (m_new == -INFINITY) sc = 0.f;
        const float mb = m_new * L2E;
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = (m_new == -INFINITY)
                              ? 0.f
                              : __builtin_amdgcn_exp2f(
                                    __builtin_fmaf(p_reg[r], L2E, -mb));
          p_reg[r] = p;
          psum += p;
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

        // P -> B-fragments via cvt_pk + permlane32_swap, then PV with
        // V^T A-fragments from ds_read_tr16_b64 (flash_attn_v6.hip has
        // the lane maps)
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
          unsigned int a0 = pp_cvt_pk(p_reg[8 * kc + 0], p_reg[8 * kc + 1]);
          unsigned int a1 = pp_cvt_pk(p_reg[8 * kc + 2], p_reg[8 * kc + 3]);
          unsigned int b0 = pp_cvt_pk(p_reg[8 * kc + 4], p_reg[8 * kc + 5]);
          unsigned int b1 = pp_cvt_pk(p_reg[8 * kc + 6], p_reg[8 * kc + 7]);
          auto sw0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
          auto sw1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
          pp_u32x4 pw{(unsigned)sw0[0], (unsigned)sw1[0], (unsigned)sw0[1],
                      (unsigned)sw1[1]};
          pp_bf16x8 pb = __builtin_bit_cast(pp_bf16x8, pw);
          const int gl = lane & 15;
          const int grp16 = (lane >> 4) & 1;
          const int vrow0 = 32 * kt + kc * 16 + a_off + (gl >> 2);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            const int vcol = dt * 32 + 16 * grp16 + 4 * (gl & 3);
            auto p0 = (__attribute__((address_space(3))) short4v*)
                &v_lds[cur][vrow0][vcol];
            auto p1 = (__attribute__((address_space(3))) short4v*)
                &v_lds[cur][vrow0 + 4][vcol];
            short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(p0);
            short4v hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(p1);
            short vtmp[8] = {lo[0], lo[1], lo[2], lo[3],
                             hi4[0], hi4[1], hi4[2], hi4[3]};
            pp_bf16x8 va = __builtin_bit_cast(
                pp_bf16x8, *reinterpret_cast<short8*>(vtmp));
            o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                va, pb, o_acc[dt], 0, 0, 0);
          }
        }
      };

      pp_f32x16 sA{}, sB{};
      if (do0) sA = s_mfma(0);
      if (do1) sB = s_mfma(1);  // in flight under sub-tile 0's softmax
      if (do0) softmax_pv(0, sA);
      if (do1) softmax_pv(1, sB);
    }

    if (t + 1 < n_tiles) {
      PP_WRITE_TILE(cur ^ 1);
    }
    __syncthreads();
  }
#undef PP_LOAD_PAGES
#undef PP_LOAD_TILE
#undef PP_WRITE_TILE

  // ---- epilogue: O[q][d] = O'[d][q] / l; padded rows are zeros ----
  if (my_q < Tq) {
    float inv = (my_q < qlen && l_run > 0.f) ? 1.f / l_run : 0.f;
    if constexpr (FP8) inv *= oscale;
    short* op = Out + my_row;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; r += 4) {
        // accumulator regs r..r+3 are 4 adjacent output columns
        const int d = 8 * (r >> 2) + 4 * hi + 32 * dt;
        short4v o4;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o4[e] = my_q < qlen ? f2bf(o_acc[dt][r + e] * inv) : (short)0;
        *reinterpret_cast<short4v*>(op + d) = o4;
      }
  }
}
