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
// row). The math is the swapped-operand tile math of fa_tile.h (s_tile,
// softmax_step with causal always on, pv_tile) over a K-swizzled LDS
// tile. This kernel's own part is the staging: a KV tile is 64 tokens =
// 4 pages; each 16-row slab of a tile is the contiguous PAGE*D block of
// one (page, kv head), found through the block table, clamped into the
// pool, and copied in 8-element chunks into double-buffered LDS while the
// previous tile computes.
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

#include "fa_tile.h"

#define PP_PAGE 16
#define PP_QW 32                      // query rows per wave
#define PP_BN 64                      // staged K/V rows per tile (4 pages)
// 128-row query tiles at or past which the binding picks 256-row tiles
#define PP_WIDE_TILE_BLOCKS 512

typedef __attribute__((ext_vector_type(2))) int pp_int2;

// a staged 8-element chunk as bf16: bf16 chunks as they are
DEV_INLINE short8 pp_stage_bf16(const short8 x) { return x; }

// fp8 chunks converted; the result goes to LDS, not to an MFMA
DEV_INLINE short8 pp_stage_bf16(const pp_int2 x) {
  u32x4 w;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float2v lo = __builtin_amdgcn_cvt_pk_f32_fp8(x[i], false);
    const float2v hi = __builtin_amdgcn_cvt_pk_f32_fp8(x[i], true);
    w[2 * i] = cvt_pk_asm(lo[0], lo[1]);
    w[2 * i + 1] = cvt_pk_asm(hi[0], hi[1]);
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
  bf16x8 q_frag[QC];
  {
    const bool q_ok = my_q < qlen;
    const short8 zero = short8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < QC; ++c)
      q_frag[c] = q_ok ? ld8(Q + my_row + 16 * c + a_off)
                       : __builtin_bit_cast(bf16x8, zero);
  }

  f32x16 o_acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) o_acc[t] = f32x16{};
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
      *reinterpret_cast<short8*>(&k_lds[buf][r][k_swz(r, c)]) =           \
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

      auto softmax_pv = [&](int kt, f32x16 s_acc) {
        const f32x16 p =
            softmax_step<DT>(s_acc, o_acc, m_run, l_run, k0 + 32 * kt, k_end,
                             true, gq, wave_gq_min, scale, hi);
        pv_tile(p, v_lds[cur], kt, lane, hi, o_acc);
      };

      f32x16 sA{}, sB{};
      if (do0) sA = s_tile(k_lds[cur], 0, lane, hi, q_frag);
      // in flight under sub-tile 0's softmax
      if (do1) sB = s_tile(k_lds[cur], 1, lane, hi, q_frag);
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
