// Paged-KV verify attention for speculative decoding: a few query tokens
// per sequence (the last accepted token and its drafts) attend causally
// to a long paged cache, with the KV split over blocks as in decode.
//
// q [B, Tq, Hq, D] bf16, caches [num_pages, Hkv, PAGE, D] bf16 or e4m3fn.
// Semantics are paged_attn_prefill.hip's: the rows' own K/V are appended
// before the launch, query row i of sequence b sits at position
// ctx_lens[b] + i and sees cache rows j <= ctx_lens[b] + i, rows
// i >= q_lens[b] are written as zeros, and a sequence with q_len <= 0
// writes zeros and loads nothing.
//
// paged_attn_verify_kernel<D, FP8>: grid (num_splits, Hkv, B), 4 waves.
//
// Columns. The Tq * REP <= 32 (token, head) pairs of one KV head are the
// 32 query columns of fa_tile.h's swapped-operand tile (keys on MFMA
// rows, one query column per lane): column c is token c / REP, head
// c % REP of the group. K and V of a group therefore stream from HBM once
// for all its heads and all its draft tokens. The causal mask is per
// column: softmax_step takes the lane's own gq = ctx + token. A column
// with no query behind it (c >= Tq * REP, or token >= q_len) has gq = -1,
// so every key is masked for it, its running max stays -inf and
// softmax_step gives it p = 0: it cannot produce NaN, and its output is
// written as zeros. When such a column exists gq0 = -1 keeps the whole
// block off softmax_step's unmasked fast path.
//
// KV split twice. The ceil((ctx + q_len) / 64) tiles of 64 tokens
// (4 pages) are cut into num_splits contiguous slices, one per block;
// wave w of a block takes tiles w, w + 4, ... of the slice. All waves
// hold the same 32 query columns with their own (m, l, O') and merge
// through LDS once at the end, in wave order. The slice bounds come from
// ctx_lens / q_lens on the device and the grid from shapes only, so a
// captured graph replays for any lengths. num_splits == 1 writes bf16;
// otherwise a block writes its unnormalised fp32 partial (m in the log2
// domain, l, o) in paged_attn_decode's workspace layout with Tq * Hq
// "heads" per sequence, and paged_attn_reduce_bf16 combines them in split
// order. A slice that is empty for a short sequence writes the neutral
// partial (m = -inf, l = 0) like any other.
//
// Staging: per wave, through LDS, 32 keys at a time. A wave owns a
// K [32][D] (k_swz-swizzled) and a V [32][D] image and runs s_tile,
// softmax_step and pv_tile on it; the next 32 rows are in flight in
// registers (D/8 16-byte loads a lane) while it computes, and their two
// page ids, which are wave-uniform, are fetched one step further ahead.
// Per wave and not per block because the waves do not share keys: a
// block-wide tile would put a barrier in every step and buy nothing,
// whereas here the four waves never wait for each other until the merge.
// Through LDS and not K-to-registers because V needs the transposed
// read (ld_tr8) anyway and K then takes the same path: 8 waves a CU
// (64 KB a block at D = 128, two blocks a CU) keep 128 KB of loads in
// flight, which is what a pure KV stream needs. The merge reuses the tile
// memory.
//
// Rows at or beyond ctx + q_len (last-page tails, unused table entries,
// the null page) are never loaded: they are staged as zeros and masked to
// -inf, since the pool is uninitialised memory and 0 x NaN is NaN. Page
// ids are clamped into the pool.
//
// FP8 caches differ in staging only (pp_stage_bf16: e4m3 -> f32 -> bf16
// in registers, exact). k_scale is folded into `scale` by the binding,
// v_scale (oscale) into the final 1/l or the partial o.
//
// This file is part of the ops.hip unit and comes after paged_attn.hip
// (pa_w, pa_store8, paged_attn_reduce_bf16) and paged_attn_prefill.hip
// (pp_int2, pp_stage_bf16).
#include <type_traits>

#include "fa_tile.h"

#define PV_PAGE 16
#define PV_WAVES 4
#define PV_BN 64        // tokens per tile: slices are whole tiles
#define PV_SUB 32       // keys a wave stages and computes at a time
#define PV_MAX_ROWS 32  // Tq * REP: the query columns of one MFMA tile

// LDS writes of one wave made visible to its own later reads: the
// hardware runs a wave's ds instructions in order, this keeps the
// compiler from moving them across.
DEV_INLINE void pv_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int D, bool FP8>
__global__ __launch_bounds__(PV_WAVES * 64, 2) void paged_attn_verify_kernel(
    const short* __restrict__ Q,          // [B, Tq, Hq, D]
    const void* __restrict__ Kc_,         // [num_pages, Hkv, PAGE, D]
    const void* __restrict__ Vc_,
    const int* __restrict__ block_table,  // [B, max_pages]
    const int* __restrict__ ctx_lens,     // [B]
    const int* __restrict__ q_lens,       // [B]
    short* __restrict__ Out,              // [B, Tq, Hq, D] (num_splits == 1)
    float* __restrict__ ws_o,             // [B, Tq*Hq, S, D]
    float* __restrict__ ws_ml,            // [B, Tq*Hq, S, 2]
    int Tq, int Hkv, int rep_shift, int num_pages, int max_pages,
    float scale, float oscale) {
  typedef std::conditional_t<FP8, unsigned char, short> elem_t;
  typedef std::conditional_t<FP8, pp_int2, short8> stage_t;
  const elem_t* Kc = static_cast<const elem_t*>(Kc_);
  const elem_t* Vc = static_cast<const elem_t*>(Vc_);
  static_assert(D == 64 || D == 128, "head_dim is 64 or 128");
  constexpr int QC = D / 16;   // k-chunks of the S' product
  constexpr int DT = D / 32;   // 32-column tiles of the output
  constexpr int CPR = D / 8;   // 8-element chunks per row
  constexpr int NST = PV_SUB * CPR / 64;  // staged chunks per lane
  constexpr int RPJ = 64 / CPR;           // rows one wave-load covers
  // chunks j < NST/2 of a lane lie in the first page of a sub-tile, the
  // others in the second
  static_assert(NST / 2 * RPJ == PV_PAGE, "a sub-tile is two pages");
  constexpr int TILE = PV_SUB * D;        // elements of one LDS image
  constexpr float L2E = 1.4426950408889634f;

  // per wave: K image, V image; after the loop: the merge buffers
  __shared__ __attribute__((aligned(16))) short smem[PV_WAVES * 2 * TILE];
  static_assert(((PV_WAVES - 1) * 16 * DT * 64 + 2 * PV_WAVES * 32) * 4 <=
                    PV_WAVES * 2 * TILE * 2,
                "merge buffers fit the tile memory");

  const int split = blockIdx.x, S = gridDim.x;
  const int hkv = blockIdx.y;
  const int b = blockIdx.z;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int qcol = lane & 31;
  const int hi = lane >> 5;
  const int a_off = 8 * hi;
  const int REP = 1 << rep_shift;
  const int Hq = Hkv * REP;

  // never leave the block table: lengths are clamped to its capacity
  const int cap = max_pages * PV_PAGE;
  const int ctx = min(max(ctx_lens[b], 0), cap);
  const int qlen = min(max(q_lens[b], 0), Tq);
  const int kv_len = qlen > 0 ? min(ctx + qlen, cap) : 0;

  // the lane's column: token, head, output row
  const int tok = qcol >> rep_shift;
  const bool q_ok = tok < qlen;   // a query stands behind the column
  const bool has_out = tok < Tq;  // the column has an output row
  const long long row =
      ((long long)b * Tq + tok) * Hq + hkv * REP + (qcol & (REP - 1));
  const int gq = q_ok ? ctx + tok : -1;
  const int gq0 = (qlen * REP < PV_MAX_ROWS) ? -1 : ctx;

  bf16x8 q_frag[QC];
  {
    const short8 zero = short8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < QC; ++c)
      q_frag[c] = q_ok ? ld8(Q + row * D + 16 * c + a_off)
                       : __builtin_bit_cast(bf16x8, zero);
  }

  f32x16 o_acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) o_acc[t] = f32x16{};
  float m_run = -INFINITY, l_run = 0.f;

  // the block's slice of tiles, and this wave's sub-tiles within it:
  // step n is half n & 1 of tile t_begin + wave + (n >> 1) * PV_WAVES
  const int tiles = (kv_len + PV_BN - 1) / PV_BN;
  const int tps = (tiles + S - 1) / S;
  const int t_begin = split * tps;
  const int t_end = min(tiles, t_begin + tps);
  const int my_tiles =
      max(0, (t_end - t_begin - wave + PV_WAVES - 1) / PV_WAVES);
  auto k0_of = [&](int n) {
    return (t_begin + wave + (n >> 1) * PV_WAVES) * PV_BN + (n & 1) * PV_SUB;
  };
  int n_sub = 2 * my_tiles;
  // the second half of the last tile may lie wholly past the rows
  if (n_sub > 0 && k0_of(n_sub - 1) >= kv_len) --n_sub;

  short (&k_tile)[PV_SUB][D] =
      *reinterpret_cast<short (*)[PV_SUB][D]>(smem + wave * 2 * TILE);
  short (&v_tile)[PV_SUB][D] =
      *reinterpret_cast<short (*)[PV_SUB][D]>(smem + wave * 2 * TILE + TILE);

  const int* bt = block_table + (long long)b * max_pages;
  stage_t k_stage[NST], v_stage[NST];
  int pg_a = 0, pg_b = 0;  // the two pages of the step after the staged one

  // a page is looked up only if its first row is below kv_len <= cap, so
  // the index stays inside the table
  auto load_pages = [&](int n) {
    int a = 0, c = 0;
    if (n < n_sub) {
      const int k0 = k0_of(n);
      if (k0 < kv_len) a = bt[k0 / PV_PAGE];
      if (k0 + PV_PAGE < kv_len) c = bt[k0 / PV_PAGE + 1];
    }
    pg_a = min(max(a, 0), num_pages - 1);
    pg_b = min(max(c, 0), num_pages - 1);
  };
  auto load_sub = [&](int n) {
    const int k0 = k0_of(n);
#pragma unroll
    for (int j = 0; j < NST; ++j) {
      const int i = lane + 64 * j;
      const int r = i / CPR;
      const int c = (i % CPR) * 8;
      stage_t kv{}, vv{};
      if (k0 + r < kv_len) {
        const int page = j < NST / 2 ? pg_a : pg_b;
        const long long off =
            (((long long)page * Hkv + hkv) * PV_PAGE + (r % PV_PAGE)) * D + c;
        kv = *reinterpret_cast<const stage_t*>(Kc + off);
        vv = *reinterpret_cast<const stage_t*>(Vc + off);
      }
      k_stage[j] = kv;
      v_stage[j] = vv;
    }
  };

  if (n_sub > 0) {
    load_pages(0);
    load_sub(0);
    load_pages(1);
  }
  for (int n = 0; n < n_sub; ++n) {
#pragma unroll
    for (int j = 0; j < NST; ++j) {
      const int i = lane + 64 * j;
      const int r = i / CPR;
      const int c = (i % CPR) * 8;
      *reinterpret_cast<short8*>(&k_tile[r][k_swz(r, c)]) =
          pp_stage_bf16(k_stage[j]);
      *reinterpret_cast<short8*>(&v_tile[r][c]) = pp_stage_bf16(v_stage[j]);
    }
    if (n + 1 < n_sub) {
      load_sub(n + 1);
      load_pages(n + 2);
    }
    pv_wave_sync();
    const int k0 = k0_of(n);
    const f32x16 s_acc = s_tile(k_tile, 0, lane, hi, q_frag);
    const f32x16 p = softmax_step<DT>(s_acc, o_acc, m_run, l_run, k0, kv_len,
                                      true, gq, gq0, scale, hi);
    pv_tile(p, v_tile, 0, lane, hi, o_acc);
    pv_wave_sync();
  }

  // ---- merge the waves: 1..3 hand (m, l, O') to wave 0 through LDS ----
  float* mo = reinterpret_cast<float*>(smem);  // [w-1][DT][16][64]
  float* mm = mo + (PV_WAVES - 1) * DT * 16 * 64;  // [w][32]
  float* ml = mm + PV_WAVES * 32;                  // [w][32]
  const float m2 = m_run * L2E;  // log2 domain, as the reduce kernel reads
  __syncthreads();  // every wave is done with its tile memory
  if (hi == 0) {
    mm[wave * 32 + qcol] = m2;
    ml[wave * 32 + qcol] = l_run;
  }
  if (wave > 0) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        mo[(((wave - 1) * DT + dt) * 16 + r) * 64 + lane] = o_acc[dt][r];
  }
  __syncthreads();
  if (wave > 0) return;

  float M = m2;
#pragma unroll
  for (int w = 1; w < PV_WAVES; ++w) M = fmaxf(M, mm[w * 32 + qcol]);
  float a = pa_w(m2, M);
  float lsum = l_run * a;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[dt][r] *= a;
#pragma unroll
  for (int w = 1; w < PV_WAVES; ++w) {
    a = pa_w(mm[w * 32 + qcol], M);
    lsum += ml[w * 32 + qcol] * a;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        o_acc[dt][r] += mo[(((w - 1) * DT + dt) * 16 + r) * 64 + lane] * a;
  }

  // ---- epilogue: O[q][d] = O'[d][q]; accumulator regs r..r+3 are 4
  // adjacent output columns ----
  if (!has_out) return;
  if (S == 1) {
    float inv = (q_ok && lsum > 0.f) ? 1.f / lsum : 0.f;
    if constexpr (FP8) inv *= oscale;
    short* op = Out + row * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; r += 4) {
        const int d = 8 * (r >> 2) + 4 * hi + 32 * dt;
        short4v o4;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o4[e] = q_ok ? f2bf(o_acc[dt][r + e] * inv) : (short)0;
        *reinterpret_cast<short4v*>(op + d) = o4;
      }
  } else {
    // a column without a query is the neutral partial: M = -inf, l = 0
    float* op = ws_o + (row * S + split) * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; r += 4) {
        const int d = 8 * (r >> 2) + 4 * hi + 32 * dt;
        float4v o4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o4[e] = q_ok ? o_acc[dt][r + e] : 0.f;
          if constexpr (FP8) o4[e] *= oscale;
        }
        *reinterpret_cast<float4v*>(op + d) = o4;
      }
    if (hi == 0) {
      ws_ml[(row * S + split) * 2 + 0] = q_ok ? M : -INFINITY;
      ws_ml[(row * S + split) * 2 + 1] = q_ok ? lsum : 0.f;
    }
  }
}

// Fused verify-step RoPE + KV append: grid (Tq, B), one block per row.
// Row (b, i) sits at position p = pos0[b] + i. For pos0[b] >= 0 and
// i < q_lens[b] it is handled as rope_append_paged_kernel handles a row:
// q and k rotated (rotate-halves, fp32 tables), rotated k and raw v
// written to page block_table[b, p/PAGE] slot p%PAGE (pa_store8, so fp8
// pages hold pa_quant8 of the same bf16 values), rotated q to Qout
// [B, Tq, Hq, D]. Every other row, and a row whose p lies outside the
// rope tables or the block table, touches no cache and gets zero q. A
// page id outside the pool is not written; q is still rotated.
// q/k/v may be slices of a fused QKV row: *_bs / *_ts are the batch and
// token strides.
template <bool FP8>
__global__ __launch_bounds__(256) void rope_append_paged_multi_kernel(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, long long q_bs, long long q_ts,
    long long k_bs, long long k_ts, long long v_bs, long long v_ts,
    const float* __restrict__ cosT, const float* __restrict__ sinT,
    const int* __restrict__ pos0, const int* __restrict__ q_lens,
    const int* __restrict__ block_table, void* __restrict__ Kc,
    void* __restrict__ Vc, short* __restrict__ Qout, int Hq, int Hkv, int D,
    int table_rows, int num_pages, int max_pages, float k_inv, float v_inv) {
  const int i = blockIdx.x, Tq = gridDim.x;
  const int b = blockIdx.y;
  const int half = D / 2;
  const int hc = half / 8;  // 16-byte chunks per half row
  const int p0 = pos0[b];
  const long long p = (long long)p0 + i;
  short* qo = Qout + ((long long)b * Tq + i) * Hq * D;
  if (p0 < 0 || i >= q_lens[b] || p >= table_rows ||
      p / PV_PAGE >= max_pages) {
    const short8 zero = short8{0, 0, 0, 0, 0, 0, 0, 0};
    for (int w = threadIdx.x; w < Hq * (D / 8); w += blockDim.x)
      *reinterpret_cast<short8*>(qo + w * 8) = zero;
    return;
  }
  const int page = block_table[(long long)b * max_pages + p / PV_PAGE];
  const bool page_ok = page >= 0 && page < num_pages;
  const int slot = (int)(p % PV_PAGE);
  const float* cr = cosT + p * half;
  const float* sr = sinT + p * half;
  const short* qr = Q + b * q_bs + i * q_ts;
  const short* kr = K + b * k_bs + i * k_ts;
  const short* vr = V + b * v_bs + i * v_ts;
  const int n_q = Hq * hc, n_k = Hkv * hc, n_v = Hkv * (D / 8);
  for (int w = threadIdx.x; w < n_q + n_k + n_v; w += blockDim.x) {
    if (w < n_q + n_k) {
      const bool is_q = w < n_q;
      if (!is_q && !page_ok) continue;
      const int u = is_q ? w : w - n_q;
      const int h = u / hc, c = (u % hc) * 8;
      const short* src = (is_q ? qr : kr) + h * D;
      const short8 x1 = *reinterpret_cast<const short8*>(src + c);
      const short8 x2 = *reinterpret_cast<const short8*>(src + half + c);
      short8 y1, y2;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float a = bf2f(x1[j]), bb = bf2f(x2[j]);
        const float cs = cr[c + j], sn = sr[c + j];
        y1[j] = f2bf(a * cs - bb * sn);
        y2[j] = f2bf(bb * cs + a * sn);
      }
      if (is_q) {
        *reinterpret_cast<short8*>(qo + h * D + c) = y1;
        *reinterpret_cast<short8*>(qo + h * D + half + c) = y2;
      } else {
        const long long off =
            (((long long)page * Hkv + h) * PV_PAGE + slot) * D;
        pa_store8<FP8>(Kc, off + c, y1, k_inv);
        pa_store8<FP8>(Kc, off + half + c, y2, k_inv);
      }
    } else if (page_ok) {
      const int u = w - n_q - n_k;
      const int h = u / (D / 8), c = (u % (D / 8)) * 8;
      pa_store8<FP8>(
          Vc, (((long long)page * Hkv + h) * PV_PAGE + slot) * D + c,
          *reinterpret_cast<const short8*>(vr + h * D + c), v_inv);
    }
  }
}
