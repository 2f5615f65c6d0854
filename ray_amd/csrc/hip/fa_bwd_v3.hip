// Flash-attention backward v3: dv/dk kernels restructured with the
// v6-forward toolkit (guide §5.5): K (and V) register-resident per
// wave — no K tile in LDS at all — q/dO staged in 64-row
// double-buffered LDS tiles with the async-STAGE split (next tile's
// global loads issue before this tile's compute), XOR-swizzled
// ds_read_b128 on every row-read path, one __syncthreads per 64-q
// tile. The GQA head loop and q-tile loop
// are flattened into one iteration space so the software pipeline
// runs across head boundaries.
//
// Math (FA2-style split, Dao 2023 §3, no atomics): S' = K·Q^T on
// mfma_f32_32x32x16_bf16 puts the softmax row (a fixed q) in ONE lane
// column, so P^T = exp(S'·s − lse[q]) and dS̃^T = P^T ⊙ (dP^T − D[q])·s
// are register-local elementwise ops; dP^T = V·dO^T has the same shape.
// dV += P^T·dO and dK += dS̃^T·Q need a true 32x32 lane transpose, done
// through a per-wave padded LDS scratch tile.
//
// The MFMA lane layouts are in fa_tile.h.
#include "fa_bwd_frag.h"

// ---------------------------------------------------------------------
// dK (DK = true) or dV (DK = false) of 128 key rows: grid (T/128, B*Hkv),
// 4 waves x 32 kv rows; K in registers, the output accumulates in
// registers.
//   dv[k][d] = sum_q P^T[k][q] dO[q][d]
//   dk[k][d] = sum_q dS̃^T[k][q] Q[q][d]
// dK also holds V in registers for dP^T = V·dO^T and stages Dsum; its
// second product reads q_lds where dV's reads do_lds. Two kernels, not
// one, so that each fits 2 waves/SIMD.
// ---------------------------------------------------------------------
template <bool DK>
__global__ __launch_bounds__(256) void fa_bwd_dkv_v3_bf16(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ Dsum,
    short* __restrict__ dKV, int B, int Hq, int Hkv, int T, int causal,
    float scale) {
  __shared__ short q_lds[2][FB3_QT][FB3_D];
  __shared__ short do_lds[2][FB3_QT][FB3_D];
  __shared__ float lse_lds[2][FB3_QT];
  __shared__ float dsum_lds[2][FB3_QT];  // DK only: unused, it costs no LDS
  __shared__ short scratch[4][32][40];

  const int k0 = blockIdx.x * 128;
  const int bh = blockIdx.y;
  const int b = bh / Hkv;
  const int hkv = bh % Hkv;
  const int rep = Hq / Hkv;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int hi = lane >> 5;
  const int a_off = 8 * hi;

  const long long kbase = (((long long)b * Hkv + hkv) * T + k0) * FB3_D;
  // K (and V) register-resident: only this wave's own 32 rows are ever read
  bf16x8 k_frag[8], v_frag[8];
  {
    const short* kp = K + kbase + ((long long)32 * wave + (lane & 31)) * FB3_D;
    const short* vp = V + kbase + ((long long)32 * wave + (lane & 31)) * FB3_D;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      k_frag[c] = ld8(kp + 16 * c + a_off);
      if constexpr (DK) v_frag[c] = ld8(vp + 16 * c + a_off);
    }
  }

  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x16{};
  const float L2E = 1.4426950408889634f;

  const int q_start = causal ? k0 : 0;
  const int nq = (T - q_start + FB3_QT - 1) / FB3_QT;
  const int n_tiles = rep * nq;

  // Staging of tile t_idx of the flattened (head, q-tile) sequence: 64 rows
  // x 16 chunks / 256 threads = 4 chunks per tensor; chunk j of a thread is
  // row r, columns c .. c+7 of the tile.
#define FB3_TILE_BASE(t_idx)                                              \
  const int g_ = (t_idx) / nq;                                            \
  const int q0_ = q_start + ((t_idx) % nq) * FB3_QT;                      \
  const int hq_ = hkv * rep + g_;                                         \
  const long long qb_ = (((long long)b * Hq + hq_) * T) * FB3_D;          \
  const long long lb_ = ((long long)b * Hq + hq_) * T;
#define FB3_CHUNK(j)                                                      \
  int i = threadIdx.x + 256 * (j);                                        \
  int r = i >> 4;                                                         \
  int c = (i & 15) * 8;
  // global -> qv, dv (zero past T)
#define FB3_CHUNK_LOAD(j)                                                 \
  FB3_CHUNK(j)                                                            \
  int qrow = q0_ + r;                                                     \
  short8 qv{0, 0, 0, 0, 0, 0, 0, 0}, dv{0, 0, 0, 0, 0, 0, 0, 0};          \
  if (qrow < T) {                                                         \
    qv = *reinterpret_cast<const short8*>(qb_ + Q +                       \
                                          (long long)qrow * FB3_D + c);   \
    dv = *reinterpret_cast<const short8*>(qb_ + dO +                      \
                                          (long long)qrow * FB3_D + c);   \
  }
#define FB3_CHUNK_WRITE(buf, qv_, dv_)                                    \
  int csw = c ^ ((r & 7) << 3);                                           \
  *reinterpret_cast<short8*>(&q_lds[buf][r][csw]) = qv_;                  \
  *reinterpret_cast<short8*>(&do_lds[buf][r][csw]) = dv_;

  // dV stages through registers: the next tile's global loads are issued
  // before this tile's compute (LOAD) and written after it (WRITE).
  short8 q_stage[4], do_stage[4];
  float lse_stage = 0.f;
#define FB3_DV_LOAD(t_idx)                                                \
  do {                                                                    \
    FB3_TILE_BASE(t_idx)                                                  \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                       \
      FB3_CHUNK_LOAD(j)                                                   \
      q_stage[j] = qv;                                                    \
      do_stage[j] = dv;                                                   \
    }                                                                     \
    if (threadIdx.x < FB3_QT) {                                           \
      int qrow = q0_ + threadIdx.x;                                       \
      lse_stage = (qrow < T) ? LSE[lb_ + qrow] : INFINITY;                \
    }                                                                     \
  } while (0)
#define FB3_DV_WRITE(buf)                                                 \
  do {                                                                    \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                       \
      FB3_CHUNK(j)                                                        \
      FB3_CHUNK_WRITE(buf, q_stage[j], do_stage[j])                       \
    }                                                                     \
    if (threadIdx.x < FB3_QT) lse_lds[buf][threadIdx.x] = lse_stage;      \
  } while (0)
  // dk holds K AND V register-resident plus the dK accumulators —
  // reg-staged async loads (like dv's) push it to 289 regs = 1
  // wave/SIMD (measured: the whole-bwd regression). Stage DIRECTLY
  // global->LDS into the double buffer instead: minimal register
  // liveness, still one barrier per 64-row tile.
#define FB3_DK_STAGE(t_idx, buf)                                          \
  do {                                                                    \
    FB3_TILE_BASE(t_idx)                                                  \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                       \
      FB3_CHUNK_LOAD(j)                                                   \
      FB3_CHUNK_WRITE(buf, qv, dv)                                        \
    }                                                                     \
    if (threadIdx.x < FB3_QT) {                                           \
      int qrow = q0_ + threadIdx.x;                                       \
      lse_lds[buf][threadIdx.x] = (qrow < T) ? LSE[lb_ + qrow] : INFINITY; \
      dsum_lds[buf][threadIdx.x] = (qrow < T) ? Dsum[lb_ + qrow] : 0.f;   \
    }                                                                     \
  } while (0)

  if constexpr (DK) {
    FB3_DK_STAGE(0, 0);
  } else {
    FB3_DV_LOAD(0);
    FB3_DV_WRITE(0);
  }
  __syncthreads();

  for (int t = 0; t < n_tiles; ++t) {
    const int cur = t & 1;
    const int q0s = q_start + (t % nq) * FB3_QT;
    if (t + 1 < n_tiles) {
      if constexpr (DK) FB3_DK_STAGE(t + 1, cur ^ 1);
      else FB3_DV_LOAD(t + 1);
    }

#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int qts = q0s + 32 * qt;
      if (qts >= T) break;
      if (causal && k0 + 32 * wave > qts + 31) continue;

      f32x16 s_acc{}, dp_acc{};
      {
        const int rr = 32 * qt + (lane & 31);
        const short* qrow = &q_lds[cur][rr][0];
        const short* dorow = &do_lds[cur][rr][0];
        const int sw = (rr & 7) << 3;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          // S'^T tile: A = this wave's K rows (regs), B = Q^T from LDS;
          // dP^T likewise from V and dO^T
          bf16x8 qf = ld8(qrow + ((16 * c + a_off) ^ sw));
          bf16x8 dof;
          if constexpr (DK) dof = ld8(dorow + ((16 * c + a_off) ^ sw));
          s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k_frag[c], qf,
                                                          s_acc, 0, 0, 0);
          if constexpr (DK)
            dp_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                v_frag[c], dof, dp_acc, 0, 0, 0);
        }
      }
      // C layout: col = lane&31 = q (this lane's loaded q row),
      // rows = this wave's k
      const int gq = qts + (lane & 31);
      const float lse_q = lse_lds[cur][32 * qt + (lane & 31)];
      float d_q = 0.f;
      if constexpr (DK) d_q = dsum_lds[cur][32 * qt + (lane & 31)];
      const bool full_tile = !causal || (k0 + 32 * wave + 31 <= qts);
      short(*scr)[40] = scratch[wave];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        // c_row spelled out: the call changes this loop's code
        int gk = k0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * hi;
        float pv = __builtin_amdgcn_exp2f(
            __builtin_fmaf(s_acc[r] * scale, L2E, -lse_q * L2E));
        if (!full_tile && gk > gq) pv = 0.f;
        if constexpr (DK) pv = pv * (dp_acc[r] - d_q) * scale;  // dS̃
        scr[c_row(r, hi)][lane & 31] = f2bf(pv);
      }
      __builtin_amdgcn_s_waitcnt(0);
      // second product: B = Q (dK) or dO (dV), gathered by column
      const short(*src)[FB3_D] = DK ? q_lds[cur] : do_lds[cur];
#pragma unroll
      for (int qc = 0; qc < 2; ++qc) {
        bf16x8 af = __builtin_bit_cast(
            bf16x8, *reinterpret_cast<const short8*>(
                            &scr[lane & 31][16 * qc + a_off]));
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          short tmp[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            int row = 32 * qt + 16 * qc + a_off + i;
            int col = 32 * dt + (lane & 31);
            tmp[i] = src[row][col ^ ((row & 7) << 3)];
          }
          bf16x8 bf = __builtin_bit_cast(
              bf16x8, *reinterpret_cast<short8*>(tmp));
          acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              af, bf, acc[dt], 0, 0, 0);
        }
      }
    }

    if constexpr (!DK) {
      if (t + 1 < n_tiles) FB3_DV_WRITE(cur ^ 1);
    }
    __syncthreads();
  }
#undef FB3_TILE_BASE
#undef FB3_CHUNK
#undef FB3_CHUNK_LOAD
#undef FB3_CHUNK_WRITE
#undef FB3_DV_LOAD
#undef FB3_DV_WRITE
#undef FB3_DK_STAGE

  c_store(acc, dKV + kbase + (long long)wave * 32 * FB3_D, FB3_D, lane, hi);
}

// the two instances ops.hip launches, so that this file emits them when
// it is compiled on its own
template __global__ void fa_bwd_dkv_v3_bf16<false>(
    const short*, const short*, const short*, const short*, const float*,
    const float*, short*, int, int, int, int, int, float);
template __global__ void fa_bwd_dkv_v3_bf16<true>(
    const short*, const short*, const short*, const short*, const float*,
    const float*, short*, int, int, int, int, int, float);

// ---------------------------------------------------------------------
// dQ v3: grid (T/128, B*Hq), 4 waves x 32 q rows; 32-row K/V tiles
// double-buffered with direct global->LDS staging (one barrier per
// tile), XOR-swizzled row reads, cvt_pk+permlane dS
// exchange.  dQ[q][d] += sum_k dS^T[k][q] K[k][d]
// ---------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(256) void fa_bwd_dq_v3_bf16(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ Dsum,
    short* __restrict__ dQ, int B, int Hq, int Hkv, int T, int causal,
    float scale, int bthd) {
  __shared__ short k_lds[2][32][FB3_D];
  __shared__ short v_lds[2][32][FB3_D];

  const int q0 = blockIdx.x * 128;
  const int bh = blockIdx.y;
  const int b = bh / Hq;
  const int hq = bh % Hq;
  const int hkv = hq / (Hq / Hkv);
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int hi = lane >> 5;
  const int a_off = 8 * hi;

  const long long q_rs = bthd ? (long long)Hq * FB3_D : FB3_D;
  const long long kv_rs = bthd ? (long long)Hkv * FB3_D : FB3_D;
  const long long qbase =
      bthd ? (((long long)b * T + q0) * Hq + hq) * FB3_D
           : (((long long)b * Hq + hq) * T + q0) * FB3_D;
  const long long kbase =
      bthd ? ((long long)b * T * Hkv + hkv) * FB3_D
           : (((long long)b * Hkv + hkv) * T) * FB3_D;
  const int my_q = q0 + wave * 32 + (lane & 31);

  bf16x8 q_frag[8], do_frag[8];
  {
    const short* qp = Q + qbase + ((long long)wave * 32 + (lane & 31)) * q_rs;
    const short* dp = dO + qbase + ((long long)wave * 32 + (lane & 31)) * q_rs;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      q_frag[c] = ld8(qp + 16 * c + a_off);
      do_frag[c] = ld8(dp + 16 * c + a_off);
    }
  }
  const float L2E = 1.4426950408889634f;
  const float lse_q = LSE[((long long)b * Hq + hq) * T + my_q];
  const float d_q = Dsum[((long long)b * Hq + hq) * T + my_q];

  f32x16 dq_acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) dq_acc[t] = f32x16{};

  const int wave_k_max = q0 + wave * 32 + 31;  // last k this wave needs
  const int k_end = causal ? min(T, q0 + 128) : T;
  const int n_tiles = (k_end + 31) / 32;

  // 32 rows x 16 chunks = 512 chunks / 256 threads = 2 per tensor
#define FB3_DQ_STAGE(t_idx, buf)                                          \
  do {                                                                    \
    const int kt0 = (t_idx) * 32;                                         \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                       \
      int i = threadIdx.x + 256 * j;                                      \
      int r = i >> 4;                                                     \
      int c = (i & 15) * 8;                                               \
      int csw = c ^ ((r & 7) << 3);                                       \
      *reinterpret_cast<short8*>(&k_lds[buf][r][csw]) =                   \
          *reinterpret_cast<const short8*>(                               \
              K + kbase + (long long)(kt0 + r) * kv_rs + c);              \
      *reinterpret_cast<short8*>(&v_lds[buf][r][csw]) =                   \
          *reinterpret_cast<const short8*>(                               \
              V + kbase + (long long)(kt0 + r) * kv_rs + c);              \
    }                                                                     \
  } while (0)

  FB3_DQ_STAGE(0, 0);
  __syncthreads();

  for (int t = 0; t < n_tiles; ++t) {
    const int cur = t & 1;
    const int k0 = t * 32;
    if (t + 1 < n_tiles) FB3_DQ_STAGE(t + 1, cur ^ 1);

    if (!(causal && k0 > wave_k_max)) {
      // S' = K·Q^T and dP^T = V·dO^T (both [k][q], lane owns column q)
      f32x16 s_acc{}, dp_acc{};
      {
        const int rr = lane & 31;
        const short* krow = &k_lds[cur][rr][0];
        const short* vrow = &v_lds[cur][rr][0];
        const int sw = (rr & 7) << 3;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          bf16x8 kf = ld8(krow + ((16 * c + a_off) ^ sw));
          bf16x8 vf = ld8(vrow + ((16 * c + a_off) ^ sw));
          s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, q_frag[c],
                                                          s_acc, 0, 0, 0);
          dp_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, do_frag[c],
                                                           dp_acc, 0, 0, 0);
        }
      }

      f32x16 ds;
      const bool full_tile = !causal || (k0 + 31 <= q0 + wave * 32);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        // c_row spelled out: the call changes this loop's code
        int gk = k0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        float p = __builtin_amdgcn_exp2f(
            __builtin_fmaf(s_acc[r] * scale, L2E, -lse_q * L2E));
        if (!full_tile && (causal && gk > my_q)) p = 0.f;
        ds[r] = p * (dp_acc[r] - d_q) * scale;
      }

      // dS A-fragments via pack_swap, then dQ += dS·K
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        bf16x8 af = pack_swap<true>(ds, kc);
        {
          const int gl = lane & 15;
          const int grp16 = (lane >> 4) & 1;
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            // ld_tr8 spelled out: the call changes this loop's code
            short ktmp[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              int row = 16 * kc + a_off + 4 * h + (gl >> 2);
              int col = (32 * dt + 16 * grp16 + 4 * (gl & 3))
                        ^ ((row & 7) << 3);
              auto p = (__attribute__((address_space(3))) short4v*)
                  &k_lds[cur][row][col];
              short4v r4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(p);
#pragma unroll
              for (int j = 0; j < 4; ++j) ktmp[4 * h + j] = r4[j];
            }
            bf16x8 bf = __builtin_bit_cast(
                bf16x8, *reinterpret_cast<short8*>(ktmp));
            dq_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                af, bf, dq_acc[dt], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }

  // c_store spelled out: the call changes the tile loop's code
  short* out = dQ + qbase + (long long)wave * 32 * q_rs;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int qrow = (r & 3) + 8 * (r >> 2) + 4 * hi;
      out[(long long)qrow * q_rs + 32 * dt + (lane & 31)] =
          f2bf(dq_acc[dt][r]);
    }
}
