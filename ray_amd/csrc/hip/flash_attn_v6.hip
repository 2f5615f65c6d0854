// Flash-attention forward v6: the guide's 8-wave ladder structure
// (§B "8-warp 32x32 ladder": dbuf + async-STAGE + K XOR-swizzle +
// cvt_pk/permlane P exchange + defer-max) on the swapped-operand tile
// math of fa_tile.h, which also has the fragment layouts.
//
// Structure per block: 8 waves x 32 query rows = 256 q/block;
// K/V tiles of 64 rows double-buffered in LDS. Per tile iteration:
//   1. issue next tile's global loads into registers (async-STAGE
//      split: HBM latency hides under this tile's compute)
//   2. per 32-row sub-tile: s_tile (K read from swizzled LDS),
//      softmax_step, pv_tile (V^T by ds_read_tr16_b64)
//   3. ds_write staged registers into the other buffer; one
//      __syncthreads per tile.
#include "fa_tile.h"

#define FA6_D 128
#define FA6_QW 32         // query rows per wave
#define FA6_WAVES 8
#define FA6_BM (FA6_QW * FA6_WAVES)  // 256 q rows per block
#define FA6_BN 64         // staged K/V rows per tile
#define FA6_THREADS (FA6_WAVES * 64)

extern "C" __global__ __launch_bounds__(FA6_THREADS) void
flash_attn_fwd_v6_bf16(const short* __restrict__ Q,
                       const short* __restrict__ K,
                       const short* __restrict__ V, short* __restrict__ O,
                       float* __restrict__ LSE, int B, int Hq, int Hkv,
                       int T, int Tk, int causal, int q_offset,
                       float scale, int bthd, int q_rs_, int o_rs_,
                       int kv_rs_) {
  // bthd=1: Q/K/V/O are token-row storage (the model's natural layout:
  // [B,T,H,D], or the q/k/v column sections of one packed [B,T,rs] GEMM
  // output); q_rs, o_rs and kv_rs are the token-row strides in elements
  // of Q, of O and of K/V, each >= H*D. bthd=0: contiguous [B,H,T,D],
  // all three strides are D. They are 32-bit arguments: a row offset is
  // then one 32 x 32 -> 64-bit multiply-add.
  __shared__ short k_lds[2][FA6_BN][FA6_D];
  __shared__ short v_lds[2][FA6_BN][FA6_D];

  // heaviest causal block (the last query rows) first: the light blocks
  // fill the tail of the grid
  const int q0 = (gridDim.x - 1 - blockIdx.x) * FA6_BM;
  const int bh = blockIdx.y;
  const int b = bh / Hq;
  const int hq = bh % Hq;
  const int hkv = hq / (Hq / Hkv);
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int qcol = lane & 31;
  const int hi = lane >> 5;
  const int a_off = 8 * hi;

  const long long q_rs = q_rs_, o_rs = o_rs_, kv_rs = kv_rs_;
  const long long qbase =
      bthd ? ((long long)b * T + q0) * q_rs + hq * FA6_D
           : (((long long)b * Hq + hq) * T + q0) * FA6_D;
  const long long obase =
      bthd ? ((long long)b * T + q0) * o_rs + hq * FA6_D : qbase;
  const long long kbase =
      bthd ? (long long)b * Tk * kv_rs + hkv * FA6_D
           : (((long long)b * Hkv + hkv) * Tk) * FA6_D;
  const int my_q = q0 + wave * FA6_QW + qcol;
  const int gq = q_offset + my_q;                  // causal-global index
  const int wave_gq_min = q_offset + q0 + wave * FA6_QW;
  const int wave_gq_max = wave_gq_min + FA6_QW - 1;

  // Q fragments (B operand): lane reads its own query row
  bf16x8 q_frag[8];
  {
    const short* qp = Q + qbase + ((long long)wave * FA6_QW + qcol) * q_rs;
#pragma unroll
    for (int c = 0; c < 8; ++c) q_frag[c] = ld8(qp + 16 * c + a_off);
  }

  f32x16 o_acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) o_acc[t] = f32x16{};
  float m_run = -INFINITY, l_run = 0.f;

  const int k_end =
      causal ? min(Tk, q_offset + q0 + FA6_BM) : Tk;
  const int n_tiles = (k_end + FA6_BN - 1) / FA6_BN;

  // each thread stages 2 short8 chunks per tensor per tile:
  // 64 rows x 16 chunks = 1024 chunks / 512 threads
  short8 k_stage[2], v_stage[2];

#define FA6_LOAD_TILE(t_idx)                                              \
  do {                                                                    \
    const int kt0 = (t_idx)*FA6_BN;                                       \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                       \
      int i = threadIdx.x + FA6_THREADS * j;                              \
      int r = i >> 4;                                                     \
      int c = (i & 15) * 8;                                               \
      int krow = kt0 + r;                                                 \
      short8 kv{0, 0, 0, 0, 0, 0, 0, 0}, vv{0, 0, 0, 0, 0, 0, 0, 0};      \
      if (krow < Tk) {                                                    \
        kv = *reinterpret_cast<const short8*>(                            \
            K + kbase + (long long)krow * kv_rs + c);                     \
        vv = *reinterpret_cast<const short8*>(                            \
            V + kbase + (long long)krow * kv_rs + c);                     \
      }                                                                   \
      k_stage[j] = kv;                                                    \
      v_stage[j] = vv;                                                    \
    }                                                                     \
  } while (0)

#define FA6_WRITE_TILE(buf)                                               \
  do {                                                                    \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                       \
      int i = threadIdx.x + FA6_THREADS * j;                              \
      int r = i >> 4;                                                     \
      int c = (i & 15) * 8;                                               \
      *reinterpret_cast<short8*>(&k_lds[buf][r][k_swz(r, c)]) =           \
          k_stage[j];                                                     \
      *reinterpret_cast<short8*>(&v_lds[buf][r][c]) = v_stage[j];         \
    }                                                                     \
  } while (0)

  // prologue: stage tile 0
  FA6_LOAD_TILE(0);
  FA6_WRITE_TILE(0);
  __syncthreads();

  for (int t = 0; t < n_tiles; ++t) {
    const int cur = t & 1;
    const int k0 = t * FA6_BN;
    if (t + 1 < n_tiles) FA6_LOAD_TILE(t + 1);

    const bool wave_active = !causal || (k0 <= wave_gq_max);
    if (wave_active) {
      // att[2]-style pipeline (T15): BOTH sub-tiles' S'=K·Q^T MFMAs
      // issue up front, so sub-tile 1's matrix work fills the MFMA
      // pipe while sub-tile 0's softmax runs on the VALU pipe (the
      // pipes are independent; m114).
      const bool do0 =
          (k0 < k_end) && !(causal && k0 > wave_gq_max);
      const bool do1 =
          (k0 + 32 < k_end) && !(causal && k0 + 32 > wave_gq_max);

      auto softmax_pv = [&](int kt, f32x16 s_acc) {
        const f32x16 p =
            softmax_step<4>(s_acc, o_acc, m_run, l_run, k0 + 32 * kt, Tk,
                             causal, gq, wave_gq_min, scale, hi);
        pv_tile(p, v_lds[cur], kt, lane, hi, o_acc);
      };

      f32x16 sA{}, sB{};
      if (do0) sA = s_tile(k_lds[cur], 0, lane, hi, q_frag);
      // in flight under sub-tile 0's softmax
      if (do1) sB = s_tile(k_lds[cur], 1, lane, hi, q_frag);
      if (do0) softmax_pv(0, sA);
      if (do1) softmax_pv(1, sB);
    }    // wave_active

    if (t + 1 < n_tiles) {
      FA6_WRITE_TILE(cur ^ 1);
    }
    __syncthreads();
  }

  // ---- epilogue: O[q][d] = O'[d][q] / l ----
  float inv = (l_run > 0.f) ? 1.f / l_run : 0.f;
  if (my_q < T) {
    short* op = O + obase + ((long long)wave * FA6_QW + qcol) * o_rs;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int d = (r & 3) + 8 * (r >> 2) + 4 * hi + 32 * dt;
        op[d] = f2bf(o_acc[dt][r] * inv);
      }
  }
  if (LSE != nullptr && hi == 0 && my_q < T) {
    LSE[((long long)b * Hq + hq) * T + my_q] =
        (l_run > 0.f) ? m_run + __logf(l_run) : -INFINITY;
  }
}
