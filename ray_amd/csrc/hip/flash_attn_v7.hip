// Flash-attention forward v7: the 256-row kernel (8 waves x 32 query rows,
// 64-row K/V tiles, swapped K·Q^T, tr16 reads for V^T) on a two-phase
// ping-pong schedule. The arithmetic is that of fa_tile.h's s_tile,
// softmax_step and pv_tile, operation for operation, in the order of its
// "Two-phase form".
//
// A wave's work on tile t is cut into
//   V(t): softmax of both 32-key sub-tiles -> packed P. VALU only; the
//         wave also stages its share of the coming K/V tiles here (global
//         loads at the head, ds_write at the end).
//   M(t): P·V of tile t, then S' = K·Q^T of tile t+1. Every MFMA and every
//         LDS read; operands are read into registers ahead of their MFMAs.
// with one barrier after each phase. Waves 4-7 run one phase behind waves
// 0-3 (waves w and w+4 share a SIMD), so on every SIMD one wave is in M
// while its partner is in V:
//   interval   -1     0      1      2      3
//   waves 0-3  S(0)   V(0)   M(0)   V(1)   M(1) ...
//   waves 4-7  stage  S(0)   V(0)   M(0)   V(1) ...
// M(t) reads V(t) and K(t+1), in intervals 2t+1 (waves 0-3) and 2t+2
// (waves 4-7). Their successors V(t+1) and K(t+2) go to the other buffers
// in exactly those two intervals: waves 4-7 write them in V(t) (interval
// 2t+1), waves 0-3 in V(t+1) (interval 2t+2). Those buffers held V(t-1) and
// K(t), last read in interval 2t. Two buffers per tensor suffice.
//
// Tiles that no wave has to mask (below the causal diagonal, inside Tk) run
// in a loop without tests, except the wave-uniform skip of the O rescale.
// The diagonal tiles and a ragged tail run through the same two phases with
// the mask applied by select; waves wholly above the diagonal skip their
// compute and keep their barriers.
#include <type_traits>

#include "fa_bwd_lds_layout.h"
#include "fa_tile.h"

#define FA7_D 128
#define FA7_QW 32                    // query rows per wave
#define FA7_BM 256                   // query rows per block
#define FA7_BN 64                    // staged K/V rows per tile
#define FA7_THREADS 512
#define FA7_IMG (FA7_BN * FA7_D)     // elements of one tile image
#define FA7_EP_STRIDE 136            // epilogue row: 256 B + 16 B pad

extern "C" __global__ __launch_bounds__(FA7_THREADS) void
flash_attn_fwd_v7_bf16(const short* __restrict__ Q,
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
  //
  // K and V double buffers, then the epilogue's per-wave [32][136] images.
  // The epilogue has memory of its own: waves 0-3 reach it while waves 4-7
  // still read the last V tile.
  __shared__ __attribute__((aligned(16))) short
      smem[4 * FA7_IMG + 8 * FA7_QW * FA7_EP_STRIDE];
  short* const k_lds = smem;                // [2][64 x 128]
  short* const v_lds = smem + 2 * FA7_IMG;  // [2][64 x 128]
  short* const ep_lds = smem + 4 * FA7_IMG;

  // Heavy causal blocks (the last query rows) before light ones inside
  // every row of the grid, and the order rotated from row to row.
  // Workgroups go to the 8 XCDs round-robin in dispatch order, so with a
  // fixed order and gridDim.x a multiple of 8 one XCD gets the heaviest
  // query block of every head and another the lightest (96 against 40
  // tiles per head at T 4096): the kernel then lasts as long as the
  // heaviest XCD. Rotated, every XCD sees every weight equally often, and
  // the blocks of one head still run together and share K/V in the L2.
  const int qb = (blockIdx.x + blockIdx.y) % gridDim.x;
  const int q0 = (gridDim.x - 1 - qb) * FA7_BM;
  const int bh = blockIdx.y;
  const int b = bh / Hq;
  const int hq = bh % Hq;
  const int hkv = hq / (Hq / Hkv);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar
  const int grp = wave >> 2;  // 0: leading waves, 1: one phase behind
  const int lane = tid & 63;
  const int qcol = lane & 31;
  const int hi = lane >> 5;
  const int a_off = 8 * hi;

  const long long q_rs = q_rs_, o_rs = o_rs_, kv_rs = kv_rs_;
  const long long qbase =
      bthd ? ((long long)b * T + q0) * q_rs + hq * FA7_D
           : (((long long)b * Hq + hq) * T + q0) * FA7_D;
  const long long obase =
      bthd ? ((long long)b * T + q0) * o_rs + hq * FA7_D : qbase;
  const long long kbase =
      bthd ? (long long)b * Tk * kv_rs + hkv * FA7_D
           : (((long long)b * Hkv + hkv) * Tk) * FA7_D;
  const int my_q = q0 + wave * FA7_QW + qcol;
  const int gq = q_offset + my_q;                  // causal-global index
  const int wave_gq_max = q_offset + q0 + wave * FA7_QW + FA7_QW - 1;

  // Q fragments (B operand): lane reads its own query row
  bf16x8 q_frag[8];
  {
    const short* qp = Q + qbase + ((long long)wave * FA7_QW + qcol) * q_rs;
#pragma unroll
    for (int c = 0; c < 8; ++c) q_frag[c] = ld8(qp + 16 * c + a_off);
  }

  f32x16 o_acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) o_acc[t] = f32x16{};
  float m_run = -INFINITY, l_run = 0.f;

  const int k_end = causal ? min(Tk, q_offset + q0 + FA7_BM) : Tk;
  const int n_tiles = (k_end + FA7_BN - 1) / FA7_BN;
  // tiles that no wave masks: k0 + 64 <= Tk and k0 + 63 <= q_offset + q0
  int n_full = Tk / FA7_BN;
  if (causal) n_full = min(n_full, max(q_offset + q0 + 1, 0) / FA7_BN);
  // the test-free loop: V(t) unmasked, M(t) runs S(t+1), and the tiles it
  // loads (up to t+3) lie wholly inside Tk
  const int n_fast =
      max(0, min(min(n_full, n_tiles - 1), Tk / FA7_BN - 3));

  // a sub-tile is computed unless it starts at or past k_end or lies
  // wholly above the wave's diagonal
  auto sub_on = [&](int k0s) {
    return (k0s < k_end) && !(causal && k0s > wave_gq_max);
  };

  // staging: 64 rows x 16 chunks = 1024 chunks / 512 threads = 2 per tensor
  const int st_r = tid >> 4;  // + 32 j
  const int st_c = tid & 15;
  const int st_o = fb6_off(st_r, st_c);  // + 4096 j
  const int rb0 = fb6_rbase(lane, 0), rb1 = fb6_rbase(lane, 1);
  const int tb0 = fa_pv_tbase(lane, 0), tb1 = fa_pv_tbase(lane, 1);

  // Rows at or past Tk are staged as zeros and never read from memory: a
  // masked P of 0 times a NaN V would be NaN. GUARD = false is for tiles
  // known to lie inside Tk.
#define FA7_LOAD(SRC, st, tile, GUARD)                                    \
  do {                                                                    \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                       \
      const int krow = (tile)*FA7_BN + st_r + 32 * j;                     \
      short8 x_{0, 0, 0, 0, 0, 0, 0, 0};                                  \
      if (!(GUARD) || ((tile) < n_tiles && krow < Tk))                    \
        x_ = *reinterpret_cast<const short8*>(                            \
            SRC + kbase + (long long)krow * kv_rs + 8 * st_c);            \
      st[j] = x_;                                                         \
    }                                                                     \
  } while (0)
#define FA7_WRITE(dst, st, tile)                                          \
  do {                                                                    \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                         \
      *reinterpret_cast<short8*>(dst + ((tile)&1) * FA7_IMG + st_o +      \
                                 4096 * j) = st[j];                       \
  } while (0)

  f32x16 sA{}, sB{};         // S' of the two sub-tiles of the coming V phase
  bf16x8 pb0[2], pb1[2];     // packed P of the two sub-tiles
  bool need1 = false;        // sub-tile 1's O rescale, applied in M
  float sc1 = 1.f;

  // Staged rows travel in registers for a whole tile: a V phase writes
  // what the previous V phase loaded, then loads for the next one. Half a
  // tile does not cover the latency of a K/V row that misses the L2.
  short8 k_st[2], v_st[2];

  // V(t): scores -> packed P; write V(t + grp) and K(t + 1 + grp) to LDS
  // and load their successors.
  auto phase_v = [&](auto fast_c, int t) {
    constexpr bool FAST = decltype(fast_c)::value;
    const int k0 = t * FA7_BN;
    const int tv = t + grp, tk = t + 1 + grp;
    if (FAST || tv < n_tiles) FA7_WRITE(v_lds, v_st, tv);
    if (FAST || tk < n_tiles) FA7_WRITE(k_lds, k_st, tk);
    FA7_LOAD(V, v_st, tv + 1, !FAST);
    FA7_LOAD(K, k_st, tk + 1, !FAST);
    need1 = false;
    if (FAST || sub_on(k0)) {
      bool need0;
      float sc0;
      softmax_pack<!FAST>(sA, m_run, l_run, k0, Tk, causal, gq, scale, hi,
                          pb0, need0, sc0);
      o_rescale(o_acc, need0, sc0);
    }
    if (FAST || sub_on(k0 + 32))
      softmax_pack<!FAST>(sB, m_run, l_run, k0 + 32, Tk, causal, gq, scale,
                          hi, pb1, need1, sc1);
  };

  // S'(t) of both sub-tiles into sA / sB
  auto s_both = [&](auto fast_c, int t) {
    constexpr bool FAST = decltype(fast_c)::value;
    const short* kb = k_lds + (t & 1) * FA7_IMG;
    if (FAST || sub_on(t * FA7_BN)) sA = s_sub(kb, rb0, rb1, q_frag);
    if (FAST || sub_on(t * FA7_BN + 32))
      sB = s_sub(kb + 4096, rb0, rb1, q_frag);
  };

  // M(t): O' += V^T·P of tile t, then S'(t+1).
  auto phase_m = [&](auto fast_c, int t) {
    constexpr bool FAST = decltype(fast_c)::value;
    const int k0 = t * FA7_BN;
    const short* vb = v_lds + (t & 1) * FA7_IMG;
    if (FAST || sub_on(k0)) pv_sub(pb0, vb, tb0, tb1, o_acc);
    if (FAST || sub_on(k0 + 32)) {
      o_rescale(o_acc, need1, sc1);
      pv_sub(pb1, vb + 4096, tb0, tb1, o_acc);
    }
    if (FAST || t + 1 < n_tiles) s_both(fast_c, t + 1);
  };

  // A phase ends at its barrier for the instruction scheduler too: hipcc
  // otherwise sinks the tail of a softmax below the barrier and lifts MFMAs
  // above it, and the two waves of a SIMD meet in the same pipe.
#define FA7_PHASE_END()                                                   \
  do {                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                    \
    __syncthreads();                                                      \
    __builtin_amdgcn_sched_barrier(0);                                    \
  } while (0)

  const std::true_type fast_c{};
  const std::false_type slow_c{};

  // prologue: K(0) by all waves; then the leading waves run S'(0) while
  // the others stage their share of V(0) and K(1), and catch up with
  // S'(0) one interval later
  FA7_LOAD(K, k_st, 0, true);
  if (n_tiles > 0) FA7_WRITE(k_lds, k_st, 0);
  // what each half writes in its V(0)
  FA7_LOAD(V, v_st, grp, true);
  FA7_LOAD(K, k_st, 1 + grp, true);
  __syncthreads();
  if (grp == 0) {
    if (n_tiles > 0) s_both(slow_c, 0);
  } else {
    short8 k_p[2], v_p[2];
    FA7_LOAD(V, v_p, 0, true);
    FA7_LOAD(K, k_p, 1, true);
    if (n_tiles > 0) FA7_WRITE(v_lds, v_p, 0);
    if (n_tiles > 1) FA7_WRITE(k_lds, k_p, 1);
  }
  __syncthreads();
  if (grp == 1) {
    // the half that is dispatched second loses VALU arbitration at equal
    // priority: one static raise, no per-phase flips
    __builtin_amdgcn_s_setprio(1);
    if (n_tiles > 0) s_both(slow_c, 0);
    __syncthreads();
  }

  int t = 0;
  for (; t < n_fast; ++t) {
    phase_v(fast_c, t);
    FA7_PHASE_END();
    phase_m(fast_c, t);
    FA7_PHASE_END();
  }
  for (; t < n_tiles; ++t) {
    phase_v(slow_c, t);
    FA7_PHASE_END();
    phase_m(slow_c, t);
    FA7_PHASE_END();
  }
#undef FA7_PHASE_END
#undef FA7_LOAD
#undef FA7_WRITE

  // ---- epilogue: O[q][d] = O'[d][q] / l ----
  // o_acc[dt][r] is (d = 32dt + (r&3) + 8(r>>2) + 4hi, q = lane&31): each
  // lane writes 4 consecutive d (8 bytes) into its query's row of the
  // wave's [32][136] image, then the wave stores whole 256-byte rows.
  float inv = (l_run > 0.f) ? 1.f / l_run : 0.f;
  {
    short* const ep = ep_lds + wave * (FA7_QW * FA7_EP_STRIDE);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        u32x2 w{cvt_pk(o_acc[dt][4 * g + 0] * inv, o_acc[dt][4 * g + 1] * inv),
                cvt_pk(o_acc[dt][4 * g + 2] * inv, o_acc[dt][4 * g + 3] * inv)};
        *reinterpret_cast<u32x2*>(ep + qcol * FA7_EP_STRIDE + 32 * dt +
                                  8 * g + 4 * hi) = w;
      }
    short* out = O + obase + (long long)wave * FA7_QW * o_rs;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = lane + 64 * j;
      const int row = i >> 4;
      const int ch = i & 15;
      *reinterpret_cast<short8*>(out + (long long)row * o_rs + 8 * ch) =
          *reinterpret_cast<const short8*>(ep + row * FA7_EP_STRIDE + 8 * ch);
    }
  }
  if (LSE != nullptr && hi == 0) {
    LSE[((long long)b * Hq + hq) * T + my_q] =
        (l_run > 0.f) ? m_run + __logf(l_run) : -INFINITY;
  }
  // the trailing waves' last barrier
  if (grp == 0) __syncthreads();
}
