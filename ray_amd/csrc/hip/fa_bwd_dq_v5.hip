// dq v5: grid (T/256, B*Hq), 8 waves x 32 q rows, Q/dO register-resident,
//  - 64-row K/V tiles, double buffered: 48 MFMAs per wave per barrier;
//  - split staging: the global loads of tile t+1 are issued before tile
//    t's MFMAs and written to the other buffer after them, before the
//    tile's one barrier (loading and storing in one statement makes every
//    wave sit through the load latency at the top of each tile);
//  - -LSE/scale and -delta as the initial accumulators of the S and dP
//    chains (lane constants here: the query is on the lane);
//  - dS is exchanged with cvt_pk + permlane32_swap: feeding the packed
//    registers to the MFMA directly (permuted k order) measured slower,
//    see PERFORMANCE.md;
//  - the fb6_off LDS image (conflict-free row and transposed reads, two
//    address registers per kind of read).
// dQ[q][d] += sum_k dS^T[k][q] K[k][d]
#include "fa_bwd_frag.h"
#include "fa_bwd_lds_layout.h"

#define FB5_KT 64  // K/V rows per staged tile

extern "C" __global__ __launch_bounds__(512) void fa_bwd_dq_v5_bf16(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ Dsum,
    short* __restrict__ dQ, int B, int Hq, int Hkv, int T, int causal,
    float scale, int bthd, int q_rs_, int o_rs_, int kv_rs_, int dq_rs_) {
  // bthd=1: token-row storage with row strides (elements) q_rs for Q, o_rs
  // for dO, kv_rs for K/V and dq_rs for dQ (a [B,T,H,D] tensor or a column
  // section of a packed [B,T,rs] buffer); bthd=0: contiguous [B,H,T,D],
  // every stride is D. 32-bit arguments: a row offset is then one
  // 32 x 32 -> 64-bit multiply-add.
  __shared__ __attribute__((aligned(16))) short k_lds[2 * FB5_KT * FB3_D];
  __shared__ __attribute__((aligned(16))) short v_lds[2 * FB5_KT * FB3_D];

  // heaviest causal block (the last query rows) first inside a grid row,
  // and the order rotated from row to row: workgroups are dealt to the 8
  // XCDs round-robin, so with gridDim.x a multiple of 8 and a fixed order
  // one XCD gets the heaviest block of every head (PERFORMANCE.md). A
  // head's blocks stay together in time and share K/V in the L2.
  const int qb = (blockIdx.x + blockIdx.y) % gridDim.x;
  const int q0 = (gridDim.x - 1 - qb) * 256;
  const int bh = blockIdx.y;
  const int b = bh / Hq;
  const int hq = bh % Hq;
  const int hkv = hq / (Hq / Hkv);
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int hi = lane >> 5;

  const long long q_rs = q_rs_, o_rs = o_rs_, kv_rs = kv_rs_, dq_rs = dq_rs_;
  const long long qbase =
      bthd ? ((long long)b * T + q0) * q_rs + hq * FB3_D
           : (((long long)b * Hq + hq) * T + q0) * FB3_D;
  const long long obase =
      bthd ? ((long long)b * T + q0) * o_rs + hq * FB3_D : qbase;
  const long long dqbase =
      bthd ? ((long long)b * T + q0) * dq_rs + hq * FB3_D : qbase;
  const long long kbase =
      bthd ? (long long)b * T * kv_rs + hkv * FB3_D
           : (((long long)b * Hkv + hkv) * T) * FB3_D;
  const int my_q = q0 + wave * 32 + (lane & 31);

  bf16x8 q_frag[8], do_frag[8];
  {
    const short* qp = Q + qbase + ((long long)wave * 32 + (lane & 31)) * q_rs;
    const short* dp = dO + obase + ((long long)wave * 32 + (lane & 31)) * o_rs;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      q_frag[c] = ld8(qp + 16 * c + 8 * hi);
      do_frag[c] = ld8(dp + 16 * c + 8 * hi);
    }
  }
  const float c2 = scale * 1.4426950408889634f;
  float s_init = -LSE[((long long)b * Hq + hq) * T + my_q] / scale;
  float dp_init = -Dsum[((long long)b * Hq + hq) * T + my_q];

  f32x16 dq_acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) dq_acc[t] = f32x16{};

  const int wave_k_max = q0 + wave * 32 + 31;  // last k this wave needs
  const int k_end = causal ? min(T, q0 + 256) : T;
  const int n_tiles = k_end / FB5_KT;  // T % 256 == 0

  // 64 rows x 16 chunks / 512 threads = 2 chunks per tensor
  short8 k_st[2], v_st[2];
  const int st_r = tid >> 4;  // + 32 * j
  const int st_c = tid & 15;

#define FB5_DQ_LOAD(t_idx)                                                \
  do {                                                                    \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                       \
      const long long go_ =                                               \
          kbase + (long long)((t_idx) * FB5_KT + st_r + 32 * j) * kv_rs + \
          8 * st_c;                                                       \
      k_st[j] = *reinterpret_cast<const short8*>(K + go_);                \
      v_st[j] = *reinterpret_cast<const short8*>(V + go_);                \
    }                                                                     \
  } while (0)

#define FB5_DQ_WRITE(buf)                                                 \
  do {                                                                    \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                       \
      const int o_ = (buf) * (FB5_KT * FB3_D) + fb6_off(st_r + 32 * j, st_c); \
      *reinterpret_cast<short8*>(k_lds + o_) = k_st[j];                   \
      *reinterpret_cast<short8*>(v_lds + o_) = v_st[j];                   \
    }                                                                     \
  } while (0)

  FB5_DQ_LOAD(0);
  FB5_DQ_WRITE(0);
  __syncthreads();

  const int rb0 = fb6_rbase(lane, 0), rb1 = fb6_rbase(lane, 1);
  const int gl = lane & 15;
  const int grp16 = (lane >> 4) & 1;

  // Retire the Q/dO fragment and row-constant loads here, once. Left
  // pending into the loop, the first use of a fragment in EVERY iteration
  // gets a full vmcnt(0), which also waits for the tile just issued.
  // The empty asm takes the values as operands, so the loads cannot be
  // moved below it.
#pragma unroll
  for (int c = 0; c < 8; ++c)
    asm volatile("" : "+v"(q_frag[c]), "+v"(do_frag[c]));
  asm volatile("" : "+v"(s_init), "+v"(dp_init));

  for (int t = 0; t < n_tiles; ++t) {
    const int cur = t & 1;
    const bool more = t + 1 < n_tiles;
    if (more) FB5_DQ_LOAD(t + 1);
    const short* kbuf = k_lds + cur * (FB5_KT * FB3_D);
    const short* vbuf = v_lds + cur * (FB5_KT * FB3_D);

#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      const int k0 = t * FB5_KT + 32 * kt;
      // wave-uniform skip of tiles wholly above the diagonal
      if (causal && k0 > wave_k_max) continue;

      // S'^T = K·Q^T - LSE/scale and dP'^T = V·dO^T - delta ([k][q], the
      // lane owns column q)
      f32x16 s_acc, dp_acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s_acc[r] = s_init;
        dp_acc[r] = dp_init;
      }
      {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const int o = ((c & 1) ? rb1 : rb0) + 256 * (c >> 1) + 4096 * kt;
          bf16x8 kf = ld8(kbuf + o);
          bf16x8 vf = ld8(vbuf + o);
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
        const int gk = k0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        float p = __builtin_amdgcn_exp2f(s_acc[r] * c2);
        if (!full_tile && gk > my_q) p = 0.f;
        ds[r] = p * dp_acc[r] * scale;
      }

      // dQ += dS·K: A = dS via pack_swap (plain cvt_pk, see fa_tile.h),
      // B = K via ds_read_tr16_b64
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 af = pack_swap<false>(ds, s);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          // ld_tr8 spelled out: the call changes this loop's code
          short ktmp[8];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int row = 32 * kt + 16 * s + 8 * hi + 4 * h + (gl >> 2);
            const int o =
                fb6_off(row, 4 * dt + 2 * grp16 + ((gl & 3) >> 1)) +
                4 * (gl & 1);
            short4v r4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) short4v*)(kbuf + o));
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

    // write-late half of the staging split: the other buffer was last
    // read before the previous barrier
    if (more) FB5_DQ_WRITE(cur ^ 1);
    __syncthreads();
  }
#undef FB5_DQ_LOAD
#undef FB5_DQ_WRITE

  c_store(dq_acc, dQ + dqbase + (long long)wave * 32 * dq_rs, dq_rs, lane,
          hi);
}
