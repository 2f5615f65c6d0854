// fa_bwd dkv v6: fused dK+dV with the KEY on the MFMA lane.
//
// With S^T = K·Q^T (query on the lane, as in fa_bwd_v3.hip) the dV and dK
// products, which sum over the query index, need P and dS transposed: 2x16
// two-byte LDS writes, two full waitcnt drains and 4 reads per 32x32 tile.
// v6 computes S = Q·K^T and dP = dO·V^T (A = Q / dO rows from LDS, B = the
// K fragment in registers / V rows from LDS). The accumulators then have
// the key on the lane and 16 query rows in the registers, which is
// already the B-operand layout of
//     dV^T[d][k] += dO^T[d][q] · P[q][k]     dK^T[d][k] += Q^T[d][q] · dS[q][k]
// Registers 8s..8s+7, packed to bf16, are the fragment of k-step s; its
// k order is permuted (element j of lane half h is query row
// 16s + 8(j>>2) + 4h + (j&3)), so the transposed reads of do_lds / q_lds
// take their two 4-row blocks at rows 16s+4h and 16s+4h+8.
//
// -LSE/scale and -delta are the initial accumulators of the S and dP
// chains (they differ per register, not per lane, in this orientation),
// so p = exp2(c·S') and dS = p·dP'·scale need no subtract.
//
// Staging of Q/dO is split (issue early, write late): tile t+1's Q loads
// are issued before tile t's first 32 query rows and written to the other
// LDS buffer after them; its dO loads fly across the second 32 rows and are
// written just before the tile's one barrier.
//
// The q/dO/V images are built of 8-row x 32-column subtiles of 512 B with
// an XOR inside each 64-byte subtile row (fb6_off): conflict-free for both
// the ds_read_b128 row reads and the ds_read_tr16_b64 column reads, and
// every read of a tile is one of two lane-dependent bases plus a
// compile-time offset, so the addresses cost 6 registers, not 40.
//
// LDS: V 64K + q/dO double buffers 64K + row constants 1K = 129 KB. The
// epilogue transposes dK^T/dV^T through the same memory and stores whole
// 256-byte rows.
#include "fa_bwd_frag.h"
#include "fa_bwd_lds_layout.h"

#define FB6_EP_STRIDE 136  // epilogue row stride in bf16 (256 B + 16 B pad)

// Grid (B*Hkv, T/256): the key block is the slow dimension, so key block 0,
// the heaviest under the causal mask, is dispatched first.
extern "C" __global__ __launch_bounds__(512) void fa_bwd_dkv_v6_bf16(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ Dsum,
    short* __restrict__ dK, short* __restrict__ dV, int B, int Hq,
    int Hkv, int T, int causal, float scale, int bthd, int q_rs_, int o_rs_,
    int kv_rs_, int dkv_rs_) {
  // bthd=1: token-row storage with row strides (elements) q_rs for Q, o_rs
  // for dO, kv_rs for K/V and dkv_rs for dK/dV (a [B,T,H,D] tensor or a
  // column section of a packed [B,T,rs] buffer); bthd=0: contiguous
  // [B,H,T,D], every stride is D.
  __shared__ __attribute__((aligned(16))) short smem[65536 + 512];
  // q and dO first: every tile read is then base + immediate (< 64 KB)
  short* const q_lds = smem;                  // [2][64][128]
  short* const do_lds = smem + 16384;         // [2][64][128]
  short* const v_lds = smem + 32768;          // [256][128]
  float* const lse_lds = reinterpret_cast<float*>(smem + 65536);  // [2][64]
  float* const dsum_lds = lse_lds + 128;                          // [2][64]

  const int kb = blockIdx.y;
  const int bh = blockIdx.x;
  const int k0 = kb * 256;
  const int b = bh / Hkv;
  const int hkv = bh % Hkv;
  const int rep = Hq / Hkv;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar
  const int lane = tid & 63;
  const int hi = lane >> 5;

  const long long q_rs = q_rs_, o_rs = o_rs_, kv_rs = kv_rs_, dkv_rs = dkv_rs_;
  const long long kbase =
      bthd ? ((long long)b * T + k0) * kv_rs + hkv * FB3_D
           : (((long long)b * Hkv + hkv) * T + k0) * FB3_D;
  const long long dkbase =
      bthd ? ((long long)b * T + k0) * dkv_rs + hkv * FB3_D : kbase;

  // K register-resident (B operand of S: lane = key, 8 d per k-step half);
  // V into LDS once.
  bf16x8 k_frag[8];
  {
    const short* kp = K + kbase + ((long long)32 * wave + (lane & 31)) * kv_rs;
#pragma unroll
    for (int c = 0; c < 8; ++c) k_frag[c] = ld8(kp + 16 * c + 8 * hi);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int i = tid + 512 * j;
    int r = i >> 4;
    int c = i & 15;
    *reinterpret_cast<short8*>(v_lds + fb6_off(r, c)) =
        *reinterpret_cast<const short8*>(V + kbase + (long long)r * kv_rs +
                                         8 * c);
  }

  f32x16 dk_acc[4], dv_acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    dk_acc[t] = f32x16{};
    dv_acc[t] = f32x16{};
  }
  const float c2 = scale * 1.4426950408889634f;

  const int q_start = causal ? k0 : 0;
  const int nq = (T - q_start) / FB3_QT;
  const int n_tiles = rep * nq;

  // staging registers: 64 rows x 16 chunks / 512 threads = 2 per tensor.
  // Q is in flight across the tile's first 32 query rows and dO across the
  // second 32, so only one of the two is live at a time (8 registers).
  short8 q_st[2], do_st[2];
  float c_st = 0.f;
  const int st_r = tid >> 4;  // + 32 * j
  const int st_c = tid & 15;
  // lane part of a staged chunk's global offset (a tile is < 2^31 elements
  // from its first row: the host checks 64 rows x row stride); the tile
  // part is scalar. Q and dO have a row stride each.
  const unsigned st_go = (unsigned)(st_r * (int)q_rs + 8 * st_c);
  const unsigned st_go_do = (unsigned)(st_r * (int)o_rs + 8 * st_c);
  // wave 0 stages -LSE/scale, wave 1 stages -delta (lse_lds, dsum_lds are
  // adjacent)
  const float* const c_src = wave == 0 ? LSE : Dsum;
  const float c_div = wave == 0 ? scale : 1.f;
  float* const c_dst = lse_lds + 2 * FB3_QT * wave;

#define FB6_TILE_BASE(t_idx, rs_)                                         \
  const int g_ = (t_idx) / nq;                                            \
  const int q0_ = q_start + ((t_idx) - g_ * nq) * FB3_QT;                 \
  const int hq_ = hkv * rep + g_;                                         \
  const long long qb_ =                                                   \
      (bthd ? (long long)b * T * (rs_) + hq_ * FB3_D                      \
            : (((long long)b * Hq + hq_) * T) * FB3_D) +                  \
      (long long)q0_ * (rs_);                                             \
  const long long lb_ = ((long long)b * Hq + hq_) * T + q0_;

#define FB6_LOAD_Q(t_idx)                                                 \
  do {                                                                    \
    FB6_TILE_BASE(t_idx, q_rs)                                            \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                         \
      q_st[j] = *reinterpret_cast<const short8*>(                         \
          Q + qb_ + 32 * j * q_rs + st_go);                               \
    if (wave < 2) c_st = (c_src + lb_)[fb6_lane_fresh()];                 \
  } while (0)

#define FB6_LOAD_DO(t_idx)                                                \
  do {                                                                    \
    FB6_TILE_BASE(t_idx, o_rs)                                            \
    (void)lb_;                                                            \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                         \
      do_st[j] = *reinterpret_cast<const short8*>(                        \
          dO + qb_ + 32 * j * o_rs + st_go_do);                           \
  } while (0)

#define FB6_WRITE_Q(buf)                                                  \
  do {                                                                    \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                         \
      *reinterpret_cast<short8*>(q_lds + (buf) + 4096 * j) = q_st[j];     \
    if (wave < 2)                                                         \
      c_dst[((buf) >> 13) * FB3_QT + fb6_lane_fresh()] = -c_st / c_div;   \
  } while (0)

#define FB6_WRITE_DO(buf)                                                 \
  do {                                                                    \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                         \
      *reinterpret_cast<short8*>(do_lds + (buf) + 4096 * j) = do_st[j];   \
  } while (0)

  const int gk = k0 + 32 * wave + (lane & 31);  // this lane's key
  // Read bases into the CURRENT q buffer; dO is 16384 elements on. They
  // stay below 8192, the buffer size, with every immediate added, so the
  // buffer swap is an XOR.
  int rb0 = fb6_rbase(lane, 0), rb1 = fb6_rbase(lane, 1);
  int tb0 = fb6_tbase(lane, 0), tb1 = fb6_tbase(lane, 1);
  int st_o = fb6_off(st_r, st_c) ^ 8192;  // staging writes: the OTHER buffer
  const short* const vw0 = v_lds + 4096 * wave + fb6_rbase(lane, 0);
  const short* const vw1 = v_lds + 4096 * wave + fb6_rbase(lane, 1);

  FB6_LOAD_Q(0);
  FB6_LOAD_DO(0);
  FB6_WRITE_Q(st_o ^ 8192);
  FB6_WRITE_DO(st_o ^ 8192);
  __syncthreads();

  for (int t = 0; t < n_tiles; ++t) {
    const int cur = t & 1;
    const int q0s = q_start + (t % nq) * FB3_QT;
    const bool more = t + 1 < n_tiles;
    if (more) FB6_LOAD_Q(t + 1);

#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int qts = q0s + 32 * qt;
      if (qt == 1 && more) {
        // the other buffer was last read before the previous barrier
        FB6_WRITE_Q(st_o);
        FB6_LOAD_DO(t + 1);
      }
      // wave-uniform skip of tiles wholly above the diagonal
      if (causal && k0 + 32 * wave > qts + 31) continue;

      // S' = Q·K^T - LSE/scale and dP' = dO·V^T - delta, key on the lane
      f32x16 s_acc, dp_acc;
      {
        const float* lp = lse_lds + cur * FB3_QT + 32 * qt + 4 * hi;
        const float* dp = dsum_lds + cur * FB3_QT + 32 * qt + 4 * hi;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float4v l4 = *reinterpret_cast<const float4v*>(lp + 8 * g);
          float4v d4 = *reinterpret_cast<const float4v*>(dp + 8 * g);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            s_acc[4 * g + i] = l4[i];
            dp_acc[4 * g + i] = d4[i];
          }
        }
      }
      {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const int o = ((c & 1) ? rb1 : rb0) + 256 * (c >> 1) + 4096 * qt;
          bf16x8 qf = ld8(q_lds + o);
          bf16x8 dof = ld8(do_lds + o);
          bf16x8 vf = ld8(((c & 1) ? vw1 : vw0) + 256 * (c >> 1));
          s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, k_frag[c],
                                                          s_acc, 0, 0, 0);
          dp_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dof, vf, dp_acc,
                                                           0, 0, 0);
        }
      }

      // P -> s_acc, dS -> dp_acc (in place); register r is query row
      // qts + (r&3) + 8(r>>2) + 4hi
      const bool full_tile = !causal || (k0 + 32 * wave + 31 <= qts);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        // c_row spelled out: the call changes this loop's code
        const int gq = qts + (r & 3) + 8 * (r >> 2) + 4 * hi;
        float pv = __builtin_amdgcn_exp2f(s_acc[r] * c2);
        if (!full_tile && gk > gq) pv = 0.f;
        s_acc[r] = pv;
        dp_acc[r] = pv * dp_acc[r] * scale;
      }
      bf16x8 p_frag[2], ds_frag[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        u32x4 pw{cvt_pk(s_acc[8 * s + 0], s_acc[8 * s + 1]),
                     cvt_pk(s_acc[8 * s + 2], s_acc[8 * s + 3]),
                     cvt_pk(s_acc[8 * s + 4], s_acc[8 * s + 5]),
                     cvt_pk(s_acc[8 * s + 6], s_acc[8 * s + 7])};
        u32x4 dw{cvt_pk(dp_acc[8 * s + 0], dp_acc[8 * s + 1]),
                     cvt_pk(dp_acc[8 * s + 2], dp_acc[8 * s + 3]),
                     cvt_pk(dp_acc[8 * s + 4], dp_acc[8 * s + 5]),
                     cvt_pk(dp_acc[8 * s + 6], dp_acc[8 * s + 7])};
        p_frag[s] = __builtin_bit_cast(bf16x8, pw);
        ds_frag[s] = __builtin_bit_cast(bf16x8, dw);
      }

      // dV^T += dO^T·P and dK^T += Q^T·dS: A via ds_read_tr16_b64 in the
      // permuted query order, B = the packed accumulators
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          // ld_tr8 spelled out: dO's and Q's reads are issued in pairs
          short dtmp[8], qtmp[8];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            // rows 32qt + 16s + 8h + 4hi .. +3
            const int o = (h ? tb1 : tb0) + 1024 * (4 * qt + 2 * s + h) +
                          256 * dt;
            short4v d4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) short4v*)(do_lds + o));
            short4v q4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) short4v*)(q_lds + o));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              dtmp[4 * h + j] = d4[j];
              qtmp[4 * h + j] = q4[j];
            }
          }
          bf16x8 adO = __builtin_bit_cast(
              bf16x8, *reinterpret_cast<short8*>(dtmp));
          bf16x8 aQ = __builtin_bit_cast(
              bf16x8, *reinterpret_cast<short8*>(qtmp));
          dv_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              adO, p_frag[s], dv_acc[dt], 0, 0, 0);
          dk_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              aQ, ds_frag[s], dk_acc[dt], 0, 0, 0);
        }
      }
    }

    if (more) FB6_WRITE_DO(st_o);
    rb0 ^= 8192;
    rb1 ^= 8192;
    tb0 ^= 8192;
    tb1 ^= 8192;
    st_o ^= 8192;
    __syncthreads();
  }
#undef FB6_TILE_BASE
#undef FB6_LOAD_Q
#undef FB6_LOAD_DO
#undef FB6_WRITE_Q
#undef FB6_WRITE_DO

  // Epilogue. acc[dt][r] is (d = 32dt + (r&3) + 8(r>>2) + 4hi, key = lane):
  // each lane writes 4 consecutive d (8 bytes) into its key's row of a
  // per-wave [32][136] image, then the wave stores whole 256-byte rows.
  // The loop's last barrier has retired every read of the tile buffers.
  const int el = fb6_lane_fresh();
  const int er = el & 31;
  const int eh = el >> 5;
  short* const ep = smem + wave * (32 * FB6_EP_STRIDE);
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    short* out =
        (pass == 0 ? dK : dV) + dkbase + (long long)wave * 32 * dkv_rs;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x16& a = pass == 0 ? dk_acc[dt] : dv_acc[dt];
        u32x2 w{cvt_pk(a[4 * g + 0], a[4 * g + 1]),
                    cvt_pk(a[4 * g + 2], a[4 * g + 3])};
        *reinterpret_cast<u32x2*>(ep + er * FB6_EP_STRIDE + 32 * dt +
                                      8 * g + 4 * eh) = w;
      }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = el + 64 * j;
      const int row = i >> 4;
      const int ch = i & 15;
      *reinterpret_cast<short8*>(out + (long long)row * dkv_rs + 8 * ch) =
          *reinterpret_cast<const short8*>(ep + row * FB6_EP_STRIDE + 8 * ch);
    }
  }
}
