// FP8 weight-only skinny GEMM for decode (W8A16):
//   y[M,N] = x[M,K] · (Wq[N,K] ⊙ scale[N])^T
// x bf16, Wq OCP e4m3fn one byte per element in nn.Linear's [out, in]
// layout, scale fp32 per output channel, y bf16; 1 <= M <= 32, K % 128 == 0.
// A decode step is a weight stream (PERFORMANCE.md, "Paged KV cache"): the
// byte count is N·K, half of the bf16 GEMV's, and the math rides on the
// matrix cores so that it does not grow with the number of rows as
// gemv_bf16's VALU fmas do.
//
// MFMA and operand roles. v_mfma_f32_16x16x32_bf16, weights as A (output
// channels x k), activations as B (k x batch rows):
//   A (16x32): lane l holds A[l&15][8*(l>>4)+i], i = 0..7
//   B (32x16): lane l holds B[8*(l>>4)+i][l&15]
//   C (16x16): lane l holds C[4*(l>>4)+r][l&15], r = 0..3
// A lane loads 16 contiguous fp8 bytes of row l&15 at byte 16*(l>>4) of the
// step's 64-byte slice: the four lane groups cover 4 x 16 = 64 contiguous
// bytes of each of 16 rows, and the 16 bytes convert to 16 bf16 = two A
// fragments, so one load feeds two MFMAs (64 k per step). With
// 32x32x16 a lane's fragment is still 8 k wide but there are only two lane
// groups: 2 x 16 = 32 contiguous bytes per row, half a 64-byte segment;
// that is why the 16x16x32 shape is the one used.
//
// k-permutation instead of shuffles. MFMA j (0/1) of a step takes bytes
// 8j..8j+7 of the lane's load, so its fragment element (group g, i) is
// k = 64*step + 16*g + 8*j + i, not 32*j + 8*g + i. The sum over k has no
// order, so the B fragment is simply gathered with the same k: lane (m, g)
// takes x[m][64*step + 16*g + 8*j .. +7], one 16-byte load per MFMA, 32
// contiguous bytes per lane and 128 per row for the two. No cross-lane
// movement anywhere.
//
// Conversion in registers, exact: v_cvt_pk_f32_fp8 on each 16-bit half of a
// dword, then v_cvt_pk_bf16_f32 (the compiler-scheduled cast form of
// fa_tile.h's cvt_pk, because the result feeds the next MFMA directly).
// e4m3 has 3 mantissa bits and an exponent range inside bf16's, so every
// finite byte, subnormals and -0 included, is the same number in bf16.
// That is 4 VALU instructions per dword of weights; they sit between the
// loads of a later step and the MFMAs of this one.
//
// Weights go global -> VGPR and never through LDS: every byte is used once
// (the reasoning of "K/V straight to VGPRs" in paged_attn.hip). W8_PF = 4
// steps are in flight per lane: the loads of step s+4 are issued right
// after step s is consumed, before step s+1 is converted. The loads are
// non-temporal so the stream does not evict x from L2.
//
// Work split. A block owns 16*NT output channels and all of K; its 8 waves
// take contiguous K ranges of (K/64)/8 steps (floor split, so a K that does
// not divide evenly gives some waves one step more). With 16 channels per
// block N = 4096 gives 256 blocks, one full 8-wave block per CU, so no
// split of K across blocks is needed, there is no workspace and no second
// kernel: a captured graph has nothing to allocate. The waves' fp32
// accumulators meet in LDS ([wave][register][lane], lanes contiguous, so
// both the writes and the reads are conflict-free) and are summed in wave
// order 0..7 by one wave per 16x16 tile: no atomics, bit-identical from
// call to call. A wave's range, and so every sum, depends only on K: the
// result does not depend on NT or on the grid.
//
// Activations: deviation from staging x in LDS. Because the waves of a
// block split K, every x element a block needs is consumed by exactly one
// of its waves, exactly once: LDS would be a write and a read with no
// reuse, the same argument as for the weights. Its only other use would be
// to re-lay x for the B fragment, and the k-permutation already makes that
// fragment two plain 16-byte loads. So x also goes global -> VGPR, served
// from L2 (x is at most 32 x 14336 bf16 = 896 KB and is read by every
// block). What x costs is L2 traffic of 2*M/(16*NT) bytes per weight byte;
// NT = 2 (two A tiles share each B fragment) halves it where N is large
// enough that 32-channel blocks still fill the CUs twice over.
//
// Padding: deviation from zero fragments. Rows and columns of an MFMA do
// not mix, so a lane whose channel (>= N) or batch row (>= M) does not
// exist needs no zeros: it loads row 0 again, the same addresses as a real
// lane and so no extra traffic, and what it produces lands in accumulator
// entries that are never stored. With predicated loads instead, the branch
// around every load made the compiler drain all loads (vmcnt(0)) once per
// pipeline group; unconditional loads keep W8_PF steps in flight. Nothing
// outside the M real rows of x and the N real rows of Wq is ever read.
//
// Epilogue: fp32 sum * scale[n], one rounding to bf16, 8-byte stores of a
// lane's four consecutive channels when N % 4 == 0 (else 2-byte stores).
// Channels >= N and rows >= M are neither read nor written.
#include "fa_tile.h"

#define W8_WAVES 8
#define W8_PF 4

// The reduction and the scale multiply stay scalar fp32 (v_add_f32,
// v_mul_f32): w8_scalar pins a value to its own VGPR, so the vectoriser has
// no pair of sums to turn into one packed fp32 instruction.
DEV_INLINE float w8_scalar(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

template <int MT, int NT>
struct W8Stage {
  u32x4 w[NT];
  u32x4 x[MT][2];
};

// 16 fp8 bytes -> the A fragments of the step's two MFMAs
DEV_INLINE void w8_cvt(const u32x4& w, bf16x8& a0, bf16x8& a1) {
  unsigned int o[8];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const float2v lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], false);
    const float2v hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], true);
    o[2 * d] = cvt_pk(lo[0], lo[1]);
    o[2 * d + 1] = cvt_pk(hi[0], hi[1]);
  }
  a0 = __builtin_bit_cast(bf16x8, u32x4{o[0], o[1], o[2], o[3]});
  a1 = __builtin_bit_cast(bf16x8, u32x4{o[4], o[5], o[6], o[7]});
}

template <int MT, int NT>
__global__ __launch_bounds__(64 * W8_WAVES) void linear_w8_bf16_kernel(
    const short* __restrict__ X, const unsigned char* __restrict__ Wq,
    const float* __restrict__ scale, short* __restrict__ Y, int M, int N,
    int K) {
  __shared__ float red[W8_WAVES][NT * MT * 4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r16 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (16 * NT);
  const int steps = K / 64;
  const int beg = (int)((long long)steps * wave / W8_WAVES);
  const int end = (int)((long long)steps * (wave + 1) / W8_WAVES);

  // per-lane row pointers at the lane's 16 k of step 0; a lane whose
  // channel or batch row does not exist reads row 0 instead (see above)
  const unsigned char* wp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = n0 + 16 * t + r16;
    wp[t] = Wq + (size_t)(n < N ? n : 0) * K + 16 * g;
  }
  const short* xp[MT];
#pragma unroll
  for (int u = 0; u < MT; ++u) {
    const int m = 16 * u + r16;
    xp[u] = X + (size_t)(m < M ? m : 0) * K + 16 * g;
  }

  float4v acc[NT][MT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int u = 0; u < MT; ++u) acc[t][u] = float4v{0.f, 0.f, 0.f, 0.f};

  auto load = [&](W8Stage<MT, NT>& st, int s) {
    const size_t off = (size_t)s * 64;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      st.w[t] = __builtin_nontemporal_load(
          reinterpret_cast<const u32x4*>(wp[t] + off));
#pragma unroll
    for (int u = 0; u < MT; ++u)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        st.x[u][j] = *reinterpret_cast<const u32x4*>(xp[u] + off + 8 * j);
  };
  auto compute = [&](const W8Stage<MT, NT>& st) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      bf16x8 a0, a1;
      w8_cvt(st.w[t], a0, a1);
#pragma unroll
      for (int u = 0; u < MT; ++u) {
        acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a0, __builtin_bit_cast(bf16x8, st.x[u][0]), acc[t][u], 0, 0, 0);
        acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a1, __builtin_bit_cast(bf16x8, st.x[u][1]), acc[t][u], 0, 0, 0);
      }
    }
  };

  // the steps that do not fill a group of W8_PF go first, one at a time;
  // the rest run as a W8_PF-deep pipeline with no branch inside a group
  int s = beg;
  for (const int head = beg + (end - beg) % W8_PF; s < head; ++s) {
    W8Stage<MT, NT> st;
    load(st, s);
    compute(st);
  }
  if (s < end) {
    W8Stage<MT, NT> st[W8_PF];
#pragma unroll
    for (int p = 0; p < W8_PF; ++p) load(st[p], s + p);
    for (; s + W8_PF < end; s += W8_PF) {
#pragma unroll
      for (int p = 0; p < W8_PF; ++p) {
        compute(st[p]);
        load(st[p], s + W8_PF + p);
      }
    }
#pragma unroll
    for (int p = 0; p < W8_PF; ++p) compute(st[p]);
  }

  // fixed-order reduction over the waves
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int u = 0; u < MT; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        red[wave][(t * MT + u) * 4 + r][lane] = acc[t][u][r];
  __syncthreads();
  if (wave >= NT * MT) return;
  const int t = wave / MT, u = wave % MT;
  float sum[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    sum[r] = red[0][wave * 4 + r][lane];
#pragma unroll
    for (int w = 1; w < W8_WAVES; ++w)
      sum[r] = w8_scalar(sum[r] + red[w][wave * 4 + r][lane]);
  }
  const int m = 16 * u + r16;
  const int n = n0 + 16 * t + 4 * g;
  if (m >= M || n >= N) return;
  short* yp = Y + (size_t)m * N + n;
  if (N % 4 == 0) {
    short4v o;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      o[r] = f2bf(w8_scalar(sum[r] * scale[n + r]));
    *reinterpret_cast<short4v*>(yp) = o;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (n + r < N) yp[r] = f2bf(w8_scalar(sum[r] * scale[n + r]));
  }
}
