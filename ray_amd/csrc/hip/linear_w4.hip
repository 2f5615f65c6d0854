// MXFP4 weight-only skinny GEMM for decode (W4A16):
//   y[M,N] = x[M,K] · dequant(Wq[N,K/2], S[N,K/32])^T
// x bf16, y bf16, fp32 accumulation; 1 <= M <= 32, K % 128 == 0, any N >= 1.
// Wq holds OCP e2m1 nibbles in nn.Linear's [out, in] layout, element 2i in
// the low nibble of byte i and 2i+1 in the high nibble; S holds one e8m0
// code per 32 consecutive k (value 2^(code-127)), codes 2..252
// (ops.quantize_weight_mxfp4). A decode step is a weight stream
// (PERFORMANCE.md, "FP8 weight-only decode"); this halves the bytes again,
// to 17/32 byte per weight.
//
// MFMA and operand roles, as in linear_w8.hip. v_mfma_f32_16x16x32_bf16,
// weights as A (output channels x k), activations as B (k x batch rows):
//   A (16x32): lane l holds A[l&15][8*(l>>4)+i], i = 0..7
//   B (32x16): lane l holds B[8*(l>>4)+i][l&15]
//   C (16x16): lane l holds C[4*(l>>4)+r][l&15], r = 0..3
// A step is 128 k. Lane (r = l&15, g = l>>4) loads the 16 bytes of row r at
// byte 64*step + 16*g: 32 nibbles, k = 128*step + 32*g .. +31, which is
// exactly one MX block, so a lane needs one scale per load. The four lane
// groups cover a contiguous 64-byte slice of each of 16 rows.
//
// k-permutation instead of shuffles. One load feeds four MFMAs: MFMA j
// takes dword j of the lane's load, so its fragment element (g, i) is
//   k = 128*step + 32*g + 8*j + i        (not 32*j + 8*g + i).
// The sum over k has no order, so the B fragment is gathered under the same
// k: lane (m, g) takes x[m][128*step + 32*g + 8*j .. +7]. No cross-lane
// movement anywhere.
//
// Conversion in registers, exact. v_cvt_scalef32_pk_bf16_fp4 turns one byte
// of a dword (op_sel picks it) into two bf16 times an fp32 scale: four per
// dword, 16 per load. An e2m1 value has two significant bits and the scale
// is a power of two; with codes 2..252 every product is zero or a normal
// bf16, so nothing rounds. The scale is the e8m0 code shifted into an fp32
// exponent (code << 23). Scale fetch: K % 128 == 0 makes a row of S a whole
// number of dwords, and the dword at byte 4*step holds the step's four
// codes, one per lane group: a lane loads that dword and takes byte g. One
// 4-byte load per step next to the 16-byte weight load, no byte loads.
//
// Weights go global -> VGPR and never through LDS (every byte is used once),
// non-temporal. A chunk is W4_CH = 4 steps: a lane has the 4 + 4 loads of
// the next chunk in flight while it converts and multiplies this one.
//
// Work split and x traffic: the part that differs from linear_w8.hip. There
// a block owns 16 (or 32) channels and its waves split K, so every block
// reads all of x from L2: 2*M*K bytes of x against 16*K bytes of weights.
// At four bits the same block would have 8*K weight bytes: 0.25 x-bytes per
// weight byte at M = 1 and 8 at M = 32; the kernel would be an x stream.
// x-bytes per weight byte is 4*M/C for C channels per block, whatever the
// split of K, so C has to grow:
//   C = 16  (the fp8 split):      M/4   0.25 at M = 1,  8   at M = 32
//   C = 64  (4 waves, tile 64):   M/16  0.06 at M = 1,  2   at M = 32
//   C = 128 (8 waves, tile 128):  M/32  0.03 at M = 1,  1   at M = 32
// (x is fetched in 16-row tiles, and rows past M repeat row 0 at the same
// addresses.) Here the waves of a block split N, 16 channels each, and
// share x: a chunk of x (16 or 32 rows x 512 k) is staged once per block in
// LDS and read by every wave. It is stored in fragment order, one plane of
// 64 16-byte units per (step, row tile, j) with unit index = lane, so a
// wave's B fragment is one ds_read_b128 at consecutive addresses with no
// bank conflicts; planes are W4_PLANE = 68 units apart so that the four j
// of a staging write land in different banks. Two buffers: the global loads
// of the next chunk of x are issued before this chunk's MFMAs and written
// to the other buffer after them, one barrier per chunk. The launcher uses
// tile 128 for every M: the ratio stays <= 1, and tile 64 measured slower at
// every row count (PERFORMANCE.md, "MXFP4 weight-only decode").
//
// K split across blocks. 128-channel blocks are only 32 at N = 4096, so K
// is also split, over blockIdx.y, to fill 256 CUs. For a result that does
// not depend on the grid the order of the fp32 sums is fixed by K alone:
// the K/128 steps are cut (floor split) into W4_GROUPS = 8 groups, each
// group's products accumulate in step order from zero in the MFMA
// accumulator, and the eight group sums are added as the balanced tree
//   ((g0+g1)+(g2+g3)) + ((g4+g5)+(g6+g7)).
// A block owns an aligned run of 8/S groups (S = 1, 2, 4, 8 slices) and
// adds them as their subtree, in registers, with a three-deep stack. S = 1
// finishes the tree and stores bf16. S > 1 stores its subtree's fp32 sum in
// a workspace [S][M][N] and linear_w4_combine finishes the tree from the S
// partials: the same additions on the same values in either case. No
// atomics; bit-identical from call to call, for every S and both tiles.
// Groups without steps (K < 1024) enter the tree as zeros in both paths.
//
// Padding as in linear_w8.hip: a lane whose channel (>= N) or batch row
// (>= M) does not exist reads row 0 again, unconditionally, and what it
// produces lands in accumulator entries that are never stored. Nothing
// outside the M real rows of x and the N real rows of Wq and S is read, and
// nothing outside y[M][N] (and the workspace) is written.
//
// Deviations from the plan of record: none in the operand layout; the x
// tile is staged in LDS and K is split across blocks, both candidates, used
// together. One dword scale load per step rather than one wider load per
// chunk, because 16-byte scale loads would need K % 512 == 0.
#include "fa_tile.h"

#define W4_CH 4
#define W4_GROUPS 8
#define W4_PLANE 68

// fp32 sums stay scalar (v_add_f32): a value pinned to its own VGPR gives
// the vectoriser no pair to turn into one packed fp32 instruction
DEV_INLINE float w4_scalar(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

DEV_INLINE float4v w4_add(float4v a, float4v b) {
  float4v o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = w4_scalar(a[r] + b[r]);
  return o;
}

// one dword = 8 nibbles -> 8 bf16 (an A fragment), times the block scale
DEV_INLINE bf16x8 w4_cvt(unsigned int w, float scale) {
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3);
  return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// e8m0 code -> fp32 2^(code-127); codes 1..254 are normal fp32 exponents
DEV_INLINE float w4_scale(unsigned int code) {
  return __builtin_bit_cast(float, code << 23);
}

struct W4Stage {
  u32x4 w[W4_CH];
  unsigned int sc[W4_CH];
};

// GPB: groups per block (8 / slices). GPB == 8 stores y, else the workspace.
template <int MT, int WAVES, int GPB>
__global__ __launch_bounds__(64 * WAVES) void linear_w4_bf16_kernel(
    const short* __restrict__ X, const unsigned char* __restrict__ Wq,
    const unsigned char* __restrict__ Sc, short* __restrict__ Y,
    float* __restrict__ ws, int M, int N, int K) {
  constexpr int COMBOS = W4_CH * MT * 4;  // (step, row tile, lane group)
  constexpr int XLOADS = COMBOS / WAVES;  // staging loads per thread
  static_assert(COMBOS % WAVES == 0, "staging must divide over the waves");
  __shared__ u32x4 xs[2][W4_CH * MT * 4 * W4_PLANE];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r16 = lane & 15, g = lane >> 4;
  const int steps = K / 128;
  auto gbeg = [&](int q) { return (int)((long long)steps * q / W4_GROUPS); };
  const int q0 = blockIdx.y * GPB;
  const int se = gbeg(q0 + GPB);

  // the wave's 16 channels; a channel that does not exist reads row 0
  const int n0 = blockIdx.x * (16 * WAVES) + 16 * wave;
  const int nrow = n0 + r16 < N ? n0 + r16 : 0;
  const unsigned char* wp = Wq + (size_t)nrow * (K / 2) + 16 * g;
  const unsigned char* sp = Sc + (size_t)nrow * (K / 32);

  // staging role: 64 contiguous bytes of x (the four j of one lane group)
  // per four lanes, 16 rows per wave instruction
  const int sj = lane & 3, sr = lane >> 2;

  auto load_w = [&](W4Stage& st, int s, int n) {
#pragma unroll
    for (int p = 0; p < W4_CH; ++p) {
      // a step past the chunk repeats the chunk's last one: no branch
      const int sp_ = s + (p < n ? p : n - 1);
      st.w[p] = __builtin_nontemporal_load(
          reinterpret_cast<const u32x4*>(wp + (size_t)sp_ * 64));
      st.sc[p] = *reinterpret_cast<const unsigned int*>(sp + (size_t)sp_ * 4);
    }
  };
  auto load_x = [&](u32x4 (&xr)[XLOADS], int s, int n) {
#pragma unroll
    for (int it = 0; it < XLOADS; ++it) {
      const int combo = it * WAVES + wave;
      const int xg = combo & 3, u = (combo >> 2) % MT, sc = combo / (4 * MT);
      const int m = 16 * u + sr;
      const int sx = s + (sc < n ? sc : n - 1);
      xr[it] = *reinterpret_cast<const u32x4*>(
          X + (size_t)(m < M ? m : 0) * K + (size_t)sx * 128 + 32 * xg +
          8 * sj);
    }
  };
  auto store_x = [&](int b, const u32x4 (&xr)[XLOADS]) {
#pragma unroll
    for (int it = 0; it < XLOADS; ++it) {
      const int combo = it * WAVES + wave;
      const int xg = combo & 3, u = (combo >> 2) % MT, sc = combo / (4 * MT);
      xs[b][((sc * MT + u) * 4 + sj) * W4_PLANE + 16 * xg + sr] = xr[it];
    }
  };

  float4v acc[MT];
#pragma unroll
  for (int u = 0; u < MT; ++u) acc[u] = float4v{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](const W4Stage& st, int b, int n) {
#pragma unroll
    for (int p = 0; p < W4_CH; ++p) {
      if (p < n) {
        const float scale = w4_scale((st.sc[p] >> (8 * g)) & 0xffu);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bf16x8 a = w4_cvt(st.w[p][j], scale);
#pragma unroll
          for (int u = 0; u < MT; ++u) {
            const u32x4 xv = xs[b][((p * MT + u) * 4 + j) * W4_PLANE + lane];
            acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a, __builtin_bit_cast(bf16x8, xv), acc[u], 0, 0, 0);
          }
        }
      }
    }
  };

  // the block's groups enter their subtree in order: a binary counter of
  // pending sums, st0 one group, st1 two, st2 four; `top` ends as the sum
  float4v st0[MT], st1[MT], st2[MT], top[MT];
  auto push = [&](const float4v (&v)[MT], int i) {
#pragma unroll
    for (int u = 0; u < MT; ++u) {
      float4v t = v[u];
      if (GPB == 1) { top[u] = t; continue; }
      if (!(i & 1)) { st0[u] = t; continue; }
      t = w4_add(st0[u], t);
      if (GPB == 2) { top[u] = t; continue; }
      if (!(i & 2)) { st1[u] = t; continue; }
      t = w4_add(st1[u], t);
      if (GPB == 4) { top[u] = t; continue; }
      if (!(i & 4)) { st2[u] = t; continue; }
      top[u] = w4_add(st2[u], t);
    }
  };
  float4v zero[MT];
#pragma unroll
  for (int u = 0; u < MT; ++u) zero[u] = float4v{0.f, 0.f, 0.f, 0.f};

  int i = 0;  // groups pushed so far
  int s = gbeg(q0);
  if (s < se) {
    // the chunk at step s: its group, and its length up to the group's end
    auto chunk = [&](int s_, int& q) {
      while (gbeg(q + 1) <= s_) ++q;
      const int left = gbeg(q + 1) - s_;
      return left < W4_CH ? left : W4_CH;
    };
    int q = q0;
    int n = chunk(s, q);
    W4Stage cur, nxt;
    u32x4 xr[XLOADS];
    load_w(cur, s, n);
    load_x(xr, s, n);
    store_x(0, xr);
    __syncthreads();
    int b = 0;
    while (true) {
      const int sn = s + n;
      const bool more = sn < se;
      int qn = q, nn = 0;
      if (more) {
        nn = chunk(sn, qn);
        load_w(nxt, sn, nn);
        load_x(xr, sn, nn);
      }
      compute(cur, b, n);
      if (!more || qn != q) {  // group q is complete
        for (; i < q - q0; ++i) push(zero, i);
        push(acc, i);
        ++i;
#pragma unroll
        for (int u = 0; u < MT; ++u) acc[u] = float4v{0.f, 0.f, 0.f, 0.f};
      }
      if (!more) break;
      // every wave finished reading buffer b^1 before the last barrier
      store_x(b ^ 1, xr);
      __syncthreads();
      cur = nxt;
      s = sn; n = nn; q = qn; b ^= 1;
    }
  }
  for (; i < GPB; ++i) push(zero, i);

  const int nc = n0 + 4 * g;
  if (nc >= N) return;
#pragma unroll
  for (int u = 0; u < MT; ++u) {
    const int m = 16 * u + r16;
    if (m >= M) continue;
    if (GPB < W4_GROUPS) {
      float* wo = ws + ((size_t)blockIdx.y * M + m) * N + nc;
      if (N % 4 == 0) {
        *reinterpret_cast<float4v*>(wo) = top[u];
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (nc + r < N) wo[r] = top[u][r];
      }
    } else {
      short* yp = Y + (size_t)m * N + nc;
      if (N % 4 == 0) {
        short4v o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = f2bf(top[u][r]);
        *reinterpret_cast<short4v*>(yp) = o;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (nc + r < N) yp[r] = f2bf(top[u][r]);
      }
    }
  }
}

// The rest of the tree over the S slices' partials ws[S][total], then one
// rounding to bf16.
template <int S>
__global__ __launch_bounds__(256) void linear_w4_combine(
    const float* __restrict__ ws, short* __restrict__ Y, long long total) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  float v[S];
#pragma unroll
  for (int z = 0; z < S; ++z) v[z] = ws[z * total + e];
#pragma unroll
  for (int w = 1; w < S; w *= 2)
#pragma unroll
    for (int z = 0; z < S; z += 2 * w) v[z] = w4_scalar(v[z] + v[z + w]);
  Y[e] = f2bf(v[0]);
}

// MXFP4 -> bf16 [N, K], exact: a thread takes one MX block (16 bytes of
// nibbles, one scale byte) and stores its 32 bf16 as four 16-byte stores.
__global__ __launch_bounds__(256) void dequant_mxfp4_kernel(
    const unsigned char* __restrict__ Wq, const unsigned char* __restrict__ Sc,
    short* __restrict__ out, long long blocks) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= blocks) return;
  const u32x4 w =
      __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(Wq) + e);
  const float scale = w4_scale(Sc[e]);
  u32x4* o = reinterpret_cast<u32x4*>(out) + 4 * e;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    o[j] = __builtin_bit_cast(u32x4, w4_cvt(w[j], scale));
}
