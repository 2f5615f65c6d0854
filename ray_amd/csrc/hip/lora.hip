// Batched per-row LoRA (multi-adapter serving):
//   y[m, :] += scale[s] * (x[m, :] · A[s]^T) · B[s]^T,   s = idx[m]
// x [M, K] bf16, y [M, N] bf16 updated in place, A [S, R, K] bf16,
// B [S, N, R] bf16, scale [S] fp32, idx [M] int32 in device memory with
// entries -1 (no adapter) or 0..S-1. R is 16, 32 or 64 (smaller ranks are
// stored zero-padded), K % 128 == 0, N % 128 == 0, fp32 accumulation.
// Included after linear_w4.hip in the one translation unit (bf16x8, u32x4).
//
// Two launches whose grids depend on (M, N, K, S) only: nothing on the host
// looks at idx, so a captured graph serves any mix of adapters. A row whose
// idx is -1 (or outside 0..S-1) is in no block's list: its x is never read
// and its y never touched.
//
// Row compaction, both kernels. A block belongs to one adapter s and one
// chunk of 64 rows. Every wave loads the chunk's 64 idx entries, one a lane;
// the ballot of idx == s is the chunk's membership mask, the same in every
// wave; the lane's position in the list is the popcount of the mask below
// it, so the list is in ascending row order whatever the timing. Wave 0
// writes the list to LDS. An empty list ends the block. Listed rows are
// taken in groups of 16 (one MFMA's columns), up to four; a group's missing
// rows repeat the list's first row and land in accumulator columns that are
// never stored (an MFMA column depends on its own B column only).
//
// MFMA and operand roles as in linear_w4.hip: v_mfma_f32_16x16x32_bf16,
// adapter weights as A (16 ranks or 16 channels x k), activations as B
// (k x 16 listed rows), C lane l = C[4*(l>>4)+r][l&15].
//
// Shrink: ws[kz][m][0..R) = x[m, slice kz] · A[s][:, slice kz]^T, fp32.
// Grid (ceil(M/64), ksplit, S), 8 waves (the row chunks are the dimension
// without a 65535 limit). A wave step is 128 k, not 32: lane
// (r, g) loads the 64 contiguous bytes of its row at k = 128*step + 32*g as
// four 16-byte loads and MFMA j takes load j from both operands (the k
// permutation of linear_w4.hip: fragment element (g, i) of MFMA j is
// k = 128*step + 32*g + 8*j + i, for A[s] and for x alike), so the four lane
// groups read 256 contiguous bytes of every row instead of 64. A[s]'s
// fragments of a step (R/16 tiles x 4) are loaded once and reused by every
// row group. The slice's steps go round-robin to the 8 waves; the waves'
// accumulators are summed through LDS in wave order 0..7, one rank tile at
// a time (32 KB), by threads 0..255 (thread = group * 64 + lane), which
// store 16 bytes each. A slice without steps (forced splits at K = 128)
// stores zeros. Rows that are in no list are neither written nor read later.
//
// Expand: y[m, n0..n0+128) += scale[s] * bf16(h[m]) · B[s][n0.., :]^T.
// Grid (ceil(M/64), N/128, S), 4 waves x 32 channels (two tiles of 16).
// The block sums the ksplit partials of its listed rows in order kz = 0..,
// rounds h to bf16 once and stores it in LDS in fragment order (one plane of
// 64 16-byte units per (32 ranks, row group), unit = lane), so a B fragment
// is one conflict-free 16-byte read. R = 16 uses the same MFMA with the
// upper half of k zero in both operands (lane groups 2 and 3 hold zeros and
// load nothing). The epilogue reads a lane's four consecutive channels of y,
// adds scale * acc in fp32, rounds once and stores 8 bytes. A row has one
// adapter, so each (m, n) belongs to exactly one block: no atomics, no race,
// and the result depends on (K, ksplit) only.

DEV_INLINE int lora_compact(const int* __restrict__ idx, int M, int m0, int s,
                            int* list) {
  const int lane = threadIdx.x & 63;
  const int m = m0 + lane;
  const bool hit = m < M && idx[m] == s;
  const unsigned long long mask = __ballot(hit);
  if (threadIdx.x < 64 && hit)
    list[__popcll(mask & ((1ull << lane) - 1ull))] = m;
  __syncthreads();
  return __popcll(mask);
}

template <int R>
__global__ __launch_bounds__(512) void lora_shrink_kernel(
    const short* __restrict__ X, const short* __restrict__ A,
    const int* __restrict__ idx, float* __restrict__ ws, int M, int K) {
  constexpr int RT = R / 16;
  __shared__ int list[64];
  __shared__ float4v red[8][4][64];
  const int s = blockIdx.z, kz = blockIdx.y;
  const int count = lora_compact(idx, M, blockIdx.x * 64, s, list);
  if (count == 0) return;  // uniform over the block
  const int ng = (count + 15) >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int r16 = lane & 15, g = lane >> 4;
  const int steps = K / 128;
  const int beg = (int)((long long)steps * kz / gridDim.y);
  const int end = (int)((long long)steps * (kz + 1) / gridDim.y);

  const short* xp[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int li = 16 * u + r16;
    xp[u] = X + (size_t)list[li < count ? li : 0] * K + 32 * g;
  }
  const short* ap = A + ((size_t)s * R + r16) * K + 32 * g;

  float4v acc[RT][4];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[t][u] = float4v{0.f, 0.f, 0.f, 0.f};

  for (int st = beg + wave; st < end; st += 8) {
    const size_t k0 = (size_t)st * 128;
    u32x4 a[RT][4];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        a[t][j] = *reinterpret_cast<const u32x4*>(ap + (size_t)(16 * t) * K +
                                                  k0 + 8 * j);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (u < ng) {
        u32x4 b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          b[j] = *reinterpret_cast<const u32x4*>(xp[u] + k0 + 8 * j);
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                __builtin_bit_cast(bf16x8, a[t][j]),
                __builtin_bit_cast(bf16x8, b[j]), acc[t][u], 0, 0, 0);
      }
    }
  }

  // thread (group u = wave, lane) of the first four waves owns ranks
  // 16t + 4g .. +3 of listed row 16u + r16
  const int li = 16 * wave + r16;
  const bool owner = wave < ng && li < count;
  float* wo = nullptr;
  if (owner) wo = ws + ((size_t)kz * M + list[li]) * R + 4 * g;
#pragma unroll
  for (int t = 0; t < RT; ++t) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (u < ng) red[wave][u][lane] = acc[t][u];
    __syncthreads();
    if (owner) {
      float4v sum = red[0][wave][lane];
      for (int w = 1; w < 8; ++w) sum = w4_add(sum, red[w][wave][lane]);
      *reinterpret_cast<float4v*>(wo + 16 * t) = sum;
    }
    __syncthreads();
  }
}

template <int R>
__global__ __launch_bounds__(256) void lora_expand_kernel(
    const float* __restrict__ ws, const short* __restrict__ Bw,
    const float* __restrict__ scale, const int* __restrict__ idx,
    short* __restrict__ Y, int M, int N, int ksplit) {
  constexpr int KK = R >= 32 ? R / 32 : 1;  // MFMAs along the rank
  constexpr int QR = R / 4;                 // 4-rank pieces per row
  __shared__ int list[64];
  __shared__ u32x4 hs[KK * 4 * 64];
  const int s = blockIdx.z;
  const int count = lora_compact(idx, M, blockIdx.x * 64, s, list);
  if (count == 0) return;  // uniform over the block
  const int ng = (count + 15) >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int r16 = lane & 15, g = lane >> 4;
  // R = 16: the upper half of the MFMA's k is zero in both operands
  const bool live = R >= 32 || g < 2;

  // h = sum of the partials in slice order, one rounding to bf16, stored
  // as the B fragments: rank c of listed row i goes to plane (c/32, i/16),
  // unit (c%32/8)*16 + i%16, element c%8
  short4v* hq = reinterpret_cast<short4v*>(hs);
  for (int e = threadIdx.x; e < ng * 16 * QR; e += 256) {
    const int i = e / QR, c = 4 * (e % QR);
    float4v sum = float4v{0.f, 0.f, 0.f, 0.f};
    if (i < count) {
      const float* p = ws + (size_t)list[i] * R + c;
      sum = *reinterpret_cast<const float4v*>(p);
      for (int z = 1; z < ksplit; ++z)
        sum = w4_add(sum, *reinterpret_cast<const float4v*>(
                              p + (size_t)z * M * R));
    }
    short4v o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = f2bf(sum[r]);
    const int unit =
        ((c >> 5) * 4 + (i >> 4)) * 64 + ((c & 31) >> 3) * 16 + (i & 15);
    hq[2 * unit + ((c & 7) >> 2)] = o;
  }

  const int n0 = blockIdx.y * 128 + 32 * wave;
  const u32x4 zero = u32x4{0u, 0u, 0u, 0u};
  u32x4 a[2][KK];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int kk = 0; kk < KK; ++kk)
      a[t][kk] = live ? *reinterpret_cast<const u32x4*>(
                            Bw + ((size_t)s * N + n0 + 16 * t + r16) * R +
                            32 * kk + 8 * g)
                      : zero;
  const float sc = scale[s];
  __syncthreads();

#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (u < ng) {
      float4v acc[2] = {float4v{0.f, 0.f, 0.f, 0.f},
                        float4v{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const u32x4 b = live ? hs[(kk * 4 + u) * 64 + lane] : zero;
#pragma unroll
        for (int t = 0; t < 2; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              __builtin_bit_cast(bf16x8, a[t][kk]),
              __builtin_bit_cast(bf16x8, b), acc[t], 0, 0, 0);
      }
      const int li = 16 * u + r16;
      if (li < count) {
        short* yp = Y + (size_t)list[li] * N + n0 + 4 * g;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          short4v o = *reinterpret_cast<const short4v*>(yp + 16 * t);
#pragma unroll
          for (int r = 0; r < 4; ++r)
            o[r] = f2bf(w4_scalar(bf2f(o[r]) + w4_scalar(sc * acc[t][r])));
          *reinterpret_cast<short4v*>(yp + 16 * t) = o;
        }
      }
    }
  }
}
