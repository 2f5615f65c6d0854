// Mixture-of-experts FFN (Mixtral semantics), inference only:
//   logit[m, e] = x[m] · Wr[e]                      fp32
//   idx[m, 0..k) = the k largest logits, ties to the lower expert index
//   w[m, j]      = softmax over the k chosen logits, slot 0 the largest
//   h[p]         = bf16( silu(x[m] Wg[e]^T) * (x[m] Wu[e]^T) ),  p = m*k + j,
//   y[m]         = bf16( r[m] + sum_j w[p] * (h[p] · Wd[e]^T) )  e = idx[p]
// x [M, H] bf16, Wr [E, H], Wg, Wu [E, I, H], Wd [E, H, I] bf16 contiguous,
// E 2..64, k 1..8, H % 128 == 0, I % 128 == 0, fp32 accumulation, the sum
// over j in slot order. Included after linear_w4.hip in the one translation
// unit (bf16x8, u32x4, w4_add).
//
// Five launches whose grids and workspaces depend on (M, E, k, H, I) only:
// nothing on the host looks at the routing, so a captured graph serves any
// routing. No float atomics and no cross-block counters: every output
// element has one writer and every sum a fixed order.
//
// moe_route_kernel: one wave a row. The lanes split H in 16-byte units and
// keep eight experts' partial dots at a time, so x is read once per eight
// experts; a dot is summed over the wave by an xor butterfly (each lane adds
// the same pairs, so all lanes hold the same bits). Lane e keeps logit e.
// The top-k is k wave-wide arg-max passes under the total order (larger
// value, then lower index); logits are clamped to finite values first, so
// the winner is always a real expert. The weights are exp(l_j - l_0) over
// their sum in slot order.
//
// moe_align_kernel: one block of 1024 threads turns idx [M*k] into the
// per-expert pair lists. `lists` is one int32 tensor of 3*G + P words with
// P = M*k and G = ceil(P/64) + E:
//   [0, G)    group_expert    [G, 2G)  group_start    [2G, 3G)  group_count
//   [3G, ..)  the pairs p sorted by expert, ascending p within an expert
// A group is up to 64 pairs of one expert (four MFMA column tiles), the unit
// of work of an expert-GEMM block; sum_e ceil(c_e/64) <= P/64 + E, and the
// groups past the last real one have count 0. Histogram with LDS integer
// atomics (a count does not depend on their order), prefix by one thread,
// then an ordered scatter 1024 pairs at a time: within a wave a pair's rank
// among its expert's pairs is a ballot/popcount, across the 16 waves the
// per-wave counts are added in wave order, across chunks a per-expert cursor
// advances. A pair whose idx is outside 0..E-1 is in no list: no expert
// kernel touches it and the combine skips it.
//
// moe_gate_up_kernel / moe_down_kernel: grid (N / (16*NTI), G), 8 waves.
// A block owns one group and 16*NTI output channels of its expert. Operand
// roles as in lora.hip: v_mfma_f32_16x16x32_bf16, expert weights as A
// (16 channels x k) straight from global memory, the group's gathered rows
// as B (k x 16 pairs), C lane l = C[4*(l>>4)+r][l&15]. A wave step is 128 k
// (lane (r, g) loads the 64 contiguous bytes at k = 128*step + 32*g of its
// row as four 16-byte loads, MFMA j takes load j of both operands), each
// weight fragment is loaded once and feeds up to four MFMAs (one per tile of
// 16 pairs). The steps go round-robin to the 8 waves; the waves'
// accumulators are summed through LDS in wave order 0..7 by waves 0..3
// (wave = pair tile). Gate and up of one (pair, channel) end in the same
// lane, so SwiGLU is applied in registers before the one bf16 store of h.
// The down kernel reads h[p], multiplies by w[p] and writes fp32 ws[p, :].
// Missing pairs of the last tile repeat the group's first pair and land in
// accumulator columns that are never stored. A group with count 0 ends its
// blocks at once: an expert nobody chose costs no weight traffic.
//
// moe_combine_kernel: y[m] = bf16(sum_j ws[m*k + j] (+ r[m])), j ascending.

#define MOE_MAX_E 64
#define MOE_MAX_K 8
#define MOE_ALIGN_THREADS 1024

DEV_INLINE float moe_dot8(const u32x4& a, const u32x4& b, float acc) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc += __builtin_bit_cast(float, a[i] << 16) *
           __builtin_bit_cast(float, b[i] << 16);
    acc += __builtin_bit_cast(float, a[i] & 0xffff0000u) *
           __builtin_bit_cast(float, b[i] & 0xffff0000u);
  }
  return acc;
}

__global__ __launch_bounds__(256) void moe_route_kernel(
    const short* __restrict__ X, const short* __restrict__ Wr,
    int* __restrict__ idx, float* __restrict__ wts, int M, int H, int E,
    int k) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;  // uniform over the wave; the kernel has no barrier
  const int units = H >> 3;
  const u32x4* xp = reinterpret_cast<const u32x4*>(X + (size_t)m * H);
  float mine = -INFINITY;
  for (int e0 = 0; e0 < E; e0 += 8) {
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    for (int u = lane; u < units; u += 64) {
      const u32x4 xv = xp[u];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (e0 + i < E)
          acc[i] = moe_dot8(
              xv,
              reinterpret_cast<const u32x4*>(Wr + (size_t)(e0 + i) * H)[u],
              acc[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float s = acc[i];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (lane == e0 + i) mine = s;
    }
  }
  // finite, so a real expert always beats a taken or missing one
  mine = lane < E ? fminf(fmaxf(mine, -3.0e38f), 3.0e38f) : -INFINITY;
  float l0 = 0.f, sum = 0.f, myw = 0.f;
  int myi = 0;
  for (int j = 0; j < k; ++j) {
    float bv = mine;
    int bi = lane;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (j == 0) l0 = bv;
    const float ev = __expf(bv - l0);
    sum += ev;
    if (lane == j) {
      myw = ev;
      myi = bi;
    }
    if (lane == bi) mine = -INFINITY;
  }
  if (lane < k) {
    idx[(size_t)m * k + lane] = myi;
    wts[(size_t)m * k + lane] = myw / sum;
  }
}

__global__ __launch_bounds__(MOE_ALIGN_THREADS) void moe_align_kernel(
    const int* __restrict__ idx, int* __restrict__ lists, int P, int E,
    int G) {
  __shared__ int hist[MOE_MAX_E], seg[MOE_MAX_E], cursor[MOE_MAX_E];
  __shared__ int gbase[MOE_MAX_E + 1];
  __shared__ int cnt[MOE_ALIGN_THREADS / 64][MOE_MAX_E];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* g_expert = lists;
  int* g_start = lists + G;
  int* g_count = lists + 2 * (size_t)G;
  int* sorted = lists + 3 * (size_t)G;
  if (tid < MOE_MAX_E) {
    hist[tid] = 0;
    cursor[tid] = 0;
  }
  __syncthreads();
  for (int p = tid; p < P; p += MOE_ALIGN_THREADS) {
    const int e = idx[p];
    if ((unsigned)e < (unsigned)E) atomicAdd(&hist[e], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int s = 0, g = 0;
    for (int e = 0; e < E; ++e) {
      seg[e] = s;
      gbase[e] = g;
      s += hist[e];
      g += (hist[e] + 63) >> 6;
    }
    gbase[E] = g;
  }
  __syncthreads();
  for (int e = wave; e < E; e += MOE_ALIGN_THREADS / 64)
    for (int i = lane; i < gbase[e + 1] - gbase[e]; i += 64) {
      const int gi = gbase[e] + i;
      g_expert[gi] = e;
      g_start[gi] = seg[e] + 64 * i;
      g_count[gi] = min(64, hist[e] - 64 * i);
    }
  for (int gi = gbase[E] + tid; gi < G; gi += MOE_ALIGN_THREADS) {
    g_expert[gi] = 0;
    g_start[gi] = 0;
    g_count[gi] = 0;
  }
  // ordered scatter; every trip count below is uniform over the block
  for (int base = 0; base < P; base += MOE_ALIGN_THREADS) {
    const int p = base + tid;
    const int e = p < P ? idx[p] : -1;
    const bool valid = (unsigned)e < (unsigned)E;
    cnt[wave][lane] = 0;
    int rank = 0;
    unsigned long long todo = __ballot(valid);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int e0 = __shfl(e, leader, 64);
      const bool same = valid && e == e0;
      const unsigned long long mask = __ballot(same);
      if (same) rank = __popcll(mask & ((1ull << lane) - 1ull));
      if (lane == leader) cnt[wave][e0] = __popcll(mask);
      todo &= ~mask;
    }
    __syncthreads();
    if (valid) {
      int b = cursor[e];
      for (int w = 0; w < wave; ++w) b += cnt[w][e];
      sorted[seg[e] + b + rank] = p;
    }
    __syncthreads();
    if (tid < E) {
      int s = 0;
      for (int w = 0; w < MOE_ALIGN_THREADS / 64; ++w) s += cnt[w][tid];
      cursor[tid] += s;
    }
    __syncthreads();
  }
}

// acc[w][t][u] += W_w[16 channels of tile t] x (16 pairs of tile u), over
// the 128-k steps wave, wave + 8, ...
template <int NW, int NTI>
DEV_INLINE void moe_mma(const short* const (&wp)[NW],
                        const short* const (&bp)[4], int K, int ng, int wave,
                        float4v (&acc)[NW][NTI][4]) {
  const int steps = K >> 7;
  for (int st = wave; st < steps; st += 8) {
    const size_t k0 = (size_t)st * 128;
    u32x4 a[NW][NTI][4];
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
      for (int t = 0; t < NTI; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          a[w][t][j] = *reinterpret_cast<const u32x4*>(
              wp[w] + (size_t)(16 * t) * K + k0 + 8 * j);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (u < ng) {
        u32x4 b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          b[j] = *reinterpret_cast<const u32x4*>(bp[u] + k0 + 8 * j);
#pragma unroll
        for (int w = 0; w < NW; ++w)
#pragma unroll
          for (int t = 0; t < NTI; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              acc[w][t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  __builtin_bit_cast(bf16x8, a[w][t][j]),
                  __builtin_bit_cast(bf16x8, b[j]), acc[w][t][u], 0, 0, 0);
      }
    }
  }
}

// out[w][t] of wave u < ng, lane (r16, g): channels 16t + 4g .. +3 of pair
// 16u + r16, the 8 waves' partials added in wave order
template <int NW, int NTI>
DEV_INLINE void moe_reduce(const float4v (&acc)[NW][NTI][4],
                           float4v (*red)[4][64], int ng, int wave, int lane,
                           float4v (&out)[NW][NTI]) {
#pragma unroll
  for (int w = 0; w < NW; ++w)
#pragma unroll
    for (int t = 0; t < NTI; ++t) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (u < ng) red[wave][u][lane] = acc[w][t][u];
      __syncthreads();
      if (wave < ng) {
        float4v sum = red[0][wave][lane];
        for (int v = 1; v < 8; ++v) sum = w4_add(sum, red[v][wave][lane]);
        out[w][t] = sum;
      }
      __syncthreads();
    }
}

template <int NW, int NTI>
DEV_INLINE void moe_zero(float4v (&acc)[NW][NTI][4]) {
#pragma unroll
  for (int w = 0; w < NW; ++w)
#pragma unroll
    for (int t = 0; t < NTI; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[w][t][u] = float4v{0.f, 0.f, 0.f, 0.f};
}

template <int NTI>
__global__ __launch_bounds__(512) void moe_gate_up_kernel(
    const short* __restrict__ X, const short* __restrict__ Wg,
    const short* __restrict__ Wu, const int* __restrict__ lists,
    short* __restrict__ Hout, int k, int H, int I, int G) {
  __shared__ float4v red[8][4][64];
  const int gi = blockIdx.y;
  const int count = lists[2 * (size_t)G + gi];
  if (count == 0) return;  // uniform over the block
  const int e = lists[gi];
  const int* list = lists + 3 * (size_t)G + lists[G + gi];
  const int ng = (count + 15) >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int r16 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (16 * NTI);

  const short* bp[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int li = 16 * u + r16;
    bp[u] = X + (size_t)(list[li < count ? li : 0] / k) * H + 32 * g;
  }
  const size_t wrow = ((size_t)e * I + n0 + r16) * H + 32 * g;
  const short* wp[2] = {Wg + wrow, Wu + wrow};

  float4v acc[2][NTI][4], out[2][NTI];
  moe_zero<2, NTI>(acc);
  moe_mma<2, NTI>(wp, bp, H, ng, wave, acc);
  moe_reduce<2, NTI>(acc, red, ng, wave, lane, out);

  const int li = 16 * wave + r16;
  if (wave < ng && li < count) {
    short* hp = Hout + (size_t)list[li] * I + n0 + 4 * g;
#pragma unroll
    for (int t = 0; t < NTI; ++t) {
      short4v o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float gt = out[0][t][r];
        o[r] = f2bf(gt / (1.f + __expf(-gt)) * out[1][t][r]);
      }
      *reinterpret_cast<short4v*>(hp + 16 * t) = o;
    }
  }
}

template <int NTI>
__global__ __launch_bounds__(512) void moe_down_kernel(
    const short* __restrict__ Hin, const short* __restrict__ Wd,
    const float* __restrict__ wts, const int* __restrict__ lists,
    float* __restrict__ ws, int H, int I, int G) {
  __shared__ float4v red[8][4][64];
  const int gi = blockIdx.y;
  const int count = lists[2 * (size_t)G + gi];
  if (count == 0) return;  // uniform over the block
  const int e = lists[gi];
  const int* list = lists + 3 * (size_t)G + lists[G + gi];
  const int ng = (count + 15) >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int r16 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (16 * NTI);

  const short* bp[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int li = 16 * u + r16;
    bp[u] = Hin + (size_t)list[li < count ? li : 0] * I + 32 * g;
  }
  const short* wp[1] = {Wd + ((size_t)e * H + n0 + r16) * I + 32 * g};

  float4v acc[1][NTI][4], out[1][NTI];
  moe_zero<1, NTI>(acc);
  moe_mma<1, NTI>(wp, bp, I, ng, wave, acc);
  moe_reduce<1, NTI>(acc, red, ng, wave, lane, out);

  const int li = 16 * wave + r16;
  if (wave < ng && li < count) {
    const int p = list[li];
    const float wp_ = wts[p];
    float* op = ws + (size_t)p * H + n0 + 4 * g;
#pragma unroll
    for (int t = 0; t < NTI; ++t) {
      float4v o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = w4_scalar(wp_ * out[0][t][r]);
      *reinterpret_cast<float4v*>(op + 16 * t) = o;
    }
  }
}

__global__ __launch_bounds__(256) void moe_combine_kernel(
    const float* __restrict__ ws, const int* __restrict__ idx,
    const short* __restrict__ res, short* __restrict__ Y, long long total,
    int k, int H, int E) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int q = H >> 2;
  const long long m = t / q;
  const int c = 4 * (int)(t % q);
  float4v sum = float4v{0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < k; ++j)
    if ((unsigned)idx[m * k + j] < (unsigned)E)
      sum = w4_add(sum, *reinterpret_cast<const float4v*>(
                            ws + (size_t)(m * k + j) * H + c));
  if (res != nullptr) {
    const short4v rv =
        *reinterpret_cast<const short4v*>(res + (size_t)m * H + c);
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[r] = w4_scalar(sum[r] + bf2f(rv[r]));
  }
  short4v o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = f2bf(sum[r]);
  *reinterpret_cast<short4v*>(Y + (size_t)m * H + c) = o;
}
