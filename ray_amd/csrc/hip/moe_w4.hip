// Routed expert GEMMs over MXFP4 expert weights (W4A16), inference only.
// Semantics are those of moe.hip's header with other weight storage:
//   Wg, Wu uint8 [E, I, H/2] + e8m0 scales uint8 [E, I, H/32],
//   Wd     uint8 [E, H, I/2] + scales [E, H, I/32]
// (ops.quantize_weight_mxfp4 of w.reshape(E*N, K), reshaped back). x, h, y
// bf16, fp32 accumulation, h rounded to bf16 once, the sum over slots in
// slot order. Conversion is linear_w4.hip's exact w4_cvt / w4_scale, so the
// kernels compute with precisely the bf16 values dequant_mxfp4 returns.
// H % 128 == 0, I % 128 == 0, E 2..64, k 1..8. moe_route_kernel,
// moe_align_kernel, the `lists` format and moe_combine_kernel are moe.hip's.
// Included after moe.hip in the one translation unit.
//
// Work split. At 17/32 byte per weight a block of 16 or 32 channels (the
// bf16 split) would spend its time on the gathered rows, which it re-reads
// from L2 once per channel slice (the argument of linear_w4.hip's header).
// Here a block owns one group (up to 64 pairs of one expert) and 128 output
// channels of that expert: grid (N / 128, G, S). The 8 waves split N, 16
// channels each, and every wave keeps whole K runs, so there is no 8-wave
// LDS reduction.
//
// Operands: roles and the k-permutation of linear_w4.hip. Weights are the A
// operand straight from global memory: lane (r, g) does one non-temporal
// 16-byte load per 128-k step (one MX block) and one dword scale load, of
// which lane group g takes byte g; MFMA j takes dword j, and the B fragment
// is gathered under the same k. In the gate/up kernel a wave streams the gate
// and the up row of its channels and applies SwiGLU in registers before the
// one bf16 store of h.
//
// Staging. The group's gathered rows (of x, or of h) are staged once per
// block in LDS in fragment order (unit index = lane, planes W4_PLANE units
// apart) for MT tiles of 16 pairs, double-buffered by K chunk: the next
// chunk's global loads are issued before this chunk's MFMAs and written to
// the other buffer after them, one barrier per chunk. MT (1, 2 or 4) is a
// template parameter the launcher picks from P = M*k alone (a group has at
// most min(64, P) pairs); the tiles past the group's ng = ceil(count/16) are
// neither loaded nor multiplied. The chunk is CH steps: 512 k (CH = 4) at
// MT = 1 and 256 k (CH = 2) at MT = 2 and 4, chosen from the compiler's
// resource report, not from a timing: the pair of buffers is then 34.8,
// 34.8 and 69.6 KB, so two blocks fit a CU's 160 KB of LDS, and the MT = 1
// and MT = 2 kernels stay within the 128 VGPRs that two 8-wave blocks a CU
// allow. A 512-k chunk needs 134 to 142 VGPRs at MT = 2 (one block a CU) and
// 139 KB of LDS at MT = 4. The MT = 4 kernels use 112 to 170 VGPRs even at
// 256 k (PERFORMANCE.md, "MXFP4 expert weights", has the table). Missing
// pairs of the last tile repeat the group's first pair and land in
// accumulator columns that are never stored. A group with count 0 ends its
// block before any load.
//
// K split (down kernel). 128-channel blocks are few (Mixtral's down
// projection at M = 1: 32 x 2 live groups), so K = I is also split over
// blockIdx.z into S = 1, 2, 4 or 8 slices; S comes from (M, E, k, H, I)
// only. The order of every fp32 sum is fixed by K alone, with linear_w4.hip's
// scheme: the K/128 steps are cut (floor split) into W4_GROUPS = 8 groups,
// each accumulates in step order from zero, and the group sums are added as
// the balanced tree ((g0+g1)+(g2+g3)) + ((g4+g5)+(g6+g7)). A block adds its
// aligned run of 8/S groups as their subtree in registers. S = 1 finishes
// the tree, multiplies by w[p] and writes ws[p, :], which moe_combine_kernel
// sums over the slots. S > 1 writes the subtree's unscaled fp32 sum to
// ws[z, p, :], and moe_w4_combine_kernel finishes the tree, multiplies by
// w[p] and sums the slots: the same operations on the same values, so every
// S gives the same bits. No atomics and no cross-block counters.
//
// Departure from the plan of record: the gate/up kernel is never split over
// K (I/128 x live groups is 224 blocks at Mixtral's M = 1 already), and so it
// does not build the 8-group tree either: its products accumulate in plain
// step order in the MFMA accumulator, which keeps the three-deep stack of
// two projections x MT tiles out of its registers. Its sums still have one
// order fixed by K alone.
//
// Out-of-range reads: none. N % 128 == 0, so every weight and scale row a
// lane touches exists; a step index never passes K/128; rows of x and h are
// reached only through list entries below the group's count.

template <int NW, int CH>
struct MoeW4Stage {
  u32x4 w[NW][CH];
  unsigned int sc[NW][CH];
};

// top[w][u] = W_w[the wave's 16 channels] x (the 16 pairs of tile u) over
// the steps of the groups q0 .. q0 + GPB - 1 (TREE: as their subtree; else
// q0 = 0, GPB = 8 and plain step order). B is x (div = k) or h (div = 1).
template <int NW, int MT, int CH, int GPB, bool TREE>
DEV_INLINE void moe_w4_core(const unsigned char* const (&wp)[NW],
                            const unsigned char* const (&sp)[NW],
                            const short* __restrict__ B, const int* list,
                            int count, int div, int K, int q0, u32x4* xs,
                            float4v (&top)[NW][MT]) {
  constexpr int XLOADS = CH * MT * 4 / 8;  // staging loads per thread
  constexpr int BUF = CH * MT * 4 * W4_PLANE;
  static_assert(CH * MT * 4 % 8 == 0, "staging must divide over the waves");
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;
  const int ng = (count + 15) >> 4;
  const int steps = K / 128;
  auto gbeg = [&](int q) { return (int)((long long)steps * q / W4_GROUPS); };
  const int se = gbeg(q0 + GPB);

  // staging role: 64 contiguous bytes of a row (the four j of one lane
  // group) per four lanes, 16 rows per wave instruction
  const int sj = lane & 3, sr = lane >> 2;
  const short* xrow[XLOADS];
#pragma unroll
  for (int it = 0; it < XLOADS; ++it) {
    const int combo = it * 8 + wave;
    const int xg = combo & 3, u = (combo >> 2) % MT;
    const int li = 16 * u + sr;
    xrow[it] = B + (size_t)(list[li < count ? li : 0] / div) * K + 32 * xg +
               8 * sj;
  }

  auto load_w = [&](MoeW4Stage<NW, CH>& st, int s, int n) {
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
      for (int p = 0; p < CH; ++p) {
        // a step past the chunk repeats the chunk's last one: no branch
        const int sp_ = s + (p < n ? p : n - 1);
        st.w[w][p] = __builtin_nontemporal_load(
            reinterpret_cast<const u32x4*>(wp[w] + (size_t)sp_ * 64));
        st.sc[w][p] =
            *reinterpret_cast<const unsigned int*>(sp[w] + (size_t)sp_ * 4);
      }
  };
  auto load_x = [&](u32x4 (&xr)[XLOADS], int s, int n) {
#pragma unroll
    for (int it = 0; it < XLOADS; ++it) {
      const int combo = it * 8 + wave;
      const int u = (combo >> 2) % MT, sc = combo / (4 * MT);
      if (u < ng) {  // uniform over the wave
        const int sx = s + (sc < n ? sc : n - 1);
        xr[it] =
            *reinterpret_cast<const u32x4*>(xrow[it] + (size_t)sx * 128);
      }
    }
  };
  auto store_x = [&](int b, const u32x4 (&xr)[XLOADS]) {
#pragma unroll
    for (int it = 0; it < XLOADS; ++it) {
      const int combo = it * 8 + wave;
      const int xg = combo & 3, u = (combo >> 2) % MT, sc = combo / (4 * MT);
      if (u < ng)
        xs[b * BUF + ((sc * MT + u) * 4 + sj) * W4_PLANE + 16 * xg + sr] =
            xr[it];
    }
  };

  float4v acc[NW][MT];
#pragma unroll
  for (int w = 0; w < NW; ++w)
#pragma unroll
    for (int u = 0; u < MT; ++u) acc[w][u] = float4v{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](const MoeW4Stage<NW, CH>& st, int b, int n) {
#pragma unroll
    for (int p = 0; p < CH; ++p) {
      if (p < n) {
        float scale[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w)
          scale[w] = w4_scale((st.sc[w][p] >> (8 * g)) & 0xffu);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bf16x8 a[NW];
#pragma unroll
          for (int w = 0; w < NW; ++w) a[w] = w4_cvt(st.w[w][p][j], scale[w]);
#pragma unroll
          for (int u = 0; u < MT; ++u) {
            if (u < ng) {
              const u32x4 xv =
                  xs[b * BUF + ((p * MT + u) * 4 + j) * W4_PLANE + lane];
#pragma unroll
              for (int w = 0; w < NW; ++w)
                acc[w][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    a[w], __builtin_bit_cast(bf16x8, xv), acc[w][u], 0, 0, 0);
            }
          }
        }
      }
    }
  };

  // the block's groups enter their subtree in order: a binary counter of
  // pending sums, st0 one group, st1 two, st2 four; `top` ends as the sum
  float4v st0[NW][MT], st1[NW][MT], st2[NW][MT];
  auto push = [&](const float4v (&v)[NW][MT], int i) {
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
      for (int u = 0; u < MT; ++u) {
        float4v t = v[w][u];
        if (GPB == 1) { top[w][u] = t; continue; }
        if (!(i & 1)) { st0[w][u] = t; continue; }
        t = w4_add(st0[w][u], t);
        if (GPB == 2) { top[w][u] = t; continue; }
        if (!(i & 2)) { st1[w][u] = t; continue; }
        t = w4_add(st1[w][u], t);
        if (GPB == 4) { top[w][u] = t; continue; }
        if (!(i & 4)) { st2[w][u] = t; continue; }
        top[w][u] = w4_add(st2[w][u], t);
      }
  };
  float4v zero[NW][MT];
#pragma unroll
  for (int w = 0; w < NW; ++w)
#pragma unroll
    for (int u = 0; u < MT; ++u) zero[w][u] = float4v{0.f, 0.f, 0.f, 0.f};

  int i = 0;  // groups pushed so far
  int s = gbeg(q0);
  if (s < se) {
    // the chunk at step s: its group, and its length up to the group's end
    // (TREE) or the last step
    auto chunk = [&](int s_, int& q) {
      int left = se - s_;
      if (TREE) {
        while (gbeg(q + 1) <= s_) ++q;
        left = gbeg(q + 1) - s_;
      }
      return left < CH ? left : CH;
    };
    int q = q0;
    int n = chunk(s, q);
    MoeW4Stage<NW, CH> cur, nxt;
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
      if (TREE && (!more || qn != q)) {  // group q is complete
        for (; i < q - q0; ++i) push(zero, i);
        push(acc, i);
        ++i;
#pragma unroll
        for (int w = 0; w < NW; ++w)
#pragma unroll
          for (int u = 0; u < MT; ++u)
            acc[w][u] = float4v{0.f, 0.f, 0.f, 0.f};
      }
      if (!more) break;
      // every wave finished reading buffer b^1 before the last barrier
      store_x(b ^ 1, xr);
      __syncthreads();
      cur = nxt;
      s = sn; n = nn; q = qn; b ^= 1;
    }
  }
  if (TREE) {
    for (; i < GPB; ++i) push(zero, i);
  } else {
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
      for (int u = 0; u < MT; ++u) top[w][u] = acc[w][u];
  }
}

// grid (I / 128, G), 8 waves
template <int MT, int CH>
__global__ __launch_bounds__(512) void moe_gate_up_w4_kernel(
    const short* __restrict__ X, const unsigned char* __restrict__ Wg,
    const unsigned char* __restrict__ Sg, const unsigned char* __restrict__ Wu,
    const unsigned char* __restrict__ Su, const int* __restrict__ lists,
    short* __restrict__ Hout, int k, int H, int I, int G) {
  __shared__ u32x4 xs[2 * CH * MT * 4 * W4_PLANE];
  const int gi = blockIdx.y;
  const int count = lists[2 * (size_t)G + gi];
  if (count == 0) return;  // uniform over the block
  const int e = lists[gi];
  const int* list = lists + 3 * (size_t)G + lists[G + gi];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int r16 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 128 + 16 * wave;

  const size_t row = (size_t)e * I + n0 + r16;
  const unsigned char* wp[2] = {Wg + row * (H / 2) + 16 * g,
                                Wu + row * (H / 2) + 16 * g};
  const unsigned char* sp[2] = {Sg + row * (H / 32), Su + row * (H / 32)};
  float4v top[2][MT];
  moe_w4_core<2, MT, CH, W4_GROUPS, false>(wp, sp, X, list, count, k, H, 0,
                                           xs, top);
#pragma unroll
  for (int u = 0; u < MT; ++u) {
    const int li = 16 * u + r16;
    if (li < count) {
      short4v o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float gt = top[0][u][r];
        o[r] = f2bf(gt / (1.f + __expf(-gt)) * top[1][u][r]);
      }
      *reinterpret_cast<short4v*>(Hout + (size_t)list[li] * I + n0 + 4 * g) =
          o;
    }
  }
}

// grid (H / 128, G, 8 / GPB), 8 waves. GPB == 8: ws [P, H] holds w[p] times
// the finished sum; else ws [8 / GPB, P, H] holds the slices' subtree sums.
template <int MT, int CH, int GPB>
__global__ __launch_bounds__(512) void moe_down_w4_kernel(
    const short* __restrict__ Hin, const unsigned char* __restrict__ Wd,
    const unsigned char* __restrict__ Sd, const float* __restrict__ wts,
    const int* __restrict__ lists, float* __restrict__ ws, int P, int H,
    int I, int G) {
  __shared__ u32x4 xs[2 * CH * MT * 4 * W4_PLANE];
  const int gi = blockIdx.y;
  const int count = lists[2 * (size_t)G + gi];
  if (count == 0) return;  // uniform over the block
  const int e = lists[gi];
  const int* list = lists + 3 * (size_t)G + lists[G + gi];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int r16 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 128 + 16 * wave;

  const size_t row = (size_t)e * H + n0 + r16;
  const unsigned char* wp[1] = {Wd + row * (I / 2) + 16 * g};
  const unsigned char* sp[1] = {Sd + row * (I / 32)};
  float4v top[1][MT];
  moe_w4_core<1, MT, CH, GPB, true>(wp, sp, Hin, list, count, 1, I,
                                    blockIdx.z * GPB, xs, top);
#pragma unroll
  for (int u = 0; u < MT; ++u) {
    const int li = 16 * u + r16;
    if (li < count) {
      const int p = list[li];
      float4v o = top[0][u];
      size_t at = (size_t)p * H;
      if (GPB == W4_GROUPS) {
        const float wp_ = wts[p];
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = w4_scalar(wp_ * o[r]);
      } else {
        at += (size_t)blockIdx.z * P * H;
      }
      *reinterpret_cast<float4v*>(ws + at + n0 + 4 * g) = o;
    }
  }
}

// The rest of the tree over the S slices' partials ws [S, P, H], times w[p],
// summed over the slots in ascending order (+ r[m]), one rounding to bf16:
// what moe_down_w4_kernel<.., 8> and moe_combine_kernel do for S = 1.
template <int S>
__global__ __launch_bounds__(256) void moe_w4_combine_kernel(
    const float* __restrict__ ws, const float* __restrict__ wts,
    const int* __restrict__ idx, const short* __restrict__ res,
    short* __restrict__ Y, long long total, int k, int H, int E) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int q = H >> 2;
  const long long m = t / q;
  const int c = 4 * (int)(t % q);
  const size_t slice = (size_t)(total / q) * k * H;  // P * H
  float4v sum = float4v{0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < k; ++j) {
    const long long p = m * k + j;
    if ((unsigned)idx[p] >= (unsigned)E) continue;
    float4v v[S];
#pragma unroll
    for (int z = 0; z < S; ++z)
      v[z] = *reinterpret_cast<const float4v*>(ws + z * slice +
                                               (size_t)p * H + c);
#pragma unroll
    for (int w = 1; w < S; w *= 2)
#pragma unroll
      for (int z = 0; z < S; z += 2 * w) v[z] = w4_add(v[z], v[z + w]);
    const float wp_ = wts[p];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[0][r] = w4_scalar(wp_ * v[0][r]);
    sum = w4_add(sum, v[0]);
  }
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
