// FP8 weight-only GEMM for 33+ rows (W8A16; prefill and batched decode):
//   y[M,N] = x[M,K] · (Wq[N,K] ⊙ scale[N])^T
// x bf16, Wq OCP e4m3fn in nn.Linear's [out, in] layout, scale fp32 per
// output channel, y bf16; K % 128 == 0, N % 128 == 0, any M >= 1, x and Wq
// 16-byte aligned. It is linear_w8.hip's data path turned round: there the
// waves of a block split K and share nothing, here they split N and share
// x. Included after linear_w8.hip in the one translation unit, so w8_cvt and
// w8_scalar are that file's, not copies.
//
// Work split. A block is 4 waves and owns 128 output channels x BM rows
// (BM = 64 or 128) x one contiguous range of 64-k steps. Wave w owns
// channels 32w..32w+31 (W8G_NT = 2 tiles of 16) and ALL BM rows: BM/16 row
// tiles, NT*BM/16 accumulators of 4 registers (32 or 64).
//
// Weights: global -> VGPR, never through LDS, one 16-byte non-temporal load
// per lane, tile and step, exactly the skinny kernel's fragment: lane
// (r = l&15, g = l>>4) takes bytes 64*step + 16g .. +15 of channel row r,
// w8_cvt turns them into the A fragments of the step's two MFMAs
// (v_mfma_f32_16x16x32_bf16, weights as A), so MFMA j covers
// k = 64*step + 16g + 8j + i and the B fragment is gathered with the same k.
// Every weight byte is loaded once per row tile of BM rows.
//
// Activations: through LDS, which is the point. A step's x tile is
// [BM rows][64 k] bf16, 128 bytes per row, 8 or 16 KB. It is staged with
// global_load_lds, 16 bytes per lane (gemm_wgrad.hip's wg_stage_half is the
// precedent): one wave instruction writes 1 KB lane-linear = 8 rows, and
// each row is fetched as one full 128-byte line (8 lanes x 16 B). Wave w
// stages rows (BM/4)w .. (BM/4)(w+1)-1, BM/32 instructions a step. All four
// waves then read the whole tile as B fragments with ds_read_b128: lane
// (m, g) of MFMA j, row tile u reads the 16 bytes of row 16u + m at logical
// byte 32g + 16j, i.e. 16-byte chunk c = 2g + j of the row.
//
// Swizzle. Rows are 128 bytes apart and a bank row is 256 bytes (64 banks x
// 4 B), so unswizzled the 16 lanes m = 0..15 of one (g, j) would hit two
// 16-byte slots eight times over. Chunk c of row r is stored at chunk
// c ^ ((r >> 1) & 7). The 16-byte slot inside the bank row is then
// 8*(r&1) + (c ^ ((r>>1)&7)): for r = 0..15 at a fixed c these are 16
// different slots. Computed conflict degree, for a 128-bit read served 16
// consecutive lanes (256 bytes) per pass: 1, conflict-free. (Computed, not
// read from counters.) The swizzle is applied to the per-lane SOURCE
// address while staging, as gemm_wgrad.hip does; the DMA's LDS side is
// linear, so fills are conflict-free too. Since 16u >> 1 is a multiple of 8,
// a lane's read address is base + 2048u + stage offset: two address
// registers (j = 0, 1; they differ by XOR 16) and immediates.
//
// LDS bytes per MFMA. A fragment read is 1 KB per wave and feeds NT MFMAs:
// 1024/NT = 512 bytes per MFMA. Per step and block at BM = 128 that is
// 4 waves x 16 reads x 1 KB = 64 KB = 512 clocks of a 128 B/clk LDS, against
// 32 MFMAs per wave (each SIMD has its own) of 16 clocks = 512 clocks, and
// 8 KB of weights that take about 630 clocks at a CU's share of HBM
// (8 TB/s / 256 CUs / 2.4 GHz = 13 B/clk). NT = 2 therefore puts LDS level
// with the matrix cores and under the weight stream; NT = 1 would halve
// the weight bytes per step but not the LDS bytes (LDS 512 against HBM 315
// clocks: LDS on the critical path), NT = 4 needs 128 accumulator registers
// at BM = 128 and leaves N = 4096 with 16 blocks per row tile. These are
// counts, not measurements. x traffic from L2 per weight byte is 2*BM/128.
//
// Pipeline. A ring of W8G_RING = 4 stages of x in LDS (32 or 64 KB, two
// blocks per CU) and four register slots of weights; step r computes from
// slot r % 4 while the loads of steps r+1, r+2, r+3 are in flight
// (3 x (8 KB weights + 16 KB x) per block). One barrier per step:
//   s_waitcnt vmcnt(2*(XI+NT))   this wave's part of x(r), and w(r), landed
//   s_barrier                    everyone's part landed; everyone is done
//                                reading stage (r-1) % 4
//   issue x(r+3) -> stage (r+3) % 4, w(r+3) -> slot (r+3) % 4
//   B fragment reads of stage r % 4 one row tile ahead of the MFMAs
// RAW: a step issues XI staging loads and NT weight loads and loads return
// in order, so 2*(XI+NT) outstanding means everything up to step r's own
// loads has landed, whatever the order inside a step. WAR: stage (r+3) % 4
// was last read in step r-1, whose last fragment read is waited for
// (lgkmcnt(0)) before the barrier of step r. The count only holds if every
// step issues the same number of loads, so inside the main loop (whole
// groups of four steps, ring slots as compile-time constants) the steps
// whose step r+3 is past the range issue them too, all lanes at the first
// 16 bytes of x and of Wq (one cache line, inside the operands) into a
// stage and a slot nobody reads again: no predicated loads, no branch
// around a load. The last n % 4 steps issue nothing and wait for vmcnt(0).
// Everything that counts is inline asm. The fragment reads, because the
// compiler would wait for every outstanding LDS DMA before an LDS read it
// can see. The weight loads, because the compiler's wait insertion treats
// LDS DMA and register loads as two event kinds that may return out of
// order and answers every wait on a register load with vmcnt(0) while a
// DMA is pending: with plain loads the ring drained once per group. The
// waits are explicit: the fragment waits are pinned with sched_barrier as
// in gemm_wgrad.hip, and a step's vmcnt wait names the slot's registers as
// operands, so nothing that reads them can move above it.
//
// Padding: the skinny kernel's rule. A row >= M of the last row tile reads
// row 0 again and lands in accumulators that are never stored; nothing
// outside the M rows of x and the N rows of Wq is read. N % 128 == 0 means
// there are no partial channel tiles.
//
// Split of K across blocks. N = 4096 with one row tile is 32 blocks on 256
// CUs, so the grid is (N/128) x ceil(M/BM) x S and slice z takes steps
// floor(steps*z/S) .. floor(steps*(z+1)/S) - 1. S == 1: the epilogue
// (fp32 sum * scale[n], one rounding to bf16, 8-byte stores of a lane's
// four consecutive channels) is in this kernel and there is no workspace.
// S > 1: the slices store fp32 partials to a workspace [S][M][N] and
// linear_w8_gemm_combine sums them in order z = 0..S-1, multiplies by
// scale[n], rounds once and stores bf16 (the paged decode kernel's split-KV
// combine is the precedent). No atomics: the result depends on S, and S
// depends only on (M, N, K) and the CU count (csrc/ops.hip), so calls are
// bit-identical. A slice without steps stores zeros.

#define W8G_NT 2
#define W8G_RING 4
#define W8G_PF 3  // steps in flight ahead of the one computed

template <int BM>
struct W8gLane {
  const char* xp[BM / 32];           // staging sources at k = 0
  const unsigned char* wp[W8G_NT];   // weight rows at k = 0
  const char* x0;                    // the loads of steps past the range
  const unsigned char* w0;
  char* lds_w;                       // this wave's rows of stage 0
  unsigned rd[2];                    // fragment read address, j = 0 / 1
};

template <int BM>
struct W8gRegs {
  float4v acc[W8G_NT][BM / 16];
  u32x4 w[W8G_RING][W8G_NT];
};

template <int OFF>
DEV_INLINE u32x4 w8g_read(unsigned addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2"
               : "=v"(v)
               : "v"(addr), "n"(OFF)
               : "memory");
  return v;
}

// the loads of absolute step `step` into ring slot Q (live: inside the range)
template <int BM, int Q>
DEV_INLINE void w8g_issue(const W8gLane<BM>& L, W8gRegs<BM>& R, int step,
                          bool live) {
  typedef const __attribute__((address_space(1))) void* gptr;
  typedef __attribute__((address_space(3))) void* lptr;
  const size_t kb = (size_t)step * 64;
#pragma unroll
  for (int i = 0; i < BM / 32; ++i) {
    const char* src = live ? L.xp[i] + 2 * kb : L.x0;
    __builtin_amdgcn_global_load_lds(
        (gptr)src, (lptr)(L.lds_w + Q * (BM * 128) + 1024 * i), 16, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < W8G_NT; ++t) {
    const unsigned char* src = live ? L.wp[t] + kb : L.w0;
    asm volatile("global_load_dwordx4 %0, %1, off nt"
                 : "=v"(R.w[Q][t])
                 : "v"(src)
                 : "memory");
  }
}

// row tile U of ring slot Q: the reads of tile U+1 go out first
template <int BM, int Q, int U>
DEV_INLINE void w8g_rows(const W8gLane<BM>& L, W8gRegs<BM>& R,
                         const bf16x8 (&a)[W8G_NT][2], u32x4 (&b)[2][2]) {
  constexpr int MT = BM / 16;
  if constexpr (U + 1 < MT) {
    constexpr int OFF = Q * (BM * 128) + 2048 * (U + 1);
    b[(U + 1) & 1][0] = w8g_read<OFF>(L.rd[0]);
    b[(U + 1) & 1][1] = w8g_read<OFF>(L.rd[1]);
    asm volatile("s_waitcnt lgkmcnt(2)" ::: "memory");
  } else {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = 0; t < W8G_NT; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      R.acc[t][U] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a[t][j], __builtin_bit_cast(bf16x8, b[U & 1][j]), R.acc[t][U], 0, 0,
          0);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (U + 1 < MT) w8g_rows<BM, Q, U + 1>(L, R, a, b);
}

// Relative step r of a range of n steps that begins at absolute step beg.
// LOAD = false is a step of the tail (see the kernel): nothing to issue.
template <int BM, int Q, bool LOAD>
DEV_INLINE void w8g_step(const W8gLane<BM>& L, W8gRegs<BM>& R, int beg, int r,
                         int n) {
  constexpr int XI = BM / 32;
  static_assert(2 * (XI + W8G_NT) == 8 || 2 * (XI + W8G_NT) == 12, "vmcnt");
  // the slot's registers pass through the wait: nothing that reads them
  // can be placed before it
#define W8G_WAIT(CNT)                                \
  asm volatile("s_waitcnt vmcnt(" #CNT ")"           \
               : "+v"(R.w[Q][0]), "+v"(R.w[Q][1])    \
               :                                     \
               : "memory")
  static_assert(W8G_NT == 2, "W8G_WAIT names two tiles");
  if (!LOAD) W8G_WAIT(0);
  if (LOAD && XI == 2) W8G_WAIT(8);
  if (LOAD && XI == 4) W8G_WAIT(12);
#undef W8G_WAIT
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  if (LOAD)
    w8g_issue<BM, (Q + W8G_PF) % W8G_RING>(L, R, beg + r + W8G_PF,
                                           r + W8G_PF < n);
  __builtin_amdgcn_sched_barrier(0);
  bf16x8 a[W8G_NT][2];
#pragma unroll
  for (int t = 0; t < W8G_NT; ++t) w8_cvt(R.w[Q][t], a[t][0], a[t][1]);
  u32x4 b[2][2];
  b[0][0] = w8g_read<Q * (BM * 128)>(L.rd[0]);
  b[0][1] = w8g_read<Q * (BM * 128)>(L.rd[1]);
  w8g_rows<BM, Q, 0>(L, R, a, b);
}

template <int BM, bool SPLIT>
__global__ __launch_bounds__(256, 2) void linear_w8_gemm_kernel(
    const short* __restrict__ X, const unsigned char* __restrict__ Wq,
    const float* __restrict__ scale, short* __restrict__ Y,
    float* __restrict__ ws, int M, int N, int K) {
  __shared__ __attribute__((aligned(1024))) char smem[W8G_RING * BM * 128];
  constexpr int MT = BM / 16, XI = BM / 32;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int r16 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 128 + 32 * w;
  const int m0 = blockIdx.y * BM;
  const int steps = K / 64;
  const int beg = (int)((long long)steps * blockIdx.z / gridDim.z);
  const int end = (int)((long long)steps * (blockIdx.z + 1) / gridDim.z);
  const int n = end - beg;

  W8gLane<BM> L;
  L.x0 = reinterpret_cast<const char*>(X);
  L.w0 = Wq;
#pragma unroll
  for (int i = 0; i < XI; ++i) {
    // LDS byte 16*lane of this instruction's 1 KB: row lane>>3, stored chunk
    // lane&7, which holds logical chunk (lane&7) ^ ((row>>1)&7)
    const int row = (BM / 4) * w + 8 * i + (lane >> 3);
    const int ch = (lane & 7) ^ ((row >> 1) & 7);
    const int m = m0 + row;
    L.xp[i] = L.x0 + ((size_t)(m < M ? m : 0) * K) * 2 + 16 * ch;
  }
#pragma unroll
  for (int t = 0; t < W8G_NT; ++t)
    L.wp[t] = Wq + (size_t)(n0 + 16 * t + r16) * K + 16 * g;
  L.lds_w = smem + (BM / 4) * 128 * w;
  const unsigned sm0 =
      (unsigned)(size_t)((__attribute__((address_space(3))) char*)smem);
  L.rd[0] = sm0 + 128 * r16 + 16 * ((2 * g) ^ (r16 >> 1));
  L.rd[1] = L.rd[0] ^ 16;

  W8gRegs<BM> R;
#pragma unroll
  for (int t = 0; t < W8G_NT; ++t)
#pragma unroll
    for (int u = 0; u < MT; ++u) R.acc[t][u] = float4v{0.f, 0.f, 0.f, 0.f};

  if (n > 0) {  // uniform over the block
    w8g_issue<BM, 0>(L, R, beg, true);
    w8g_issue<BM, 1>(L, R, beg + 1, 1 < n);
    w8g_issue<BM, 2>(L, R, beg + 2, 2 < n);
    // whole groups of four steps, no branch inside a group (a branch lets
    // the compiler sink a weight load towards its use)
    int r = 0;
    for (; r + 4 <= n; r += 4) {
      w8g_step<BM, 0, true>(L, R, beg, r, n);
      w8g_step<BM, 1, true>(L, R, beg, r + 1, n);
      w8g_step<BM, 2, true>(L, R, beg, r + 2, n);
      w8g_step<BM, 3, true>(L, R, beg, r + 3, n);
    }
    // tail: the last n % 4 steps. Every load that matters has been issued,
    // so these wait for all of them, which also retires the loads of the
    // steps past the range that still target LDS.
    if (r < n) w8g_step<BM, 0, false>(L, R, beg, r, n);
    if (r + 1 < n) w8g_step<BM, 1, false>(L, R, beg, r + 1, n);
    if (r + 2 < n) w8g_step<BM, 2, false>(L, R, beg, r + 2, n);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }

#pragma unroll
  for (int t = 0; t < W8G_NT; ++t) {
    const int nn = n0 + 16 * t + 4 * g;
    float sc[4];
    if (!SPLIT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sc[r] = scale[nn + r];
    }
#pragma unroll
    for (int u = 0; u < MT; ++u) {
      const int m = m0 + 16 * u + r16;
      if (m >= M) continue;
      if (SPLIT) {
        *reinterpret_cast<float4v*>(
            ws + ((size_t)blockIdx.z * M + m) * N + nn) = R.acc[t][u];
      } else {
        short4v o;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          o[r] = f2bf(w8_scalar(R.acc[t][u][r] * sc[r]));
        *reinterpret_cast<short4v*>(Y + (size_t)m * N + nn) = o;
      }
    }
  }
}

// y = bf16(scale[n] * sum_z ws[z][m][n]), z in order; four channels a thread
__global__ __launch_bounds__(256) void linear_w8_gemm_combine(
    const float* __restrict__ ws, const float* __restrict__ scale,
    short* __restrict__ Y, long long MN, int N, int S) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= MN) return;
  const int nn = (int)(i % N);
  float4v s = *reinterpret_cast<const float4v*>(ws + i);
  for (int z = 1; z < S; ++z) {
    const float4v p = *reinterpret_cast<const float4v*>(ws + z * MN + i);
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = w8_scalar(s[r] + p[r]);
  }
  short4v o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = f2bf(w8_scalar(s[r] * scale[nn + r]));
  *reinterpret_cast<short4v*>(Y + i) = o;
}
