// MXFP4 weight-only GEMM for 33+ rows (W4A16; prefill and batched decode):
//   y[M,N] = x[M,K] · dequant(Wq[N,K/2], S[N,K/32])^T
// x bf16, y bf16, fp32 accumulation; the weight format is linear_w4.hip's
// (low nibble = even k, one e8m0 code per 32 k, codes 2..252). Any M >= 1,
// K % 128 == 0, N % 128 == 0, x and Wq 16-byte and S 4-byte aligned. Included
// after linear_w4.hip in the one translation unit, so w4_cvt, w4_scale and
// w4_scalar are that file's, not copies. The waves of a block split N and
// share x through LDS, as in linear_w8_gemm.hip; what differs is the step
// (one MX block a lane, 128 k), the row pitch in LDS and with it the
// swizzle, the ring depth per tile height, and the balance worked out below.
//
// Work split. A block is 4 waves and owns 128 output channels x BM rows
// (BM = 64 or 128) x one contiguous range of 128-k steps. Wave w owns
// channels 32w..32w+31 (W4G_NT = 2 tiles of 16) and ALL BM rows: BM/16 row
// tiles, NT*BM/16 accumulators of 4 registers (32 or 64).
//
// Weights: global -> VGPR, never through LDS, one 16-byte non-temporal load
// per lane, tile and step: lane (r = l&15, g = l>>4) takes bytes
// 64*step + 16g .. +15 of channel row r, which is one MX block. The load
// feeds four MFMAs (v_mfma_f32_16x16x32_bf16, weights as A): MFMA j takes
// dword j, so its fragment element (g, i) is k = 128*step + 32g + 8j + i and
// the B fragment is gathered under the same k; nothing crosses lanes.
// w4_cvt (v_cvt_scalef32_pk_bf16_fp4) is exact. The scale is byte g of the
// dword at byte 4*step of the channel's scale row: one 4-byte load per tile
// and step next to the 16-byte one.
//
// Activations: through LDS. A step's x tile is [BM rows][128 k] bf16, 256
// bytes per row, 16 or 32 KB, staged with global_load_lds, 16 bytes per lane:
// one wave instruction writes 1 KB lane-linear = 4 rows, each fetched as two
// full 128-byte lines. Wave w stages rows (BM/4)w .. (BM/4)(w+1)-1, BM/16
// instructions a step. All four waves read the whole tile as B fragments
// with ds_read_b128: lane (m, g) of MFMA j, row tile u reads the 16 bytes of
// row 16u + m at logical byte 64g + 16j, i.e. 16-byte chunk c = 4g + j.
//
// Swizzle. Rows are 256 bytes apart, exactly one bank row (64 banks x 4 B),
// so unswizzled the 16 lanes m = 0..15 of one (g, j) would read the same
// 16-byte slot sixteen times. The fp8 kernel's (row >> 1) & 7 is for a
// 128-byte pitch and does not carry over. Here chunk c of row r is stored at
// chunk c ^ (r & 15): for m = 0..15 at a fixed c these are the 16 different
// slots of a bank row. Computed conflict degree, for a 128-bit read served
// 16 consecutive lanes (256 bytes) per pass: 1, conflict-free. The swizzle
// is applied to the per-lane SOURCE address while staging (lane l of an
// instruction writes row l>>4, stored chunk l&15, and fetches logical chunk
// (l&15) ^ (row&15)); the DMA's LDS side is linear, so fills are
// conflict-free too. Both degrees are computed, not read from counters.
// Since 16u & 15 == 0 a lane's read address is base + 4096u + stage, and
// c = 4g + j = 4g ^ j: one address register, the four j differ by XOR 16j.
// The stage base goes into the register (one add per j and step), because
// 2 stages of 32 KB plus 4096*7 does not fit ds_read's 16-bit offset.
//
// Balance, per block and 128-k step (16 clocks per MFMA, 128 B/clk of LDS,
// 8 TB/s / 256 CUs / 2.4 GHz = 13 B/clk of HBM per CU; counts, not
// measurements):
//                                              BM = 64   BM = 128
//   MFMA clocks per wave (NT*4*BM/16 MFMAs)       512      1024
//   LDS clocks (4 waves * BM/16 * 4 reads * 1 KB) 512      1024
//   HBM clocks (8 KB nibbles + 0.5 KB scales)    ~650      ~650
// With fp8 weights the weight stream was on top at both heights; here it is
// on top only at BM = 64, and at BM = 128 the matrix cores and LDS are level
// over it. LDS bytes per MFMA: a fragment read is 1 KB per wave and feeds NT
// MFMAs, 1024/NT = 512 bytes. NT = 4 would halve that, but a wave then owns
// 64 channels: either the block is 256 channels (N % 256, and N = 4096 is
// down to 16 blocks per row tile, so more split of K and more fp32 partial
// traffic) or it is two waves (64 + 64 accumulator registers a wave at
// BM = 128, and with the 96 KB ring below one block per CU that is two of
// four SIMDs idle). LDS reads and MFMAs are issued by different units and
// overlap (the reads of row tile u+1 go out before the MFMAs of tile u), so
// level is not the sum. NT = 2 at both heights; accumulators 32 / 64.
//
// Stage size and ring depth. Stages are 128 k deep, one per weight slot, so
// the vmcnt arithmetic has one kind of step. BM = 64: W4G ring of 4 stages,
// 64 KB, two blocks per CU (160 KB of LDS), step r computes while the loads
// of steps r+1..r+3 are in flight: 384 k = 3 x (8.5 KB weights + 16 KB x) per
// block. BM = 128: a 4-stage ring would be 128 KB; the ring is 3 stages,
// 96 KB, one block per CU, 256 k = 2 x (8.5 KB + 32 KB) in flight. At 13
// B/clk and ~2000 clocks of latency a CU needs ~26 KB of weights in flight to
// run at the HBM rate; BM = 64 has 2 x 25.5 KB, and BM = 128, which needs
// only 8.5 KB per 1024 MFMA clocks = 8.3 B/clk, has 17 KB against ~17 KB.
//
// Pipeline. One barrier per step, PF = RING - 1 steps ahead:
//   s_waitcnt vmcnt((PF-1)*LD)   this wave's part of x(r), w(r), s(r) landed
//   s_barrier                    everyone's part landed; everyone is done
//                                reading stage (r-1) % RING
//   issue x(r+PF) -> stage (r+PF) % RING, w and s(r+PF) -> slot (r+PF) % RING
//   convert slot r % RING; B fragment reads one row tile ahead of the MFMAs
// RAW: a step issues LD = BM/16 staging loads + NT weight loads + NT scale
// loads (8 or 12) and loads return in order, so (PF-1)*LD outstanding (16 at
// BM = 64, 12 at BM = 128; the counter holds 63) means everything up to step
// r's own loads has landed. WAR: stage (r+PF) % RING was last read in step
// r-1, whose last fragment read is waited for (lgkmcnt(0)) before the
// barrier of step r. The count only holds if every step issues the same
// number of loads, so inside the main loop (whole groups of RING steps, ring
// slots as compile-time constants) the steps whose step r+PF is past the
// range issue them too, all lanes at the first 16 bytes of x and of Wq and
// the first 4 of S (inside the operands) into a stage and a slot nobody
// reads again: no predicated loads, no branch around a load. The last
// n % RING steps issue nothing and wait for vmcnt(0). The weight loads, the
// scale loads, the fragment reads and their waits are inline asm, for the
// reasons linear_w8_gemm.hip records (plain loads next to LDS DMA make the
// compiler drain everything with vmcnt(0)); a step's vmcnt wait names the
// slot's registers as operands, so nothing that reads them moves above it.
//
// Padding: a row >= M of the last row tile reads row 0 again and lands in
// accumulators that are never stored; nothing outside the M rows of x and
// the N rows of Wq and S is read, nothing outside y and the workspace is
// written. N % 128 == 0 means there are no partial channel tiles.
//
// Split of K across blocks. The grid is (N/128) x ceil(M/BM) x S and slice z
// takes steps floor(steps*z/S) .. floor(steps*(z+1)/S) - 1. S == 1: the
// epilogue (one rounding to bf16, 8-byte stores of a lane's four consecutive
// channels) is in this kernel and there is no workspace. S > 1: the slices
// store fp32 partials to a workspace [S][M][N] and linear_w4_gemm_combine
// sums them in order z = 0..S-1 and rounds once. No atomics: the result
// depends on S, and S depends only on (M, N, K) and the CU count
// (csrc/ops.hip), so calls are bit-identical. It does not depend on BM: an
// element's products enter its accumulator in the order (step, j) under
// either tile. A slice without steps stores zeros.
//
// Not bit-identical with the skinny kernel: linear_w4.hip's fixed 8-group
// tree needs three pending copies of the accumulator, and three copies of
// 32 or 64 registers next to the ring do not fit.

#define W4G_NT 2

template <int BM>
struct W4gLane {
  const char* xp[BM / 16];          // staging sources at k = 0
  const unsigned char* wp[W4G_NT];  // weight rows at k = 0
  const unsigned char* sp[W4G_NT];  // scale rows at k = 0
  const char* x0;                   // the loads of steps past the range
  const unsigned char* w0;
  const unsigned char* s0;
  char* lds_w;                      // this wave's rows of stage 0
  unsigned rd;                      // fragment read address, j = 0
};

template <int BM, int RING>
struct W4gRegs {
  float4v acc[W4G_NT][BM / 16];
  u32x4 w[RING][W4G_NT];
  unsigned int sc[RING][W4G_NT];
};

template <int OFF>
DEV_INLINE u32x4 w4g_read(unsigned addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2"
               : "=v"(v)
               : "v"(addr), "n"(OFF)
               : "memory");
  return v;
}

// the loads of absolute step `step` into ring slot Q (live: inside the range)
template <int BM, int RING, int Q>
DEV_INLINE void w4g_issue(const W4gLane<BM>& L, W4gRegs<BM, RING>& R, int step,
                          bool live) {
  typedef const __attribute__((address_space(1))) void* gptr;
  typedef __attribute__((address_space(3))) void* lptr;
  const size_t s = (size_t)step;
#pragma unroll
  for (int i = 0; i < BM / 16; ++i) {
    const char* src = live ? L.xp[i] + 256 * s : L.x0;
    __builtin_amdgcn_global_load_lds(
        (gptr)src, (lptr)(L.lds_w + Q * (BM * 256) + 1024 * i), 16, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < W4G_NT; ++t) {
    const unsigned char* wsrc = live ? L.wp[t] + 64 * s : L.w0;
    const unsigned char* ssrc = live ? L.sp[t] + 4 * s : L.s0;
    asm volatile("global_load_dwordx4 %0, %1, off nt"
                 : "=v"(R.w[Q][t])
                 : "v"(wsrc)
                 : "memory");
    asm volatile("global_load_dword %0, %1, off"
                 : "=v"(R.sc[Q][t])
                 : "v"(ssrc)
                 : "memory");
  }
}

// row tile U of the stage at `rd`: the reads of tile U+1 go out first
template <int BM, int RING, int U>
DEV_INLINE void w4g_rows(W4gRegs<BM, RING>& R, const unsigned (&rd)[4],
                         const bf16x8 (&a)[W4G_NT][4], u32x4 (&b)[2][4]) {
  constexpr int MT = BM / 16;
  if constexpr (U + 1 < MT) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      b[(U + 1) & 1][j] = w4g_read<4096 * (U + 1)>(rd[j]);
    asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
  } else {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = 0; t < W4G_NT; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      R.acc[t][U] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a[t][j], __builtin_bit_cast(bf16x8, b[U & 1][j]), R.acc[t][U], 0, 0,
          0);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (U + 1 < MT) w4g_rows<BM, RING, U + 1>(R, rd, a, b);
}

// Relative step r of a range of n steps that begins at absolute step beg.
// LOAD = false is a step of the tail (see the kernel): nothing to issue.
template <int BM, int RING, int Q, bool LOAD>
DEV_INLINE void w4g_step(const W4gLane<BM>& L, W4gRegs<BM, RING>& R, int beg,
                         int r, int n, int g) {
  constexpr int PF = RING - 1;
  constexpr int LD = BM / 16 + 2 * W4G_NT;  // loads a wave issues per step
  constexpr int CNT = LOAD ? (PF - 1) * LD : 0;
  static_assert(CNT <= 63, "vmcnt is a 6-bit counter");
  static_assert(W4G_NT == 2, "the wait names two tiles");
  // the slot's registers pass through the wait: nothing that reads them
  // can be placed before it
  asm volatile("s_waitcnt vmcnt(%4)"
               : "+v"(R.w[Q][0]), "+v"(R.w[Q][1]), "+v"(R.sc[Q][0]),
                 "+v"(R.sc[Q][1])
               : "n"(CNT)
               : "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  if (LOAD)
    w4g_issue<BM, RING, (Q + PF) % RING>(L, R, beg + r + PF, r + PF < n);
  __builtin_amdgcn_sched_barrier(0);
  unsigned rd[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) rd[j] = (L.rd ^ (16 * j)) + Q * (BM * 256);
  u32x4 b[2][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) b[0][j] = w4g_read<0>(rd[j]);
  bf16x8 a[W4G_NT][4];
#pragma unroll
  for (int t = 0; t < W4G_NT; ++t) {
    const float scale = w4_scale((R.sc[Q][t] >> (8 * g)) & 0xffu);
#pragma unroll
    for (int j = 0; j < 4; ++j) a[t][j] = w4_cvt(R.w[Q][t][j], scale);
  }
  w4g_rows<BM, RING, 0>(R, rd, a, b);
}

template <int BM, int RING, int Q>
DEV_INLINE void w4g_prologue(const W4gLane<BM>& L, W4gRegs<BM, RING>& R,
                             int beg, int n) {
  if constexpr (Q < RING - 1) {
    w4g_issue<BM, RING, Q>(L, R, beg + Q, Q < n);
    w4g_prologue<BM, RING, Q + 1>(L, R, beg, n);
  }
}

// RING steps from relative step r, no branch inside (a branch lets the
// compiler sink a weight load towards its use)
template <int BM, int RING, int Q>
DEV_INLINE void w4g_group(const W4gLane<BM>& L, W4gRegs<BM, RING>& R, int beg,
                          int r, int n, int g) {
  if constexpr (Q < RING) {
    w4g_step<BM, RING, Q, true>(L, R, beg, r + Q, n, g);
    w4g_group<BM, RING, Q + 1>(L, R, beg, r, n, g);
  }
}

// the last n % RING steps. Every load that matters has been issued, so these
// wait for all of them, which also retires the loads of the steps past the
// range that still target LDS.
template <int BM, int RING, int Q>
DEV_INLINE void w4g_tail(const W4gLane<BM>& L, W4gRegs<BM, RING>& R, int beg,
                         int r, int n, int g) {
  if constexpr (Q < RING - 1) {
    if (r + Q < n) w4g_step<BM, RING, Q, false>(L, R, beg, r + Q, n, g);
    w4g_tail<BM, RING, Q + 1>(L, R, beg, r, n, g);
  }
}

template <int BM, int RING, bool SPLIT>
__global__ __launch_bounds__(256, BM == 64 ? 2 : 1) void linear_w4_gemm_kernel(
    const short* __restrict__ X, const unsigned char* __restrict__ Wq,
    const unsigned char* __restrict__ Sc, short* __restrict__ Y,
    float* __restrict__ ws, int M, int N, int K) {
  __shared__ __attribute__((aligned(1024))) char smem[RING * BM * 256];
  constexpr int MT = BM / 16;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int r16 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 128 + 32 * w;
  const int m0 = blockIdx.y * BM;
  const int steps = K / 128;
  const int beg = (int)((long long)steps * blockIdx.z / gridDim.z);
  const int end = (int)((long long)steps * (blockIdx.z + 1) / gridDim.z);
  const int n = end - beg;

  W4gLane<BM> L;
  L.x0 = reinterpret_cast<const char*>(X);
  L.w0 = Wq;
  L.s0 = Sc;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    // LDS byte 16*lane of this instruction's 1 KB: row lane>>4, stored chunk
    // lane&15, which holds logical chunk (lane&15) ^ (row&15)
    const int row = (BM / 4) * w + 4 * i + (lane >> 4);
    const int ch = (lane & 15) ^ (row & 15);
    const int m = m0 + row;
    L.xp[i] = L.x0 + ((size_t)(m < M ? m : 0) * K) * 2 + 16 * ch;
  }
#pragma unroll
  for (int t = 0; t < W4G_NT; ++t) {
    const size_t ch = (size_t)(n0 + 16 * t + r16);
    L.wp[t] = Wq + ch * (K / 2) + 16 * g;
    L.sp[t] = Sc + ch * (K / 32);
  }
  L.lds_w = smem + (BM / 4) * 256 * w;
  const unsigned sm0 =
      (unsigned)(size_t)((__attribute__((address_space(3))) char*)smem);
  L.rd = sm0 + 256 * r16 + 16 * ((4 * g) ^ r16);

  W4gRegs<BM, RING> R;
#pragma unroll
  for (int t = 0; t < W4G_NT; ++t)
#pragma unroll
    for (int u = 0; u < MT; ++u) R.acc[t][u] = float4v{0.f, 0.f, 0.f, 0.f};

  if (n > 0) {  // uniform over the block
    w4g_prologue<BM, RING, 0>(L, R, beg, n);
    int r = 0;
    for (; r + RING <= n; r += RING) w4g_group<BM, RING, 0>(L, R, beg, r, n, g);
    w4g_tail<BM, RING, 0>(L, R, beg, r, n, g);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }

#pragma unroll
  for (int t = 0; t < W4G_NT; ++t) {
    const int nn = n0 + 16 * t + 4 * g;
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
        for (int r = 0; r < 4; ++r) o[r] = f2bf(R.acc[t][u][r]);
        *reinterpret_cast<short4v*>(Y + (size_t)m * N + nn) = o;
      }
    }
  }
}

// y = bf16(sum_z ws[z][m][n]), z in order; four channels a thread
__global__ __launch_bounds__(256) void linear_w4_gemm_combine(
    const float* __restrict__ ws, short* __restrict__ Y, long long MN, int S) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= MN) return;
  float4v s = *reinterpret_cast<const float4v*>(ws + i);
  for (int z = 1; z < S; ++z) {
    const float4v p = *reinterpret_cast<const float4v*>(ws + z * MN + i);
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = w4_scalar(s[r] + p[r]);
  }
  short4v o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = f2bf(s[r]);
  *reinterpret_cast<short4v*>(Y + i) = o;
}
