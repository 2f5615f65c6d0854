// gemm_wgrad: dW[N,K] = dy^T · x for bf16 row-major dy [M,N] and x [M,K]
// (fp32 accumulate, one rounding to bf16 on store).
//
// The reduction index m is the ROW of both operands, so both MFMA fragments
// are column reads of a row-major slab. They come from LDS through the
// hardware transpose read ds_read_b64_tr_b16; global memory is only ever
// read in whole rows.
//
// Tile: 256 (n) x 256 (k) per block, 64 tokens per K-step, 8 waves as
// 2 (n) x 4 (k), mfma_f32_32x32x16_bf16. Each operand slab [64 tok][256 col]
// is two "halves" of 128 columns; wave (wr, wc) owns rows 64wr..64wr+63 of
// each dy half and columns 32wc..32wc+31 of each x half, i.e. four 64x32
// output quadrants (ha, hb), 128 accumulator registers.
//
// LDS image. Every half is the [64][128] image of fa_bwd_lds_layout.h
// (8-row x 32-column subtiles of 512 B, 16-byte chunks XORed with
// (row>>2)&3 inside a 64-byte subtile row). It is filled by
// global_load_lds, 16 bytes per lane: one wave instruction writes 1 KB
// lane-linear = two subtiles = 8 tokens x 64 columns, and the swizzle is
// applied to the per-lane SOURCE address. Each token row is fetched as one
// full 128-byte line per instruction (8 lanes x 16 B). A transposed read's
// 32-lane half takes rows 4h..4h+3 of one subtile: 4 x 64 B contiguous =
// one 256-byte bank row, every dword distinct, so the computed conflict
// degree is 1 (conflict-free); fills are linear.
//
// Fragments: k-step s of a half takes its two 4-token blocks from 8-row
// groups 2s and 2s+1 (fb6_tbase), so element j of lane half h is token
// 16s + 8(j>>2) + 4h + (j&3) for A and for B alike.
//
// Pipeline. Two 64 KB stages; a tile is four phases, one quadrant each:
//   ph1 (A0,B0): read A0,B0   stage B0 of tile t+1 (other stage)
//   ph2 (A0,B1): read B1      stage A0 of tile t+2 (this stage)
//   ph3 (A1,B1): read A1      stage B1 of tile t+2
//   ph4 (A1,B0): read B0      stage A1 of tile t+2, s_waitcnt vmcnt(6)
// and every phase is {ds reads, 2 x global_load_lds, lgkmcnt(0), s_barrier,
// 8 MFMA, s_barrier}. The wr = 1 waves run one barrier behind the wr = 0
// waves (waves w and w+4 share a SIMD), so one group's reads overlap the
// other group's MFMAs. This follows the guide's 256^2 schedule (counted
// vmcnt once per tile = 2 loads x 3 half-tiles left in flight, raw
// s_barrier, one __shared__ array, staggered wave groups) but the phase
// contents were written from its description, so it counts as a new
// template: the test suite's repeatability screen applies to it.
//   RAW: vmcnt(6) before ph4's first barrier retires every half of tile
//   t+1; with the stagger the later group's wait is ordered by the earlier
//   group's SECOND ph4 barrier, and the first read is in ph1 of tile t+1.
//   WAR: a half is restaged one phase after the phase that read it, and
//   that phase's lgkmcnt(0) sits before its FIRST barrier, so the later
//   group's reads have retired when the earlier group passes its second.
// EXEC is full throughout: no lane-dependent branch anywhere in the loop.
//
// Accepted: N % 256 == 0, K % 256 == 0, M % 128 == 0 (two tiles: the loop is
// unrolled over the two stages), M >= 128; row strides multiples of 8
// elements, 16-byte-aligned bases. Checked by the launcher in ops.hip.
//
// Grouped launch: problems share x; tile rows >= nt0 belong to problem 1
// (its own dy and output pointer). A single problem passes nt0 = all rows.
#include "common.h"
#include "fa_bwd_lds_layout.h"

typedef __attribute__((ext_vector_type(8))) __bf16 wg_bf16x8;
typedef __attribute__((ext_vector_type(16))) float wg_f32x16;
typedef __attribute__((ext_vector_type(2))) unsigned int wg_u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int wg_u32x4;

#define WG_STAGE 65536  // bytes: A0 A1 B0 B1, 16 KB each
#define WG_HALF 16384
#define WG_B 32768

template <int OFF>
DEV_INLINE wg_u32x2 wg_tr(unsigned addr) {
  wg_u32x2 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
               : "=v"(v)
               : "v"(addr), "n"(OFF)
               : "memory");
  return v;
}

DEV_INLINE wg_bf16x8 wg_frag(wg_u32x2 lo, wg_u32x2 hi) {
  wg_u32x4 t = __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
  return __builtin_bit_cast(wg_bf16x8, t);
}

// one half-tile: this wave's 8 tokens x 128 columns, two 1 KB instructions
DEV_INLINE void wg_stage_half(const char* g, unsigned lane_off, char* lds) {
  typedef const __attribute__((address_space(1))) void* gptr;
  typedef __attribute__((address_space(3))) void* lptr;
  __builtin_amdgcn_global_load_lds((gptr)(g + lane_off), (lptr)lds, 16, 0, 0);
  __builtin_amdgcn_global_load_lds((gptr)(g + 128 + lane_off),
                                   (lptr)(lds + 1024), 16, 0, 0);
}

struct WgRegs {
  wg_f32x16 acc[2][2][2];  // [ha][hb][32-row block]
  wg_u32x2 a[2][4][2];     // [32-row block][k-step][4-token block]
  wg_u32x2 b[4][2];
};

// k-step S of a dy half: both 32-row blocks, both 4-token blocks
template <int BASE, int S>
DEV_INLINE void wg_read_a1(WgRegs& r, unsigned a0, unsigned a1) {
  r.a[0][S][0] = wg_tr<BASE + 4096 * S>(a0);
  r.a[0][S][1] = wg_tr<BASE + 4096 * S + 2048>(a1);
  r.a[1][S][0] = wg_tr<BASE + 4096 * S + 512>(a0);
  r.a[1][S][1] = wg_tr<BASE + 4096 * S + 2048 + 512>(a1);
}
template <int BASE>
DEV_INLINE void wg_read_a(WgRegs& r, unsigned a0, unsigned a1) {
  wg_read_a1<BASE, 0>(r, a0, a1);
  wg_read_a1<BASE, 1>(r, a0, a1);
  wg_read_a1<BASE, 2>(r, a0, a1);
  wg_read_a1<BASE, 3>(r, a0, a1);
}

template <int BASE, int S>
DEV_INLINE void wg_read_b1(WgRegs& r, unsigned b0, unsigned b1) {
  r.b[S][0] = wg_tr<BASE + 4096 * S>(b0);
  r.b[S][1] = wg_tr<BASE + 4096 * S + 2048>(b1);
}
template <int BASE>
DEV_INLINE void wg_read_b(WgRegs& r, unsigned b0, unsigned b1) {
  wg_read_b1<BASE, 0>(r, b0, b1);
  wg_read_b1<BASE, 1>(r, b0, b1);
  wg_read_b1<BASE, 2>(r, b0, b1);
  wg_read_b1<BASE, 3>(r, b0, b1);
}

template <int HA, int HB>
DEV_INLINE void wg_mma(WgRegs& r) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const wg_bf16x8 bf = wg_frag(r.b[s][0], r.b[s][1]);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      r.acc[HA][HB][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          wg_frag(r.a[i][s][0], r.a[i][s][1]), bf, r.acc[HA][HB][i], 0, 0, 0);
  }
  __builtin_amdgcn_s_setprio(0);
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// One tile out of stage ST. gA/gB: this block's operand columns at token 0
// (uniform); tile t+1's B0 goes to the other stage, tile t+2's A0,B1,A1 to
// this one. VMC: the counted wait of phase 4 (-1: none).
template <int ST, bool NEXT_B0, bool NEXT2, int VMC>
DEV_INLINE void wg_tile(WgRegs& r, const unsigned (&ra)[2][2],
                        const unsigned (&rb)[2][2], char* lds_w, const char* gA,
                        const char* gB, unsigned la, unsigned lb,
                        long long tileA, long long tileB, int t) {
  constexpr int S = ST * WG_STAGE;
  constexpr int O = (ST ^ 1) * WG_STAGE;
  // ph1
  wg_read_a<0>(r, ra[ST][0], ra[ST][1]);
  wg_read_b<0>(r, rb[ST][0], rb[ST][1]);
  if (NEXT_B0)
    wg_stage_half(gB + (t + 1) * tileB, lb, lds_w + O + WG_B);
  wg_mma<0, 0>(r);
  // ph2
  wg_read_b<WG_HALF>(r, rb[ST][0], rb[ST][1]);
  if (NEXT2) wg_stage_half(gA + (t + 2) * tileA, la, lds_w + S);
  wg_mma<0, 1>(r);
  // ph3
  wg_read_a<WG_HALF>(r, ra[ST][0], ra[ST][1]);
  if (NEXT2)
    wg_stage_half(gB + (t + 2) * tileB + 256, lb, lds_w + S + WG_B + WG_HALF);
  wg_mma<1, 1>(r);
  // ph4
  wg_read_b<0>(r, rb[ST][0], rb[ST][1]);
  if (NEXT2)
    wg_stage_half(gA + (t + 2) * tileA + 256, la, lds_w + S + WG_HALF);
  if (VMC == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  if (VMC == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  wg_mma<1, 0>(r);
}

// STAGGER = false (RAY_AMD_WGRAD_NO_STAGGER=1) keeps all eight waves in
// step: the A/B arm that shows what the stagger is worth.
template <bool STAGGER>
__global__ __launch_bounds__(512) void gemm_wgrad_bf16(
    const short* __restrict__ dy0, const short* __restrict__ dy1,
    const short* __restrict__ x, short* __restrict__ out0,
    short* __restrict__ out1, int M, long long ldy, long long ldx,
    long long ldo, int NT, int nt0, int KT) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * WG_STAGE];

  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int wr = w >> 2, wc = w & 3;

  // bijective XCD remap, then 8 tile rows x KT tile columns per group so
  // that the blocks sharing an XCD's L2 share operand panels
  int tn, tk;
  {
    const int nwg = NT * KT;
    const int orig = blockIdx.x;
    const int xcd = orig & 7;
    const int q = nwg >> 3, rr = nwg & 7;
    const int id = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) +
                   (orig >> 3);
    const int per = 8 * KT;
    const int grp = id / per;
    const int first = grp * 8;
    const int gsz = min(NT - first, 8);
    const int in = id - grp * per;
    tn = first + in % gsz;
    tk = in / gsz;
  }
  const bool p1 = tn >= nt0;
  const short* dy = p1 ? dy1 : dy0;
  short* out = p1 ? out1 : out0;
  const int tn_l = p1 ? tn - nt0 : tn;

  const char* gA = reinterpret_cast<const char*>(dy + (long long)tn_l * 256);
  const char* gB = reinterpret_cast<const char*>(x + (long long)tk * 256);
  const long long tileA = 64 * ldy * 2, tileB = 64 * ldx * 2;  // bytes

  // staging: lane j of wave w writes LDS byte 16j of row group w
  unsigned la, lb;
  {
    const int r7 = (lane >> 2) & 7;
    const int xo = 2 * (w & 1) + (r7 >> 2);
    const int ch = 4 * (lane >> 5) + ((lane & 3) ^ xo);
    const int row = 8 * w + r7;
    la = (unsigned)(row * (int)ldy * 2 + 16 * ch);
    lb = (unsigned)(row * (int)ldx * 2 + 16 * ch);
  }
  char* const lds_w = smem + 2048 * w;

  // transposed-read bases (bytes): [stage][4-token block]
  const unsigned sm0 = (unsigned)(size_t)(
      (__attribute__((address_space(3))) char*)smem);
  unsigned ra[2][2], rb[2][2];
#pragma unroll
  for (int mm = 0; mm < 2; ++mm) {
    const unsigned tb = sm0 + 2 * fb6_tbase(lane, mm);
    ra[0][mm] = tb + 1024 * wr;
    ra[1][mm] = tb + 1024 * wr + WG_STAGE;
    rb[0][mm] = tb + 512 * wc + WG_B;
    rb[1][mm] = tb + 512 * wc + WG_B + WG_STAGE;
  }

  WgRegs r;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 2; ++i) r.acc[a][b][i] = wg_f32x16{};

  const int nt = M >> 6;  // even, >= 2

  // prologue: tile 0 whole, tile 1 without B0 (phase 1 of tile 0 stages it)
  wg_stage_half(gA, la, lds_w);
  wg_stage_half(gB, lb, lds_w + WG_B);
  wg_stage_half(gB + 256, lb, lds_w + WG_B + WG_HALF);
  wg_stage_half(gA + 256, la, lds_w + WG_HALF);
  wg_stage_half(gA + tileA, la, lds_w + WG_STAGE);
  wg_stage_half(gB + tileB + 256, lb, lds_w + WG_STAGE + WG_B + WG_HALF);
  wg_stage_half(gA + tileA + 256, la, lds_w + WG_STAGE + WG_HALF);
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  // stagger: the wr = 1 waves run one barrier behind the wr = 0 waves
  if (STAGGER && wr) __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  int t = 0;
  for (; t < nt - 2; t += 2) {
    wg_tile<0, true, true, 6>(r, ra, rb, lds_w, gA, gB, la, lb, tileA, tileB,
                              t);
    wg_tile<1, true, true, 6>(r, ra, rb, lds_w, gA, gB, la, lb, tileA, tileB,
                              t + 1);
  }
  wg_tile<0, true, false, 0>(r, ra, rb, lds_w, gA, gB, la, lb, tileA, tileB,
                             t);
  wg_tile<1, false, false, -1>(r, ra, rb, lds_w, gA, gB, la, lb, tileA, tileB,
                               t + 1);
  if (STAGGER && !wr) __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  // epilogue: 128 output rows (one ha) at a time through LDS as
  // [128][256] bf16, then whole 512-byte rows to global memory. The last
  // phase ended in a barrier, so every wave is done reading the stages.
  short* const ep = reinterpret_cast<short*>(smem);
  const int hi = lane >> 5, c32 = lane & 31;
#pragma unroll
  for (int ha = 0; ha < 2; ++ha) {
#pragma unroll
    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const int row = 64 * wr + 32 * i + (g & 3) + 8 * (g >> 2) + 4 * hi;
          const int col = 128 * hb + 32 * wc + c32;
          ep[row * 256 + col] =
              __builtin_bit_cast(short, (__bf16)r.acc[ha][hb][i][g]);
        }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int c = tid + 512 * it;
      const int row = c >> 5, ch = c & 31;
      const short8 v = *reinterpret_cast<const short8*>(ep + row * 256 + 8 * ch);
      *reinterpret_cast<short8*>(
          out + ((long long)tn_l * 256 + 128 * ha + row) * ldo +
          (long long)tk * 256 + 8 * ch) = v;
    }
    __syncthreads();
  }
}
