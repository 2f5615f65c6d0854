// Batched token sampling: temperature, top-k, top-p and the draw for every
// row of logits[B, V] in one launch. The rules are those of ops.sample_ref
// (ray_amd/ops/__init__.py); in short, per row with x the logits:
//   T <= 0        token = lowest index of max x, n_kept = 1
//   0 < k < V     keep x >= (k-th largest x), ties kept
//   p_i           exp((x_i - max x) / T) on kept tokens
//   top_p < 1     keep x >= tau, tau the largest value whose upper mass
//                 reaches top_p * (mass kept by top-k), ties kept
//   draw          smallest kept index whose running mass exceeds u * Z
// The random number u is an input, so the kernel is a pure function of its
// arguments: no host synchronisation, no workspace, legal in a captured
// graph, and bit-identical from call to call (see "Integers" below).
//
// Work split. One block of 1024 threads (16 waves, one CU) per row; thread
// t owns elements [8192*c + 8*t, +8) of every 8192-element chunk c, so a
// wave's 16-byte loads cover 1 KB of contiguous bf16. A bf16 row of at most
// 131072 tokens whose start is 16-byte aligned is read from global memory
// once and kept packed in 16 x 4 = 64 VGPRs per thread for every later pass
// (SampleRow<short, true>; all chunk loops are unrolled so the registers are
// indexed at compile time). fp32 rows, longer rows and rows whose start is
// not 16-byte aligned take SampleRow<T, false>, which reads the row again
// in each pass (a row is at most 4 MB and stays in L2): 16-byte loads when
// the row start is aligned, element loads otherwise, chosen by the launcher.
// The last partial group of 8 and everything past V are element loads under
// an index check, padded with a NaN pattern whose key is below that of
// every real value and which no pass keeps; nothing outside [0, V) of a row is read.
//
// Keys. A logit's fp32 bits b (bf16 widened) map to an unsigned key in
// value order: b >= 0 ? b | 2^31 : ~b, with -0 read as +0 so that a compare
// of keys is the compare of values. Every filter is a compare of keys.
// Pass 1 is a block max of (key, lowest index), which is all a greedy row
// needs: it stores its token and leaves.
//
// Top-k is a radix select on the key, 8 bits a pass from the top: two
// passes for bf16 (the low 16 key bits are the same for all elements of one
// sign), four for fp32. A pass adds 1 for every element that matches the
// digits chosen so far into bins[digit], a block scan over the bins in
// descending digit order finds the digit at which the running count
// reaches k, and k becomes the rank inside that digit.
// Top-p is the same walk with each bin carrying mass instead of 1, the
// target being ceil(top_p * mass kept by top-k), at least 1 so that
// top_p <= 0 keeps the argmax set. The draw uses the same scan three times:
// over per-chunk totals, over the per-thread totals of the chosen chunk,
// and inside the chosen thread's 8 elements, looking for running mass
// >= floor(u * Z) + 1.
//
// Integers. A mass is round(p_i * 2^40) in a u64; p_i <= 1 and V <= 2^20,
// so no sum overflows. Integer adds are associative: bins, chunk totals,
// the threshold and the drawn token are the same whatever order the lanes
// and waves arrive in, so there are no float atomics and no ordering
// assumptions anywhere. What the fixed point drops: a term below 2^-41 of
// the row's largest probability counts as 0 (such a token is never drawn,
// though it is still counted in n_kept when its logit is above the
// threshold), and every other term is rounded by at most 2^-41 of the
// maximum, which is below fp32's own 2^-24 relative rounding of p_i for
// every p_i above 2^-17. p_i itself is v_exp_f32 of (x_i - max) * (log2 e /
// T) with one fp32 rounding of the product: relative error about
// |arg| * 2^-24 + 2^-23, recomputed from the on-chip row in every pass
// that needs it, never stored.
//
// Bins. bf16 logits of one sign and exponent share their top key digit, so
// a wave's 64 adds of the first pass would meet in one or two LDS words.
// Each digit therefore has SAMPLE_COPIES = 16 copies in adjacent words,
// picked by lane & 15 (4 lanes per word instead of 64), summed when the
// bins are scanned. 256 x 16 x 8 B = 32 KB of the CU's 160 KB; the block
// owns the CU anyway.
//
// Not done: splitting one row over several blocks. B = 1 runs on one CU;
// measured at V = 128256 bf16 on the MI355X that is 22 us for a greedy row
// and 48 / 67 / 84 us for temperature / top-k / top-p rows, and 64 rows take
// about the same (PERFORMANCE.md, "Batched sampling").
#include <utility>

#include "common.h"

#define SAMPLE_THREADS 1024
#define SAMPLE_CHUNK (8 * SAMPLE_THREADS)
#define SAMPLE_ONCHIP_CHUNKS 16    // 131072 bf16
#define SAMPLE_MAX_CHUNKS 128      // V <= 2^20
#define SAMPLE_COPIES 16
// Padding is a negative NaN: key 0, or 0xffff when it went through the
// packed bf16 row. Every real value, -inf included, has a key of at least
// 0x007fffff, so "key >= SAMPLE_KEY_MIN" is "a real element".
#define SAMPLE_PAD 0xffffffffu
#define SAMPLE_KEY_MIN 0x00010000u

typedef unsigned long long u64s;
typedef __attribute__((ext_vector_type(4))) unsigned int sample_u32x4;

// f(integral_constant<int, c>) for c = 0 .. N-1: the on-chip row is indexed
// with constants from the front end on, so it is split into registers
template <class F, int... C>
DEV_INLINE void sample_static_for(F f, std::integer_sequence<int, C...>) {
  (f(std::integral_constant<int, C>{}), ...);
}
#define SAMPLE_ONCHIP_SEQ \
  std::make_integer_sequence<int, SAMPLE_ONCHIP_CHUNKS> {}
#define SAMPLE_INLINE __attribute__((always_inline))

struct SampleSmem {
  u64s bins[256 * SAMPLE_COPIES];
  u64s wtot[SAMPLE_THREADS / 64];
  u64s sel_rem;
  int sel_idx;
  int n_kept;
};

// Values that are the same in every lane (read from LDS or from the row's
// parameters) move to SGPRs; the VGPRs are needed for the row.
DEV_INLINE unsigned sample_uniform(unsigned v) {
  return __builtin_amdgcn_readfirstlane(v);
}
DEV_INLINE u64s sample_uniform(u64s v) {
  return ((u64s)sample_uniform((unsigned)(v >> 32)) << 32) |
         sample_uniform((unsigned)v);
}

DEV_INLINE unsigned sample_key(unsigned b) {
  if (b == 0x80000000u) b = 0;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

DEV_INLINE float sample_key_value(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// round(exp((x - xmax) / T) * 2^40); scale = log2(e) / T. The product is
// pinned to its own VGPR so that neighbouring elements are not paired into
// packed fp32 instructions.
DEV_INLINE u64s sample_mass(unsigned b, float xmax, float scale) {
  float a = (__uint_as_float(b) - xmax) * scale;
  asm volatile("" : "+v"(a));
  const float p = __builtin_amdgcn_exp2f(a);
  return (u64s)(p * 0x1p40f + 0.5f);
}

// One row as seen by one thread. chunks(f) calls f(c, b) for every chunk c
// with b the fp32 bits of this thread's 8 elements (index 8192*c + 8*tid + e),
// SAMPLE_PAD past V.
template <typename T, bool ONCHIP>
struct SampleRow {
  const T* p;
  int V, nch, tid;
  bool vec;
  sample_u32x4 r[ONCHIP ? SAMPLE_ONCHIP_CHUNKS : 1];

  DEV_INLINE unsigned elem(int idx) const {
    if (idx >= V) return SAMPLE_PAD;
    if constexpr (sizeof(T) == 2)
      return ((unsigned)(unsigned short)p[idx]) << 16;
    else
      return __float_as_uint(p[idx]);
  }

  DEV_INLINE void fetch(int c, unsigned (&b)[8]) const {
    const int base = c * SAMPLE_CHUNK + tid * 8;
    if (vec && base + 8 <= V) {
      if constexpr (sizeof(T) == 2) {
        const sample_u32x4 w = *(const sample_u32x4*)(p + base);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          b[2 * d] = w[d] << 16;
          b[2 * d + 1] = w[d] & 0xffff0000u;
        }
      } else {
        const sample_u32x4 w0 = *(const sample_u32x4*)(p + base);
        const sample_u32x4 w1 = *(const sample_u32x4*)(p + base + 4);
#pragma unroll
        for (int d = 0; d < 4; ++d) { b[d] = w0[d]; b[4 + d] = w1[d]; }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) b[e] = elem(base + e);
    }
  }

  DEV_INLINE void load() {
    if constexpr (ONCHIP) {
      sample_static_for([&](auto c) SAMPLE_INLINE {
        const int base = c * SAMPLE_CHUNK + tid * 8;
        sample_u32x4 w;
        if (base + 8 <= V) {
          w = *(const sample_u32x4*)(p + base);
        } else {
#pragma unroll
          for (int d = 0; d < 4; ++d)
            w[d] = (elem(base + 2 * d) >> 16) |
                   (elem(base + 2 * d + 1) & 0xffff0000u);
        }
        r[c] = w;
      }, SAMPLE_ONCHIP_SEQ);
    }
  }

  // The empty asm makes every visit unpack again: without it the compiler
  // keeps all 128 unpacked values and keys of a thread alive across the
  // passes and spills them.
  DEV_INLINE void unpack(const sample_u32x4& w, unsigned (&b)[8]) const {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      unsigned x = w[d];
      asm volatile("" : "+v"(x));
      b[2 * d] = x << 16;
      b[2 * d + 1] = x & 0xffff0000u;
    }
  }

  template <class F>
  DEV_INLINE void chunks(F f) const {
    unsigned b[8];
    if constexpr (ONCHIP) {
      sample_static_for([&](auto c) SAMPLE_INLINE {
        if (c < nch) { unpack(r[c], b); f(c, b); }
      }, SAMPLE_ONCHIP_SEQ);
    } else {
      for (int c = 0; c < nch; ++c) { fetch(c, b); f(c, b); }
    }
  }

  // chunk c alone, c uniform over the block
  DEV_INLINE void chunk(int c, unsigned (&b)[8]) const {
    if constexpr (ONCHIP) {
      sample_u32x4 w = r[0];
      sample_static_for([&](auto i) SAMPLE_INLINE {
        if (i == c) w = r[i];
      }, SAMPLE_ONCHIP_SEQ);
      unpack(w, b);
    } else {
      fetch(c, b);
    }
  }
};

// Inclusive scan of v over the block in thread order; total: the block sum.
DEV_INLINE u64s sample_scan(u64s v, SampleSmem& sm, u64s& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64s incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const u64s t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) sm.wtot[wave] = incl;
  __syncthreads();
  u64s before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < SAMPLE_THREADS / 64; ++w) {
    const u64s t = sm.wtot[w];
    total += t;
    if (w < wave) before += t;
  }
  __syncthreads();
  return incl + before;
}

// The one thread whose running sum reaches `target` (1 <= target <= total)
// publishes its index and the part of the target that falls inside it.
DEV_INLINE void sample_publish(u64s v, u64s incl, u64s target,
                               SampleSmem& sm) {
  if (incl >= target && incl - v < target) {
    sm.sel_idx = threadIdx.x;
    sm.sel_rem = target - (incl - v);
  }
  __syncthreads();
}

DEV_INLINE void sample_zero_bins(SampleSmem& sm, int n) {
  for (int i = threadIdx.x; i < n * SAMPLE_COPIES; i += SAMPLE_THREADS)
    sm.bins[i] = 0;
  __syncthreads();
}

DEV_INLINE u64s sample_bin(const SampleSmem& sm, int i) {
  u64s s = 0;
#pragma unroll
  for (int j = 0; j < SAMPLE_COPIES; ++j) s += sm.bins[i * SAMPLE_COPIES + j];
  return s;
}

// Radix select over the elements with key >= lo. MASS false: the key of the
// element of rank `target` from the top (weights 1). MASS true: the largest
// key whose upper mass reaches ceil(top_p * total mass).
template <int NPASS, bool MASS, class Row>
DEV_INLINE unsigned sample_select(const Row& row, SampleSmem& sm, unsigned lo,
                                  u64s target, float top_p, float xmax,
                                  float scale) {
  const int tid = threadIdx.x, copy = tid & (SAMPLE_COPIES - 1);
  unsigned prefix = 0, mask = 0;
#pragma unroll 1
  for (int pass = 0; pass < NPASS; ++pass) {
    const int shift = 24 - 8 * pass;
    sample_zero_bins(sm, 256);
    row.chunks([&](int, const unsigned (&b)[8]) SAMPLE_INLINE {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned key = sample_key(b[e]);
        if (key >= lo && (key & mask) == prefix) {
          const u64s w = MASS ? sample_mass(b[e], xmax, scale) : 1;
          if (!MASS || w)
            atomicAdd(&sm.bins[((key >> shift) & 255) * SAMPLE_COPIES + copy],
                      w);
        }
      }
    });
    __syncthreads();
    const u64s v = tid < 256 ? sample_bin(sm, 255 - tid) : 0;
    u64s total;
    const u64s incl = sample_scan(v, sm, total);
    if (MASS && pass == 0) {
      const double want = (double)fminf(fmaxf(top_p, 0.f), 1.f) * (double)total;
      target = (u64s)ceil(want);
      target = target < 1 ? 1 : (target > total ? total : target);
      target = sample_uniform(target);
    }
    sample_publish(v, incl, target, sm);
    prefix |= sample_uniform(255u - (unsigned)sm.sel_idx) << shift;
    mask |= 255u << shift;
    target = sample_uniform(sm.sel_rem);
  }
  return prefix;
}

template <typename T, bool ONCHIP>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_kernel(
    const T* __restrict__ logits, long long row_stride, int V, int vec,
    const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const float* __restrict__ u,
    long long* __restrict__ tokens, int* __restrict__ n_kept) {
  __shared__ SampleSmem sm;
  constexpr int NPASS = sizeof(T) == 2 ? 2 : 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rowi = blockIdx.x;

  SampleRow<T, ONCHIP> row;
  row.p = logits + (long long)rowi * row_stride;
  row.V = V;
  row.nch = (V + SAMPLE_CHUNK - 1) / SAMPLE_CHUNK;
  row.tid = tid;
  row.vec = vec != 0;
  row.load();
  if (tid == 0) { sm.sel_idx = 0; sm.sel_rem = 1; sm.n_kept = 0; }

  // pass 1: max key, lowest index among its holders
  unsigned bk = 0, bi = 0;
  row.chunks([&](int c, const unsigned (&b)[8]) SAMPLE_INLINE {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned key = sample_key(b[e]);
      if (key > bk) { bk = key; bi = c * SAMPLE_CHUNK + tid * 8 + e; }
    }
  });
  u64s best = ((u64s)bk << 32) | (0xffffffffu - bi);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64s t = __shfl_xor(best, off, 64);
    best = t > best ? t : best;
  }
  if (lane == 0) sm.wtot[wave] = best;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < SAMPLE_THREADS / 64; ++w) {
    const u64s t = sm.wtot[w];
    best = t > best ? t : best;
  }
  __syncthreads();
  best = sample_uniform(best);

  const float temp = temperature[rowi];
  if (!(temp > 0.f)) {
    if (tid == 0) {
      tokens[rowi] = (long long)(0xffffffffu - (unsigned)best);
      n_kept[rowi] = 1;
    }
    return;
  }
  const float xmax = sample_key_value((unsigned)(best >> 32));
  const float scale = __uint_as_float(sample_uniform(
      __float_as_uint((float)(1.4426950408889634 / (double)temp))));

  unsigned lo = SAMPLE_KEY_MIN;  // every real element
  const int k = top_k[rowi];
  if (k > 0 && k < V)
    lo = sample_select<NPASS, false>(row, sm, lo, (u64s)k, 0.f, xmax, scale);
  const float tp = top_p[rowi];
  if (tp < 1.f)
    lo = sample_select<NPASS, true>(row, sm, lo, 0, tp, xmax, scale);

  // draw, level 1: mass per 8192-element chunk, and the kept count
  const int copy = tid & (SAMPLE_COPIES - 1);
  sample_zero_bins(sm, row.nch);
  int cnt = 0;
  row.chunks([&](int c, const unsigned (&b)[8]) SAMPLE_INLINE {
    u64s s = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (sample_key(b[e]) >= lo) {
        s += sample_mass(b[e], xmax, scale);
        ++cnt;
      }
    if (s) atomicAdd(&sm.bins[c * SAMPLE_COPIES + copy], s);
  });
  if (cnt) atomicAdd(&sm.n_kept, cnt);  // once per thread and row
  __syncthreads();
  u64s v = tid < row.nch ? sample_bin(sm, tid) : 0;
  u64s Z;
  u64s incl = sample_scan(v, sm, Z);
  // smallest index with running mass > floor(u * Z): running mass >= target
  u64s target = (u64s)((double)u[rowi] * (double)Z);
  target = sample_uniform(target >= Z ? Z : target + 1);
  sample_publish(v, incl, target, sm);
  const int cstar = (int)sample_uniform((unsigned)sm.sel_idx);
  target = sample_uniform(sm.sel_rem);
  if (tid == 0) n_kept[rowi] = sm.n_kept;

  // level 2: the thread inside the chunk; level 3: the element inside it
  unsigned b[8];
  u64s m[8];
  row.chunk(cstar, b);
  v = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    m[e] = sample_key(b[e]) >= lo ? sample_mass(b[e], xmax, scale) : 0;
    v += m[e];
  }
  u64s unused;
  incl = sample_scan(v, sm, unused);
  if (incl >= target && incl - v < target) {
    const u64s want = target - (incl - v);
    u64s run = 0;
    int tok = -1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      run += m[e];
      if (tok < 0 && run >= want) tok = e;
    }
    tokens[rowi] = (long long)cstar * SAMPLE_CHUNK + tid * 8 + tok;
  }
}
