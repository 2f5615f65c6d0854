// Paged-KV decode attention for serving (one query token per sequence).
//
// Cache layout: k_cache / v_cache [num_pages, Hkv, PAGE, D], so one
// (page, kv-head) slab of PAGE*D elements is contiguous. Page 0 is the
// reserved null page: unused block_table entries hold 0 and the
// allocator never hands it out, so a stray index stays inside the
// allocation.
//
// paged_attn_decode_kernel: grid (num_splits, Hkv, B), 4 waves. A block
// owns one (sequence, kv head, KV slice) and serves all REP = Hq/Hkv
// query heads of that kv head, so K and V stream from HBM once per
// group. Decode is a pure KV stream at <= 8 query rows: K/V go
// straight to VGPRs with 16-byte loads (no LDS staging, no MFMA).
// D/8 lanes cover one token row; a wave-load covers 64/(D/8) tokens and
// four such loads are issued back to back before any math. q for the
// REP heads sits in registers pre-scaled by log2e/sqrt(D) (each lane
// keeps only its own 8-column slice). The dot product is reduced
// across the lane group by DPP; each lane group runs an fp32 online
// softmax (exp2, one rescale per batch of four rows) and accumulates
// P.V in fp32 for its 8 columns. Lane groups merge by shuffles, the 4
// waves merge through LDS once at the end.
//
// Tokens at or beyond seq_len (tail slots of the last page, the null
// page) are never loaded or used: the pool is uninitialised memory and
// 0 x NaN is NaN, so masking by a zero probability would not do.
//
// FP8 caches (FP8 = true): pages hold OCP e4m3fn bytes, value =
// byte * scale with one static (k_scale, v_scale) pair per pool. A lane
// loads EPL = PA_FP8_EPL bytes = EPL elements (D/EPL lanes per row, so
// a lane keeps an EPL-column slice of q and of the accumulators) and
// v_cvt_pk_f32_fp8 turns each 32-bit word into the two float pairs the
// packed FMAs consume. No per-element multiply: k_scale is folded into
// qscale by the binding, v_scale (oscale) into the final
// normalisation, or into the partial o before it goes to the
// workspace, so the reduce kernel is the same for both formats.
//
// num_splits == 1 writes bf16 output directly; otherwise each block
// writes unnormalised fp32 partials (m, l, o) to a workspace and
// paged_attn_reduce_bf16 combines them: two plain launches, no
// in-launch cross-workgroup combine. seq_lens and block_table are read
// on the device, so a captured graph replays for any lengths.
#include "common.h"

#define PA_PAGE 16
#define PA_WAVES 4
#define PA_UNROLL 4
// Cache elements a lane loads per row from an fp8 cache. 16 (16-byte
// loads, D/16 lanes per row, twice the tokens per wave-load) measured
// 76 us against 117 us for 8 (the bf16 lane mapping with 8-byte loads)
// at B 32, seq_len 4096, Hq 32, Hkv 8, D 128, where bf16 takes 149 us:
// 8-byte loads leave the kernel short of requests in flight.
#ifndef PA_FP8_EPL
#define PA_FP8_EPL 16
#endif

// weight of a partial with running max m when merged under max M
DEV_INLINE float pa_w(float m, float M) {
  return (m == -INFINITY) ? 0.f : exp2f(m - M);
}

// Sum over the LPR (4, 8 or 16) adjacent lanes that share a token row,
// by DPP: two quad permutes, then the (LPR >= 8) half-row and
// (LPR == 16) full-row mirrors. Every lane ends with the group total.
// All lanes must be active.
template <int CTRL>
DEV_INLINE float dpp_add(float v) {
  const int x = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf,
                                            0xf, true);
  return v + __int_as_float(x);
}

template <int LPR>
DEV_INLINE float group_sum(float v) {
  static_assert(LPR == 4 || LPR == 8 || LPR == 16,
                "lane group is 4, 8 or 16 lanes");
  v = dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]
  if (LPR >= 8) v = dpp_add<0x141>(v);   // row_half_mirror
  if (LPR == 16) v = dpp_add<0x140>(v);  // row_mirror
  return v;
}

// NW 32-bit words: what one lane loads of a cache row
template <int NW>
struct pa_words {
  typedef int type __attribute__((ext_vector_type(NW)));
};

// The lane's row slice as float pairs. bf16: a word is one pair. fp8:
// a word is four e4m3fn bytes, two pairs.
template <bool FP8, int NW, int NP>
DEV_INLINE void pa_unpack(const typename pa_words<NW>::type& w,
                          float2v (&x)[NP]) {
  if constexpr (FP8) {
    static_assert(NP == 2 * NW, "four fp8 elements per word");
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      x[2 * i] = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false);
      x[2 * i + 1] = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);
    }
  } else {
    static_assert(NP == NW && NW == 4, "two bf16 elements per word");
    const short8 s = __builtin_bit_cast(short8, w);
#pragma unroll
    for (int j = 0; j < NP; ++j)
      x[j] = float2v{bf2f(s[2 * j]), bf2f(s[2 * j + 1])};
  }
}

// FP8: cache elements are e4m3fn bytes, else bf16. EPL: elements of a
// row per lane (8 for bf16; 8 or 16 for fp8).
template <int D, int REP, bool FP8, int EPL>
__global__ __launch_bounds__(256) void paged_attn_decode_kernel(
    const short* __restrict__ Q,        // [B, Hq, D]
    const void* __restrict__ Kc_,       // [num_pages, Hkv, PAGE, D]
    const void* __restrict__ Vc_,
    const int* __restrict__ block_table,  // [B, max_pages]
    const int* __restrict__ seq_lens,     // [B]
    short* __restrict__ Out,            // [B, Hq, D] (num_splits == 1)
    float* __restrict__ ws_o,           // [B, Hq, S, D]
    float* __restrict__ ws_ml,          // [B, Hq, S, 2]
    int Hkv, int num_pages, int max_pages, float qscale, float oscale) {
  static_assert(EPL == 8 || (FP8 && EPL == 16), "8 or 16 elements per lane");
  constexpr int EB = FP8 ? 1 : 2;      // bytes per cache element
  constexpr int NW = EPL * EB / 4;     // words a lane loads per row
  constexpr int NP = EPL / 2;          // float pairs per lane
  typedef typename pa_words<NW>::type words_t;
  const char* Kc = static_cast<const char*>(Kc_);
  const char* Vc = static_cast<const char*>(Vc_);
  constexpr int LPR = D / EPL;         // lanes per token row
  constexpr int TPW = 64 / LPR;        // tokens per wave-load
  constexpr int TPI = TPW * PA_UNROLL; // tokens per wave iteration
  static_assert(TPI % PA_PAGE == 0, "wave iteration must cover whole pages");

  const int split = blockIdx.x, S = gridDim.x;
  const int hkv = blockIdx.y;
  const int b = blockIdx.z;
  const int Hq = Hkv * REP;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int g = lane / LPR;    // token within the wave-load
  const int sub = lane % LPR;  // EPL-column slice of the row

  int L = seq_lens[b];
  L = min(max(L, 0), max_pages * PA_PAGE);  // never leave the block table
  const int pages = (L + PA_PAGE - 1) / PA_PAGE;
  const int pps = (pages + S - 1) / S;      // pages per split
  const int start = split * pps * PA_PAGE;
  const int end = min(L, start + pps * PA_PAGE);

  // q and the output accumulators as float pairs: the dot product and
  // P.V compile to packed fp32 FMAs
  float2v q2[REP][NP];
#pragma unroll
  for (int r = 0; r < REP; ++r) {
#pragma unroll
    for (int c = 0; c < EPL / 8; ++c) {
      const short8 qv = *reinterpret_cast<const short8*>(
          Q + ((long long)b * Hq + hkv * REP + r) * D + sub * EPL + c * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        q2[r][4 * c + j] =
            float2v{bf2f(qv[2 * j]), bf2f(qv[2 * j + 1])} * qscale;
    }
  }

  float m[REP], l[REP];
  float2v o2[REP][NP];
#pragma unroll
  for (int r = 0; r < REP; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j) o2[r][j] = float2v{0.f, 0.f};
  }

  const int* bt = block_table + (long long)b * max_pages;
  for (int t0 = start + wave * TPI; t0 < end; t0 += PA_WAVES * TPI) {
    // PA_UNROLL K and V row loads in flight before any math. Rows at or
    // past `end` are not loaded: they stay zero and get probability 0.
    words_t kv[PA_UNROLL], vv[PA_UNROLL];
    bool ok[PA_UNROLL];
#pragma unroll
    for (int u = 0; u < PA_UNROLL; ++u) {
      const int t = t0 + u * TPW + g;
      ok[u] = t < end;
      kv[u] = words_t{};
      vv[u] = kv[u];
      if (ok[u]) {
        int page = bt[t / PA_PAGE];
        page = min(max(page, 0), num_pages - 1);
        const long long off =
            ((((long long)page * Hkv + hkv) * PA_PAGE + (t % PA_PAGE)) * D +
             sub * EPL) * EB;
        kv[u] = *reinterpret_cast<const words_t*>(Kc + off);
        vv[u] = *reinterpret_cast<const words_t*>(Vc + off);
      }
    }
    // scores of the PA_UNROLL rows for every head; ok[u] is uniform over
    // a lane group and all lanes take part in the cross-lane sums
    float s[PA_UNROLL][REP];
#pragma unroll
    for (int u = 0; u < PA_UNROLL; ++u) {
      float2v k2[NP];
      pa_unpack<FP8, NW, NP>(kv[u], k2);
#pragma unroll
      for (int r = 0; r < REP; ++r) {
        float2v acc = k2[0] * q2[r][0];
#pragma unroll
        for (int j = 1; j < NP; ++j) acc = k2[j] * q2[r][j] + acc;
        s[u][r] = group_sum<LPR>(acc[0] + acc[1]);
      }
    }
    // one online-softmax step per head for the whole batch of rows
    float p[PA_UNROLL][REP], a[REP];
#pragma unroll
    for (int r = 0; r < REP; ++r) {
      float mn = m[r];
#pragma unroll
      for (int u = 0; u < PA_UNROLL; ++u)
        mn = ok[u] ? fmaxf(mn, s[u][r]) : mn;
      a[r] = pa_w(m[r], mn);  // 0 while nothing has been seen yet
      float ps = 0.f;
#pragma unroll
      for (int u = 0; u < PA_UNROLL; ++u) {
        p[u][r] = ok[u] ? exp2f(s[u][r] - mn) : 0.f;
        ps += p[u][r];
      }
      m[r] = mn;
      l[r] = l[r] * a[r] + ps;
#pragma unroll
      for (int j = 0; j < NP; ++j) o2[r][j] *= a[r];
    }
#pragma unroll
    for (int u = 0; u < PA_UNROLL; ++u) {
      float2v v2[NP];
      pa_unpack<FP8, NW, NP>(vv[u], v2);
#pragma unroll
      for (int r = 0; r < REP; ++r)
#pragma unroll
        for (int j = 0; j < NP; ++j) o2[r][j] = v2[j] * p[u][r] + o2[r][j];
    }
  }

  float o[REP][EPL];
#pragma unroll
  for (int r = 0; r < REP; ++r)
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      o[r][2 * j] = o2[r][j][0];
      o[r][2 * j + 1] = o2[r][j][1];
    }

  // merge the lane groups of a wave
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1) {
#pragma unroll
    for (int r = 0; r < REP; ++r) {
      const float m2 = __shfl_xor(m[r], off, 64);
      const float l2 = __shfl_xor(l[r], off, 64);
      const float mn = fmaxf(m[r], m2);
      const float a1 = pa_w(m[r], mn), a2 = pa_w(m2, mn);
      m[r] = mn;
      l[r] = l[r] * a1 + l2 * a2;
#pragma unroll
      for (int j = 0; j < EPL; ++j) {
        const float o2 = __shfl_xor(o[r][j], off, 64);
        o[r][j] = o[r][j] * a1 + o2 * a2;
      }
    }
  }

  // merge the waves through LDS
  __shared__ float s_m[PA_WAVES][REP];
  __shared__ float s_l[PA_WAVES][REP];
  __shared__ float s_o[PA_WAVES][REP][D];
  if (g == 0) {
#pragma unroll
    for (int r = 0; r < REP; ++r) {
      if (sub == 0) {
        s_m[wave][r] = m[r];
        s_l[wave][r] = l[r];
      }
#pragma unroll
      for (int j = 0; j < EPL; ++j) s_o[wave][r][sub * EPL + j] = o[r][j];
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < REP * D; idx += 256) {
    const int r = idx / D, d = idx % D;
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < PA_WAVES; ++w) M = fmaxf(M, s_m[w][r]);
    float lsum = 0.f, osum = 0.f;
#pragma unroll
    for (int w = 0; w < PA_WAVES; ++w) {
      const float a = pa_w(s_m[w][r], M);
      lsum += s_l[w][r] * a;
      osum += s_o[w][r][d] * a;
    }
    const long long row = (long long)b * Hq + hkv * REP + r;
    if constexpr (FP8) osum *= oscale;  // v_scale, once per output element
    if (S == 1) {
      Out[row * D + d] = f2bf(lsum > 0.f ? osum / lsum : 0.f);
    } else {
      ws_o[(row * S + split) * D + d] = osum;
      if (d == 0) {
        ws_ml[(row * S + split) * 2 + 0] = M;  // -inf marks an empty slice
        ws_ml[(row * S + split) * 2 + 1] = lsum;
      }
    }
  }
}

// Combine the per-split partials: grid (Hq, B), D threads.
extern "C" __global__ void paged_attn_reduce_bf16(
    const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
    short* __restrict__ Out, int Hq, int S, int D) {
  const long long row = (long long)blockIdx.y * Hq + blockIdx.x;
  const int d = threadIdx.x;
  if (d >= D) return;
  float M = -INFINITY;
  for (int s = 0; s < S; ++s) M = fmaxf(M, ws_ml[(row * S + s) * 2]);
  float lsum = 0.f, osum = 0.f;
  for (int s = 0; s < S; ++s) {
    const float ms = ws_ml[(row * S + s) * 2];
    if (ms == -INFINITY) continue;  // empty slice: contributes nothing
    const float a = exp2f(ms - M);
    lsum += ws_ml[(row * S + s) * 2 + 1] * a;
    osum += ws_o[(row * S + s) * D + d] * a;
  }
  Out[row * D + d] = f2bf(lsum > 0.f ? osum / lsum : 0.f);
}

// The cache quantisation rule, one definition for every writer:
// e4m3fn_rne(clamp(x * inv_scale, -448, 448)) of 8 bf16 values, as 8
// bytes. The clamp comes first, so the conversion's overflow mode never
// matters; NaN passes through the clamp and converts to the NaN byte.
DEV_INLINE float pa_clamp448(float x) {
  return x != x ? x : fminf(fmaxf(x, -448.f), 448.f);
}

typedef __attribute__((ext_vector_type(2))) int pa_int2;

DEV_INLINE pa_int2 pa_quant8(const short8 x, float inv_scale) {
  pa_int2 w{0, 0};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    float f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      f[j] = pa_clamp448(bf2f(x[4 * i + j]) * inv_scale);
    int r = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
    w[i] = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], r, true);
  }
  return w;
}

// 8 elements at element offset `off` of a bf16 or fp8 cache
template <bool FP8>
DEV_INLINE void pa_store8(void* cache, long long off, const short8 x,
                          float inv_scale) {
  if constexpr (FP8)
    *reinterpret_cast<pa_int2*>(static_cast<char*>(cache) + off) =
        pa_quant8(x, inv_scale);
  else
    *reinterpret_cast<short8*>(static_cast<short*>(cache) + off) = x;
}

// Fused decode-step RoPE + KV append: one block per sequence row.
// Rotates q and k (rotate-halves, fp32 tables) at the row's own
// position, writes rotated k and raw v into page
// block_table[b, pos/PAGE] slot pos%PAGE, writes rotated q to Qout.
// Rows with pos < 0 (inactive slots), and rows whose pos lies outside
// the rope tables or the block table, touch no cache and get zero q.
// q/k/v may be slices of a fused QKV row: *_rs are row strides.
// FP8 caches store pa_quant8 of the same bf16 values (k rounded to bf16
// after the rotation, exactly what the bf16 cache would hold).
template <bool FP8>
__global__ __launch_bounds__(256) void rope_append_paged_kernel(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, long long q_rs, long long k_rs,
    long long v_rs, const float* __restrict__ cosT,
    const float* __restrict__ sinT, const int* __restrict__ pos,
    const int* __restrict__ block_table, void* __restrict__ Kc,
    void* __restrict__ Vc, short* __restrict__ Qout, int Hq, int Hkv,
    int D, int table_rows, int num_pages, int max_pages, float k_inv,
    float v_inv) {
  const int b = blockIdx.x;
  const int half = D / 2;
  const int hc = half / 8;  // 16-byte chunks per half row
  const int p = pos[b];
  const short8 zero = short8{0, 0, 0, 0, 0, 0, 0, 0};
  if (p < 0 || p >= table_rows || p / PA_PAGE >= max_pages) {
    for (int i = threadIdx.x; i < Hq * (D / 8); i += blockDim.x)
      *reinterpret_cast<short8*>(Qout + (long long)b * Hq * D + i * 8) = zero;
    return;
  }
  int page = block_table[(long long)b * max_pages + p / PA_PAGE];
  page = min(max(page, 0), num_pages - 1);
  const int slot = p % PA_PAGE;
  const float* cr = cosT + (long long)p * half;
  const float* sr = sinT + (long long)p * half;
  const int n_q = Hq * hc, n_k = Hkv * hc, n_v = Hkv * (D / 8);
  for (int i = threadIdx.x; i < n_q + n_k + n_v; i += blockDim.x) {
    if (i < n_q + n_k) {
      const bool is_q = i < n_q;
      const int w = is_q ? i : i - n_q;
      const int h = w / hc, c = (w % hc) * 8;
      const short* src = is_q ? Q + (long long)b * q_rs + h * D
                              : K + (long long)b * k_rs + h * D;
      const short8 x1 = *reinterpret_cast<const short8*>(src + c);
      const short8 x2 = *reinterpret_cast<const short8*>(src + half + c);
      short8 y1, y2;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float a = bf2f(x1[j]), bb = bf2f(x2[j]);
        const float cs = cr[c + j], sn = sr[c + j];
        y1[j] = f2bf(a * cs - bb * sn);
        y2[j] = f2bf(bb * cs + a * sn);
      }
      if (is_q) {
        short* dst = Qout + ((long long)b * Hq + h) * D;
        *reinterpret_cast<short8*>(dst + c) = y1;
        *reinterpret_cast<short8*>(dst + half + c) = y2;
      } else {
        const long long off =
            (((long long)page * Hkv + h) * PA_PAGE + slot) * D;
        pa_store8<FP8>(Kc, off + c, y1, k_inv);
        pa_store8<FP8>(Kc, off + half + c, y2, k_inv);
      }
    } else {
      const int w = i - n_q - n_k;
      const int h = w / (D / 8), c = (w % (D / 8)) * 8;
      pa_store8<FP8>(
          Vc, (((long long)page * Hkv + h) * PA_PAGE + slot) * D + c,
          *reinterpret_cast<const short8*>(V + (long long)b * v_rs + h * D + c),
          v_inv);
    }
  }
}

// Prefill-side append: rows k[t], v[t] (t < T, k already rotated) of one
// sequence go to cache rows pos0 + t of the pages in its block-table
// row bt, quantised by pa_quant8 when the cache is fp8. grid (T), one
// thread per 8 elements. A row whose page index is past the table, or
// whose page id is outside the pool, is not written.
template <bool FP8>
__global__ __launch_bounds__(256) void kv_append_paged_kernel(
    const short* __restrict__ K, const short* __restrict__ V,
    long long k_rs, long long v_rs, const int* __restrict__ bt, int pos0,
    void* __restrict__ Kc, void* __restrict__ Vc, int Hkv, int D,
    int num_pages, int max_pages, float k_inv, float v_inv) {
  const int t = blockIdx.x;
  const long long p = (long long)pos0 + t;
  if (p / PA_PAGE >= max_pages) return;
  const int page = bt[p / PA_PAGE];
  if (page < 0 || page >= num_pages) return;
  const int slot = (int)(p % PA_PAGE);
  const int cpr = D / 8;
  for (int i = threadIdx.x; i < 2 * Hkv * cpr; i += blockDim.x) {
    const bool is_k = i < Hkv * cpr;
    const int w = is_k ? i : i - Hkv * cpr;
    const int h = w / cpr, c = (w % cpr) * 8;
    const short* src = is_k ? K + (long long)t * k_rs + h * D + c
                            : V + (long long)t * v_rs + h * D + c;
    pa_store8<FP8>(is_k ? Kc : Vc,
                   (((long long)page * Hkv + h) * PA_PAGE + slot) * D + c,
                   *reinterpret_cast<const short8*>(src),
                   is_k ? k_inv : v_inv);
  }
}
