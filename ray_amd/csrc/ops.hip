// ray_amd HIP ops extension: torch bindings for the CDNA4 kernels.
// Built directly with hipcc for gfx950 (no hipify, no CUDA path) by
// ray_amd/csrc/build.py -> ray_amd/_hip_ops.so (in-tree).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "hip/rmsnorm.hip"
#include "hip/elementwise.hip"
#include "hip/rl_scans.hip"
#include "hip/cross_entropy.hip"
// Flash attention has two paths, chosen from the shape alone:
//   T % 256 == 0: 256-row kernels (fwd v7, dq v5, dkv v6), which read
//                 contiguous BHTD or BTHD-view tensors;
//   otherwise:    128-row kernels (fwd v5, dq v3, the two instances of dkv
//                 v3), contiguous BHTD.
// Each file below compiles on its own.
#include "hip/flash_attn_v5.hip"
#include "hip/flash_attn_v7.hip"
#include "hip/fa_bwd_prep.hip"
#include "hip/fa_bwd_v3.hip"
#include "hip/fa_bwd_dq_v5.hip"
#include "hip/fa_bwd_dkv_v6.hip"
#include "hip/gemv.hip"
#include "hip/paged_attn.hip"
#include "hip/paged_attn_prefill.hip"
#include "hip/gemm_wgrad.hip"

#define CHECK_IN(x)                                                     \
  TORCH_CHECK(x.is_cuda(), #x " must be on GPU");                       \
  TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

static inline hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

static inline bool aligned16(const at::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

static inline int grid_for(long long n, int block = 256, int cap = 2048) {
  long long g = (n + block - 1) / block;
  return (int)std::min<long long>(g, cap);
}

// ---------------- RMSNorm ----------------

// The kernels read x, w and dy as raw bf16 with 16-byte loads: another
// dtype would be reinterpreted bit for bit, so it is refused here.
#define CHECK_RMS_BF16(t)                                               \
  CHECK_IN(t);                                                          \
  TORCH_CHECK(t.scalar_type() == at::kBFloat16,                         \
              "rmsnorm: " #t " must be bf16, got ", t.scalar_type());   \
  TORCH_CHECK(aligned16(t), "rmsnorm: " #t " must be 16-byte aligned")

static int rmsnorm_check_hw(const at::Tensor& x, const at::Tensor& w) {
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0, "rmsnorm: x must be [..., H]");
  TORCH_CHECK(x.size(-1) % 8 == 0 && x.size(-1) < (1ll << 31),
              "rmsnorm: H must be a multiple of 8");
  TORCH_CHECK(w.dim() == 1 && w.size(0) == x.size(-1),
              "rmsnorm: w must be [H]");
  return (int)x.size(-1);
}

std::vector<at::Tensor> rmsnorm_fwd(at::Tensor x, at::Tensor w, double eps) {
  CHECK_RMS_BF16(x);
  CHECK_RMS_BF16(w);
  int H = rmsnorm_check_hw(x, w);
  long long N = x.numel() / H;
  auto y = at::empty_like(x);
  auto inv = at::empty({N}, x.options().dtype(at::kFloat));
  hipLaunchKernelGGL(rmsnorm_fwd_bf16, dim3((unsigned)N), dim3(256), 0,
                     cur_stream(), (const short*)x.data_ptr(),
                     (const short*)w.data_ptr(), (short*)y.data_ptr(),
                     inv.data_ptr<float>(), H, (float)eps);
  return {y, inv};
}

static long long rmsnorm_bwd_check(const at::Tensor& dy, const at::Tensor& x,
                                   const at::Tensor& w, const at::Tensor& inv,
                                   int* H_out) {
  CHECK_RMS_BF16(dy); CHECK_RMS_BF16(x); CHECK_RMS_BF16(w); CHECK_IN(inv);
  int H = rmsnorm_check_hw(x, w);
  long long N = x.numel() / H;
  TORCH_CHECK(dy.sizes() == x.sizes(), "rmsnorm: dy must have x's shape");
  TORCH_CHECK(inv.scalar_type() == at::kFloat && inv.numel() == N,
              "rmsnorm: inv must be fp32 [N]");
  *H_out = H;
  return N;
}

// dx kernel, then a second pass over dy and x for dw (atomic adds across
// row splits). Serves an H the one-pass kernel's template does not cover
// (H > 8192). Bound for the tests and tools/glue_bench.py only, which
// compare the one-pass kernel with it; nothing in the package calls the
// binding.
std::vector<at::Tensor> rmsnorm_bwd_two_pass(at::Tensor dy, at::Tensor x,
                                             at::Tensor w, at::Tensor inv) {
  int H;
  long long N = rmsnorm_bwd_check(dy, x, w, inv, &H);
  auto dx = at::empty_like(x);
  auto dw = at::zeros({H}, x.options().dtype(at::kFloat));
  if (N == 0) return {dx, dw};
  hipLaunchKernelGGL(rmsnorm_bwd_dx_bf16, dim3((unsigned)N), dim3(256), 0,
                     cur_stream(), (const short*)dy.data_ptr(),
                     (const short*)x.data_ptr(), (const short*)w.data_ptr(),
                     inv.data_ptr<float>(), (short*)dx.data_ptr(), H);
  int row_splits = (int)std::min<long long>(256, std::max<long long>(1, N / 64));
  hipLaunchKernelGGL(rmsnorm_bwd_dw_bf16,
                     dim3((H + 255) / 256, row_splits), dim3(256), 0,
                     cur_stream(), (const short*)dy.data_ptr(),
                     (const short*)x.data_ptr(), inv.data_ptr<float>(),
                     dw.data_ptr<float>(), N, H);
  return {dx, dw};
}

static void launch_add_bf16(const at::Tensor& a, const at::Tensor& b,
                            at::Tensor& y) {
  long long n8 = a.numel() / 8;
  if (n8 == 0) return;
  hipLaunchKernelGGL(add_bf16, dim3(grid_for(n8)), dim3(256), 0, cur_stream(),
                     (const short*)a.data_ptr(), (const short*)b.data_ptr(),
                     (short*)y.data_ptr(), n8);
}

// One pass over dy and x: dx (plus g_res when given, rounded as the bf16
// add of the two tensors would be) and dw fp32 [H], summed in a fixed order.
// `grid` overrides the number of blocks (0: the default below); it is there
// for tools/glue_bench.py and the tests, the package always passes 0.
std::vector<at::Tensor> rmsnorm_bwd_res(at::Tensor dy, at::Tensor x,
                                        at::Tensor w, at::Tensor inv,
                                        c10::optional<at::Tensor> g_res,
                                        int64_t grid) {
  int H;
  long long N = rmsnorm_bwd_check(dy, x, w, inv, &H);
  const bool res = g_res.has_value();
  if (res) {
    CHECK_RMS_BF16((*g_res));
    TORCH_CHECK(g_res->sizes() == x.sizes(),
                "rmsnorm: g_res must have x's shape");
  }
  TORCH_CHECK(grid >= 0 && grid <= 65536, "rmsnorm: grid must be 0..65536");
  if (H > 4 * RMS_CHUNK || N == 0) {
    auto r = rmsnorm_bwd_two_pass(dy, x, w, inv);
    if (res) {
      auto sum = at::empty_like(r[0]);
      launch_add_bf16(r[0], *g_res, sum);
      r[0] = sum;
    }
    return r;
  }
  const long long blocks =
      grid ? grid
           : std::min<long long>(RMS_BWD_GRID, (N + RMS_BWD_MIN_ROWS - 1) /
                                                   RMS_BWD_MIN_ROWS);
  const int G = (int)std::min<long long>(N, blocks);
  auto dx = at::empty_like(x);
  auto part = at::empty({G, H}, x.options().dtype(at::kFloat));
  auto dw = at::empty({H}, x.options().dtype(at::kFloat));
  const short* gp = res ? (const short*)g_res->data_ptr() : nullptr;
#define RMS_BWD_LAUNCH(CC, RR)                                              \
  hipLaunchKernelGGL((rmsnorm_bwd_onepass_bf16<CC, RR>), dim3(G), dim3(256), \
                     0, cur_stream(), (const short*)dy.data_ptr(),          \
                     (const short*)x.data_ptr(), (const short*)w.data_ptr(), \
                     inv.data_ptr<float>(), gp, (short*)dx.data_ptr(),      \
                     part.data_ptr<float>(), N, H)
#define RMS_BWD_CHUNKS(CC)                                                  \
  if (res) { RMS_BWD_LAUNCH(CC, true); } else { RMS_BWD_LAUNCH(CC, false); }
  if (H <= RMS_CHUNK) { RMS_BWD_CHUNKS(1) }
  else if (H <= 2 * RMS_CHUNK) { RMS_BWD_CHUNKS(2) }
  else { RMS_BWD_CHUNKS(4) }
#undef RMS_BWD_CHUNKS
#undef RMS_BWD_LAUNCH
  hipLaunchKernelGGL(rmsnorm_dw_reduce_f32, dim3((H + 31) / 32), dim3(256), 0,
                     cur_stream(), part.data_ptr<float>(),
                     dw.data_ptr<float>(), G, H);
  return {dx, dw};
}

std::vector<at::Tensor> rmsnorm_bwd(at::Tensor dy, at::Tensor x, at::Tensor w,
                                    at::Tensor inv) {
  return rmsnorm_bwd_res(dy, x, w, inv, c10::nullopt, 0);
}

// s = bf16(x + r), h = rmsnorm(s), inv_rms: one pass
std::vector<at::Tensor> add_rmsnorm_fwd(at::Tensor x, at::Tensor r,
                                        at::Tensor w, double eps) {
  CHECK_RMS_BF16(x);
  CHECK_RMS_BF16(r);
  CHECK_RMS_BF16(w);
  int H = rmsnorm_check_hw(x, w);
  TORCH_CHECK(r.sizes() == x.sizes(), "add_rmsnorm: r must have x's shape");
  long long N = x.numel() / H;
  auto s = at::empty_like(x);
  if (N == 0)
    return {s, at::empty_like(x),
            at::empty({0}, x.options().dtype(at::kFloat))};
  if (H > 4 * RMS_CHUNK) {
    launch_add_bf16(x, r, s);
    auto yi = rmsnorm_fwd(s, w, eps);
    return {s, yi[0], yi[1]};
  }
  auto y = at::empty_like(x);
  auto inv = at::empty({N}, x.options().dtype(at::kFloat));
#define ADD_RMS_LAUNCH(CC)                                                  \
  hipLaunchKernelGGL((add_rmsnorm_fwd_bf16<CC>), dim3((unsigned)N),         \
                     dim3(256), 0, cur_stream(), (const short*)x.data_ptr(), \
                     (const short*)r.data_ptr(), (const short*)w.data_ptr(), \
                     (short*)s.data_ptr(), (short*)y.data_ptr(),            \
                     inv.data_ptr<float>(), H, (float)eps)
  if (H <= RMS_CHUNK) { ADD_RMS_LAUNCH(1); }
  else if (H <= 2 * RMS_CHUNK) { ADD_RMS_LAUNCH(2); }
  else { ADD_RMS_LAUNCH(4); }
#undef ADD_RMS_LAUNCH
  return {s, y, inv};
}

// ---------------- SwiGLU ----------------

at::Tensor swiglu_fwd(at::Tensor a, at::Tensor b) {
  CHECK_IN(a); CHECK_IN(b);
  TORCH_CHECK(a.numel() == b.numel() && a.numel() % 8 == 0);
  auto y = at::empty_like(a);
  long long n8 = a.numel() / 8;
  hipLaunchKernelGGL(swiglu_fwd_bf16, dim3(grid_for(n8)), dim3(256), 0,
                     cur_stream(), (const short*)a.data_ptr(),
                     (const short*)b.data_ptr(), (short*)y.data_ptr(), n8);
  return y;
}

std::vector<at::Tensor> swiglu_bwd(at::Tensor dy, at::Tensor a, at::Tensor b) {
  CHECK_IN(dy); CHECK_IN(a); CHECK_IN(b);
  auto da = at::empty_like(a);
  auto db = at::empty_like(b);
  long long n8 = a.numel() / 8;
  hipLaunchKernelGGL(swiglu_bwd_bf16, dim3(grid_for(n8)), dim3(256), 0,
                     cur_stream(), (const short*)dy.data_ptr(),
                     (const short*)a.data_ptr(), (const short*)b.data_ptr(),
                     (short*)da.data_ptr(), (short*)db.data_ptr(), n8);
  return {da, db};
}

// ---------------- RoPE ----------------

at::Tensor rope_apply(at::Tensor x, at::Tensor cosT, at::Tensor sinT,
                      int64_t n_heads, int64_t T, int64_t sign) {
  CHECK_IN(cosT); CHECK_IN(sinT);
  int D = (int)x.size(-1);
  long long rows = x.numel() / D;
  // accept a no-copy [B,T,H,D] slice of a fused-QKV row (contiguous
  // [H,D] tail, arbitrary (b,t)-row stride); anything else must be
  // contiguous
  long long in_rs = (long long)n_heads * D;
  if (!x.is_contiguous()) {
    TORCH_CHECK(x.dim() == 4 && x.stride(3) == 1 && x.stride(2) == D
                    && x.stride(0) == x.size(1) * x.stride(1),
                "rope: input must be contiguous or a fused-QKV slice");
    in_rs = (long long)x.stride(1);
  }
  auto y = x.is_contiguous()
               ? at::empty_like(x)
               : at::empty({x.size(0), x.size(1), x.size(2), x.size(3)},
                           x.options());
  // eight pairs per lane with 16-byte accesses where the layout allows it
  const bool vec = D % 16 == 0 && in_rs % 8 == 0 && aligned16(x) &&
                   aligned16(y) && aligned16(cosT) && aligned16(sinT);
  long long total = vec ? rows * (D / 16) : rows * (D / 2);
  if (total == 0) return y;
#define ROPE_LAUNCH(KERNEL)                                                 \
  hipLaunchKernelGGL(KERNEL, dim3(grid_for(total)), dim3(256), 0,           \
                     cur_stream(), (const short*)x.data_ptr(),              \
                     (short*)y.data_ptr(), cosT.data_ptr<float>(),          \
                     sinT.data_ptr<float>(), rows, D, (int)n_heads, (int)T, \
                     (int)sign, in_rs)
  if (vec) { ROPE_LAUNCH(rope_fwd_bf16); }
  else { ROPE_LAUNCH(rope_fwd_scalar_bf16); }
#undef ROPE_LAUNCH
  return y;
}

// ---------------- small-batch GEMV (decode linear) ----------------

at::Tensor gemv(at::Tensor x, at::Tensor w) {
  // x: [B, K] (B <= 8), w: [N, K] bf16 row-major -> y [B, N]
  CHECK_IN(x); CHECK_IN(w);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
              w.scalar_type() == at::kBFloat16, "gemv: bf16 only");
  int B = (int)x.size(0);
  long long K = x.size(1);
  int N = (int)w.size(0);
  TORCH_CHECK(B >= 1 && B <= 8, "gemv: batch must be 1..8");
  TORCH_CHECK(w.size(1) == K && K % 512 == 0, "gemv: K%512 != 0");
  auto y = at::empty({B, N}, x.options());
  int blocks = (int)std::min<long long>((N + 3) / 4, 4096);
  hipLaunchKernelGGL(gemv_bf16, dim3(blocks), dim3(256), 0, cur_stream(),
                     (const short*)w.data_ptr(), (const short*)x.data_ptr(),
                     (short*)y.data_ptr(), N, B, K);
  return y;
}

// ---------------- paged-KV decode attention ----------------

#define CHECK_I32(x)                                                    \
  CHECK_IN(x);                                                          \
  TORCH_CHECK(x.scalar_type() == at::kInt, #x " must be int32")

// Returns true for an fp8 (OCP e4m3fn) cache, false for bf16. The
// scales are the pool's static dequantisation factors: value = stored *
// scale. They only mean something for fp8, so anything but 1 with a
// bf16 cache is refused.
static bool check_paged_cache(const at::Tensor& k_cache,
                              const at::Tensor& v_cache, int Hkv, int D,
                              double k_scale, double v_scale) {
  CHECK_IN(k_cache); CHECK_IN(v_cache);
  TORCH_CHECK(k_cache.scalar_type() == v_cache.scalar_type(),
              "k_cache and v_cache must have the same dtype");
  const bool fp8 = k_cache.scalar_type() == at::kFloat8_e4m3fn;
  TORCH_CHECK(fp8 || k_cache.scalar_type() == at::kBFloat16,
              "paged cache must be bf16 or float8_e4m3fn, got ",
              k_cache.scalar_type());
  TORCH_CHECK(std::isfinite(k_scale) && k_scale > 0 &&
              std::isfinite(v_scale) && v_scale > 0,
              "paged cache scales must be positive and finite");
  TORCH_CHECK(fp8 || (k_scale == 1.0 && v_scale == 1.0),
              "paged cache scales other than 1 need an fp8 cache");
  // the widest load of an fp8 cache: a decode lane's PA_FP8_EPL bytes
  // (prefill staging and the appends move 8)
  if (fp8)
    TORCH_CHECK(
        reinterpret_cast<uintptr_t>(k_cache.data_ptr()) % PA_FP8_EPL == 0 &&
        reinterpret_cast<uintptr_t>(v_cache.data_ptr()) % PA_FP8_EPL == 0,
        "fp8 paged caches must be ", PA_FP8_EPL, "-byte aligned");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.sizes() == v_cache.sizes(),
              "k_cache/v_cache must both be [num_pages, Hkv, 16, D]");
  TORCH_CHECK(k_cache.size(0) >= 1 && k_cache.size(1) == Hkv &&
              k_cache.size(2) == PA_PAGE && k_cache.size(3) == D,
              "paged cache must be [num_pages, Hkv, 16, D] matching q/k");
  return fp8;
}

// What decode and prefill attention check alike: the head dimension, the
// caches (check_paged_cache, whose result is returned), the GQA ratio the
// kernels are instantiated for and the block table. *Hkv is the caches'.
static bool check_paged_attn(const at::Tensor& k_cache,
                             const at::Tensor& v_cache,
                             const at::Tensor& block_table, int B, int Hq,
                             int D, double k_scale, double v_scale, int* Hkv) {
  TORCH_CHECK(D == 64 || D == 128, "paged_attn: head_dim must be 64 or 128");
  TORCH_CHECK(k_cache.dim() == 4, "k_cache must be [num_pages, Hkv, 16, D]");
  *Hkv = (int)k_cache.size(1);
  const bool fp8 = check_paged_cache(k_cache, v_cache, *Hkv, D, k_scale,
                                     v_scale);
  TORCH_CHECK(*Hkv >= 1 && Hq % *Hkv == 0, "GQA requires Hq % Hkv == 0");
  const int rep = Hq / *Hkv;
  TORCH_CHECK(rep == 1 || rep == 2 || rep == 4 || rep == 8,
              "paged_attn: Hq/Hkv must be 1, 2, 4 or 8");
  TORCH_CHECK(block_table.dim() == 2 && block_table.size(0) == B &&
              block_table.size(1) >= 1,
              "block_table must be [B, max_pages]");
  return fp8;
}

static void launch_paged_reduce(const at::Tensor& ws, at::Tensor& out, int B,
                                int Hq, int D, int S) {
  const float* ws_o = ws.data_ptr<float>();
  const float* ws_ml = ws_o + (long long)B * Hq * S * D;
  hipLaunchKernelGGL(paged_attn_reduce_bf16, dim3(Hq, B), dim3(D), 0,
                     cur_stream(), ws_o, ws_ml, (short*)out.data_ptr(), Hq, S,
                     D);
}

// Combine split partials; workspace is [B*Hq*S*(D+2)] fp32 as written
// by paged_attn_decode (o partials, then (m, l) pairs).
at::Tensor paged_attn_reduce(at::Tensor workspace, int64_t B, int64_t Hq,
                             int64_t D, int64_t num_splits) {
  CHECK_IN(workspace);
  TORCH_CHECK(workspace.scalar_type() == at::kFloat, "workspace must be fp32");
  TORCH_CHECK(D == 64 || D == 128, "paged_attn: head_dim must be 64 or 128");
  TORCH_CHECK(B >= 1 && B <= 65535 && Hq >= 1 && Hq <= 65535 &&
              num_splits >= 1, "paged_attn_reduce: bad B/Hq/num_splits");
  TORCH_CHECK(workspace.numel() >= B * Hq * num_splits * (D + 2),
              "paged_attn: workspace too small");
  auto out = at::empty({B, Hq, D}, workspace.options().dtype(at::kBFloat16));
  launch_paged_reduce(workspace, out, (int)B, (int)Hq, (int)D,
                      (int)num_splits);
  return out;
}

template <int D, int REP, bool FP8, int EPL>
static void launch_paged_decode(const at::Tensor& q, const at::Tensor& kc,
                                const at::Tensor& vc, const at::Tensor& bt,
                                const at::Tensor& sl, at::Tensor& out,
                                float* ws_o, float* ws_ml, int S, int Hkv,
                                float k_scale, float v_scale) {
  int B = (int)q.size(0);
  hipLaunchKernelGGL((paged_attn_decode_kernel<D, REP, FP8, EPL>),
                     dim3(S, Hkv, B), dim3(256), 0, cur_stream(),
                     (const short*)q.data_ptr(), (const void*)kc.data_ptr(),
                     (const void*)vc.data_ptr(), bt.data_ptr<int>(),
                     sl.data_ptr<int>(), (short*)out.data_ptr(), ws_o, ws_ml,
                     Hkv, (int)kc.size(0), (int)bt.size(1),
                     1.4426950408889634f / sqrtf((float)D) * k_scale,
                     v_scale);
}

at::Tensor paged_attn_decode(at::Tensor q, at::Tensor k_cache,
                             at::Tensor v_cache, at::Tensor block_table,
                             at::Tensor seq_lens, int64_t num_splits,
                             c10::optional<at::Tensor> workspace,
                             double k_scale, double v_scale) {
  CHECK_IN(q);
  CHECK_I32(block_table);
  CHECK_I32(seq_lens);
  TORCH_CHECK(q.scalar_type() == at::kBFloat16, "q must be bf16");
  TORCH_CHECK(q.dim() == 3, "q must be [B, Hq, D]");
  int B = (int)q.size(0), Hq = (int)q.size(1), D = (int)q.size(2);
  int Hkv;
  const bool fp8 = check_paged_attn(k_cache, v_cache, block_table, B, Hq, D,
                                    k_scale, v_scale, &Hkv);
  int rep = Hq / Hkv;
  TORCH_CHECK(seq_lens.dim() == 1 && seq_lens.size(0) == B,
              "seq_lens must be [B]");
  TORCH_CHECK(B >= 1 && B <= 65535 && Hkv <= 65535,
              "paged_attn: B and Hkv must fit a grid dimension");
  int S = (int)num_splits;
  TORCH_CHECK(num_splits >= 1 && num_splits <= 1024,
              "paged_attn: num_splits must be 1..1024");
  auto out = at::empty({B, Hq, D}, q.options());
  at::Tensor ws;
  float *ws_o = nullptr, *ws_ml = nullptr;
  if (S > 1) {
    long long need = (long long)B * Hq * S * (D + 2);
    if (workspace.has_value()) {
      ws = *workspace;
      CHECK_IN(ws);
      TORCH_CHECK(ws.scalar_type() == at::kFloat && ws.numel() >= need,
                  "paged_attn: workspace must be fp32 with >= B*Hq*S*(D+2) "
                  "elements");
    } else {
      ws = at::empty({need}, q.options().dtype(at::kFloat));
    }
    ws_o = ws.data_ptr<float>();
    ws_ml = ws_o + (long long)B * Hq * S * D;
  }
#define PA_LAUNCH(DD, RR)                                                   \
  if (fp8)                                                                  \
    launch_paged_decode<DD, RR, true, PA_FP8_EPL>(                          \
        q, k_cache, v_cache, block_table, seq_lens, out, ws_o, ws_ml, S,    \
        Hkv, (float)k_scale, (float)v_scale);                               \
  else                                                                      \
    launch_paged_decode<DD, RR, false, 8>(q, k_cache, v_cache, block_table, \
                                          seq_lens, out, ws_o, ws_ml, S,    \
                                          Hkv, 1.f, 1.f)
#define PA_REP(DD)                                                          \
  switch (rep) {                                                            \
    case 1: PA_LAUNCH(DD, 1); break;                                        \
    case 2: PA_LAUNCH(DD, 2); break;                                        \
    case 4: PA_LAUNCH(DD, 4); break;                                        \
    default: PA_LAUNCH(DD, 8); break;                                       \
  }
  if (D == 64) { PA_REP(64) } else { PA_REP(128) }
#undef PA_REP
#undef PA_LAUNCH
  if (S > 1) launch_paged_reduce(ws, out, B, Hq, D, S);
  return out;
}

// Chunk prefill over the paged cache: q [B, Tq, Hq, D] at positions
// ctx_lens[b] .. ctx_lens[b]+Tq-1, whose own K/V are already appended.
at::Tensor paged_attn_prefill(at::Tensor q, at::Tensor k_cache,
                              at::Tensor v_cache, at::Tensor block_table,
                              at::Tensor ctx_lens, at::Tensor q_lens,
                              double k_scale, double v_scale) {
  CHECK_IN(q);
  CHECK_I32(block_table);
  CHECK_I32(ctx_lens);
  CHECK_I32(q_lens);
  TORCH_CHECK(q.scalar_type() == at::kBFloat16, "q must be bf16");
  TORCH_CHECK(q.dim() == 4, "q must be [B, Tq, Hq, D]");
  TORCH_CHECK(aligned16(q), "paged_attn_prefill: q must be 16-byte aligned");
  int B = (int)q.size(0), Hq = (int)q.size(2), D = (int)q.size(3);
  int Hkv;
  const bool fp8 = check_paged_attn(k_cache, v_cache, block_table, B, Hq, D,
                                    k_scale, v_scale, &Hkv);
  TORCH_CHECK(fp8 || (aligned16(k_cache) && aligned16(v_cache)),
              "paged_attn_prefill: caches must be 16-byte aligned");
  TORCH_CHECK(block_table.size(1) <= (1 << 26),
              "paged_attn_prefill: block table too wide");
  TORCH_CHECK(ctx_lens.dim() == 1 && ctx_lens.size(0) == B &&
              q_lens.dim() == 1 && q_lens.size(0) == B,
              "ctx_lens and q_lens must be [B]");
  TORCH_CHECK(q.size(1) >= 1 && q.size(1) <= (1 << 26),
              "paged_attn_prefill: Tq must be 1..2^26");
  int Tq = (int)q.size(1);
  TORCH_CHECK(B >= 1 && B <= 65535 && Hq <= 65535,
              "paged_attn_prefill: B and Hq must fit a grid dimension");
  auto out = at::empty_like(q);
  // 128-row query tiles (4 waves) while they are what fills the GPU;
  // once there are two such blocks for each of the 256 CUs, 256-row
  // tiles (8 waves) stage every K/V tile half as often per query row
  const long long blocks128 = (long long)((Tq + 127) / 128) * Hq * B;
  const int waves = blocks128 >= PP_WIDE_TILE_BLOCKS ? 8 : 4;
  dim3 grid((Tq + 32 * waves - 1) / (32 * waves), Hq, B);
#define PP_LAUNCH_T(DD, WW, FP8)                                             \
  hipLaunchKernelGGL((paged_attn_prefill_kernel<DD, WW, FP8>), grid,        \
                     dim3(64 * WW), 0, cur_stream(),                        \
                     (const short*)q.data_ptr(),                            \
                     (const void*)k_cache.data_ptr(),                       \
                     (const void*)v_cache.data_ptr(),                       \
                     block_table.data_ptr<int>(), ctx_lens.data_ptr<int>(), \
                     q_lens.data_ptr<int>(), (short*)out.data_ptr(), Tq,    \
                     Hq, Hkv, (int)k_cache.size(0),                         \
                     (int)block_table.size(1),                              \
                     1.0f / sqrtf((float)D) * (float)k_scale,               \
                     (float)v_scale)
#define PP_LAUNCH(DD, WW)                                                   \
  if (fp8) { PP_LAUNCH_T(DD, WW, true); } else { PP_LAUNCH_T(DD, WW, false); }
  if (D == 64) {
    if (waves == 4) { PP_LAUNCH(64, 4); } else { PP_LAUNCH(64, 8); }
  } else {
    if (waves == 4) { PP_LAUNCH(128, 4); } else { PP_LAUNCH(128, 8); }
  }
#undef PP_LAUNCH
#undef PP_LAUNCH_T
  return out;
}

// q [B,Hq,D], k/v [B,Hkv,D]: contiguous or slices of a fused QKV row
// (contiguous [H,D] tail, arbitrary 16-byte-aligned row stride).
static long long paged_row_stride(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.dim() == 3 && t.stride(2) == 1 && t.stride(1) == t.size(2),
              name, " must be [B, H, D] with a contiguous [H, D] tail");
  TORCH_CHECK(t.stride(0) % 8 == 0 && aligned16(t), name,
              " rows must be 16-byte aligned");
  return (long long)t.stride(0);
}

at::Tensor rope_append_paged(at::Tensor q, at::Tensor k, at::Tensor v,
                             at::Tensor cosT, at::Tensor sinT, at::Tensor pos,
                             at::Tensor block_table, at::Tensor k_cache,
                             at::Tensor v_cache, double k_scale,
                             double v_scale) {
  long long q_rs = paged_row_stride(q, "q");
  long long k_rs = paged_row_stride(k, "k");
  long long v_rs = paged_row_stride(v, "v");
  CHECK_IN(cosT); CHECK_IN(sinT);
  CHECK_I32(pos);
  CHECK_I32(block_table);
  int B = (int)q.size(0), Hq = (int)q.size(1), D = (int)q.size(2);
  int Hkv = (int)k.size(1);
  TORCH_CHECK(D == 64 || D == 128, "paged_attn: head_dim must be 64 or 128");
  TORCH_CHECK(k.size(0) == B && v.size(0) == B && k.size(2) == D &&
              v.size(2) == D && v.size(1) == Hkv,
              "q/k/v shapes disagree");
  const bool fp8 = check_paged_cache(k_cache, v_cache, Hkv, D, k_scale,
                                     v_scale);
  TORCH_CHECK(cosT.scalar_type() == at::kFloat &&
              sinT.scalar_type() == at::kFloat && cosT.dim() == 2 &&
              cosT.size(1) == D / 2 && sinT.sizes() == cosT.sizes(),
              "cosT/sinT must be fp32 [T, D/2]");
  TORCH_CHECK(pos.dim() == 1 && pos.size(0) == B, "pos must be [B]");
  TORCH_CHECK(block_table.dim() == 2 && block_table.size(0) == B &&
              block_table.size(1) >= 1,
              "block_table must be [B, max_pages]");
  auto q_rot = at::empty({B, Hq, D}, q.options());
  if (B == 0) return q_rot;
  // the stored value is x * fp32(1 / scale): the reciprocal is taken
  // in double and rounded once, as ops.quantize_kv_fp8 does
#define RA_LAUNCH(FP8)                                                      \
  hipLaunchKernelGGL(rope_append_paged_kernel<FP8>, dim3(B), dim3(256), 0,  \
                     cur_stream(), (const short*)q.data_ptr(),              \
                     (const short*)k.data_ptr(), (const short*)v.data_ptr(),\
                     q_rs, k_rs, v_rs, cosT.data_ptr<float>(),              \
                     sinT.data_ptr<float>(), pos.data_ptr<int>(),           \
                     block_table.data_ptr<int>(), k_cache.data_ptr(),       \
                     v_cache.data_ptr(), (short*)q_rot.data_ptr(), Hq, Hkv, \
                     D, (int)cosT.size(0), (int)k_cache.size(0),            \
                     (int)block_table.size(1), (float)(1.0 / k_scale),      \
                     (float)(1.0 / v_scale))
  if (fp8) { RA_LAUNCH(true); } else { RA_LAUNCH(false); }
#undef RA_LAUNCH
  return q_rot;
}

// Append T rows of one sequence to its pages: k (already rotated) and v
// [T, Hkv, D] go to cache rows pos0 .. pos0+T-1 through the sequence's
// block-table row, quantised when the caches are fp8.
void kv_append_paged(at::Tensor k, at::Tensor v, int64_t pos0,
                     at::Tensor block_table_row, at::Tensor k_cache,
                     at::Tensor v_cache, double k_scale, double v_scale) {
  long long k_rs = paged_row_stride(k, "k");
  long long v_rs = paged_row_stride(v, "v");
  CHECK_I32(block_table_row);
  int Hkv = (int)k.size(1), D = (int)k.size(2);
  TORCH_CHECK(D == 64 || D == 128, "paged_attn: head_dim must be 64 or 128");
  TORCH_CHECK(v.sizes() == k.sizes(), "k/v shapes disagree");
  const bool fp8 = check_paged_cache(k_cache, v_cache, Hkv, D, k_scale,
                                     v_scale);
  TORCH_CHECK(block_table_row.dim() == 1 && block_table_row.size(0) >= 1,
              "block_table_row must be [max_pages]");
  TORCH_CHECK(pos0 >= 0 && pos0 < (1ll << 31) && k.size(0) < (1ll << 31),
              "kv_append_paged: pos0 and T must be in 0..2^31");
  int T = (int)k.size(0);
  if (T == 0) return;
#define KA_LAUNCH(FP8)                                                      \
  hipLaunchKernelGGL(kv_append_paged_kernel<FP8>, dim3(T), dim3(128), 0,    \
                     cur_stream(), (const short*)k.data_ptr(),              \
                     (const short*)v.data_ptr(), k_rs, v_rs,                \
                     block_table_row.data_ptr<int>(), (int)pos0,            \
                     k_cache.data_ptr(), v_cache.data_ptr(), Hkv, D,        \
                     (int)k_cache.size(0), (int)block_table_row.size(0),    \
                     (float)(1.0 / k_scale), (float)(1.0 / v_scale))
  if (fp8) { KA_LAUNCH(true); } else { KA_LAUNCH(false); }
#undef KA_LAUNCH
}

// ---------------- weight-gradient GEMM ----------------

// [rows, cols] bf16, unit column stride, 16-byte-aligned rows (a column
// slice of a wider tensor qualifies); returns the row stride in elements
static long long wgrad_operand(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1 && t.stride(0) >= t.size(1),
              name, " must be 2-D with unit column stride");
  TORCH_CHECK(t.stride(0) % 8 == 0 && aligned16(t), name,
              " rows must be 16-byte aligned");
  TORCH_CHECK(t.size(1) % 256 == 0 && t.size(1) >= 256, name,
              ": columns must be a multiple of 256");
  return (long long)t.stride(0);
}

static void launch_wgrad(const at::Tensor& dy0, const at::Tensor& dy1,
                         const at::Tensor& x, at::Tensor& out0,
                         at::Tensor& out1, int problems) {
  const long long ldy = wgrad_operand(dy0, "dy");
  const long long ldx = wgrad_operand(x, "x");
  const long long ldo = wgrad_operand(out0, "out");
  const long long M = dy0.size(0), N = dy0.size(1), K = x.size(1);
  TORCH_CHECK(x.size(0) == M && M >= 128 && M % 128 == 0,
              "gemm_wgrad: dy and x need the same number of rows, a "
              "multiple of 128");
  TORCH_CHECK(out0.size(0) == N && out0.size(1) == K,
              "gemm_wgrad: out must be [N, K]");
  TORCH_CHECK(ldy * 64 < (1ll << 30) && ldx * 64 < (1ll << 30),
              "gemm_wgrad: row stride too large");
  if (problems == 2) {
    TORCH_CHECK(wgrad_operand(dy1, "dy1") == ldy && dy1.size(0) == M &&
                    dy1.size(1) == N,
                "gemm_wgrad: grouped dy operands must match");
    TORCH_CHECK(wgrad_operand(out1, "out1") == ldo && out1.size(0) == N &&
                    out1.size(1) == K,
                "gemm_wgrad: grouped outputs must match");
  }
  const int nt0 = (int)(N / 256), KT = (int)(K / 256);
  const int NT = nt0 * problems;
  TORCH_CHECK((long long)NT * KT < (1ll << 31), "gemm_wgrad: grid too large");
#define WGRAD_LAUNCH(ST)                                                     \
  hipLaunchKernelGGL(gemm_wgrad_bf16<ST>, dim3((unsigned)(NT * KT)),         \
                     dim3(512), 0, cur_stream(),                             \
                     (const short*)dy0.data_ptr(),                           \
                     (const short*)dy1.data_ptr(),                           \
                     (const short*)x.data_ptr(), (short*)out0.data_ptr(),    \
                     (short*)out1.data_ptr(), (int)M, ldy, ldx, ldo, NT,     \
                     nt0, KT)
  // read on every call, so one process can measure both variants
  if (getenv("RAY_AMD_WGRAD_NO_STAGGER") != nullptr) {
    WGRAD_LAUNCH(false);
  } else {
    WGRAD_LAUNCH(true);
  }
#undef WGRAD_LAUNCH
}

// dW[N,K] = dy[M,N]^T · x[M,K]; `out` may be a view with a larger row stride
at::Tensor gemm_wgrad(at::Tensor dy, at::Tensor x,
                      c10::optional<at::Tensor> out) {
  at::Tensor o = out.has_value()
                     ? *out
                     : at::empty({dy.size(1), x.size(1)}, dy.options());
  launch_wgrad(dy, dy, x, o, o, 1);
  return o;
}

// two problems that share x (the MLP's gate and up weights) in one grid
std::vector<at::Tensor> gemm_wgrad_grouped(at::Tensor dy0, at::Tensor dy1,
                                           at::Tensor x) {
  auto o0 = at::empty({dy0.size(1), x.size(1)}, dy0.options());
  auto o1 = at::empty_like(o0);
  launch_wgrad(dy0, dy1, x, o0, o1, 2);
  return {o0, o1};
}

// ---------------- AdamW ----------------

void adamw_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
                at::Tensor master, double lr, double beta1, double beta2,
                double eps, double wd, int64_t step, double grad_scale) {
  CHECK_IN(p); CHECK_IN(g); CHECK_IN(m); CHECK_IN(v);
  long long n = p.numel();
  float bc1 = 1.f - powf((float)beta1, (float)step);
  float bc2 = 1.f - powf((float)beta2, (float)step);
  if (p.scalar_type() == at::kBFloat16) {
    CHECK_IN(master);
    hipLaunchKernelGGL(adamw_step_bf16, dim3(grid_for(n)), dim3(256), 0,
                       cur_stream(), (short*)p.data_ptr(),
                       (const short*)g.data_ptr(), m.data_ptr<float>(),
                       v.data_ptr<float>(), master.data_ptr<float>(), n,
                       (float)lr, (float)beta1, (float)beta2, (float)eps,
                       (float)wd, bc1, bc2, (float)grad_scale);
  } else {
    hipLaunchKernelGGL(adamw_step_f32, dim3(grid_for(n)), dim3(256), 0,
                       cur_stream(), p.data_ptr<float>(),
                       g.data_ptr<float>(), m.data_ptr<float>(),
                       v.data_ptr<float>(), n, (float)lr, (float)beta1,
                       (float)beta2, (float)eps, (float)wd, bc1, bc2,
                       (float)grad_scale);
  }
}

// ---------------- RL scans ----------------

std::vector<at::Tensor> gae(at::Tensor rewards, at::Tensor values,
                            at::Tensor cont, double gamma, double lam) {
  CHECK_IN(rewards); CHECK_IN(values); CHECK_IN(cont);
  int T = (int)rewards.size(0);
  int B = (int)rewards.size(1);
  TORCH_CHECK(values.size(0) == T + 1, "values must be [T+1, B]");
  auto adv = at::empty_like(rewards);
  auto vt = at::empty_like(rewards);
  hipLaunchKernelGGL(gae_scan_f32, dim3((B + 255) / 256), dim3(256), 0,
                     cur_stream(), rewards.data_ptr<float>(),
                     values.data_ptr<float>(), cont.data_ptr<float>(),
                     adv.data_ptr<float>(), vt.data_ptr<float>(), T, B,
                     (float)gamma, (float)lam);
  return {adv, vt};
}

std::vector<at::Tensor> vtrace(at::Tensor log_rhos, at::Tensor rewards,
                               at::Tensor values, at::Tensor cont,
                               double gamma, double rho_clip, double c_clip,
                               double rho_pg_clip) {
  CHECK_IN(log_rhos); CHECK_IN(rewards); CHECK_IN(values); CHECK_IN(cont);
  int T = (int)rewards.size(0);
  int B = (int)rewards.size(1);
  auto vs = at::empty_like(rewards);
  auto pg = at::empty_like(rewards);
  hipLaunchKernelGGL(vtrace_scan_f32, dim3((B + 255) / 256), dim3(256), 0,
                     cur_stream(), log_rhos.data_ptr<float>(),
                     rewards.data_ptr<float>(), values.data_ptr<float>(),
                     cont.data_ptr<float>(), vs.data_ptr<float>(),
                     pg.data_ptr<float>(), T, B, (float)gamma,
                     (float)rho_clip, (float)c_clip, (float)rho_pg_clip);
  return {vs, pg};
}

// ---------------- image normalize ----------------

at::Tensor img_normalize(at::Tensor in, at::Tensor mean, at::Tensor inv_std) {
  CHECK_IN(in); CHECK_IN(mean); CHECK_IN(inv_std);
  TORCH_CHECK(in.scalar_type() == at::kByte && in.dim() == 4);
  long long N = in.size(0);
  int H = (int)in.size(1), W = (int)in.size(2), C = (int)in.size(3);
  auto out = at::empty({N, C, H, W}, in.options().dtype(at::kBFloat16));
  long long total = in.numel();
  hipLaunchKernelGGL(img_norm_u8_bf16, dim3(grid_for(total)), dim3(256), 0,
                     cur_stream(), in.data_ptr<unsigned char>(),
                     (short*)out.data_ptr(), mean.data_ptr<float>(),
                     inv_std.data_ptr<float>(), N, H, W, C);
  return out;
}

// ---------------- cross entropy ----------------

static void ce_check(const at::Tensor& logits, const at::Tensor& target) {
  CHECK_IN(logits); CHECK_IN(target);
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16, "ce: logits must be bf16");
  TORCH_CHECK(target.scalar_type() == at::kInt, "ce: target must be int32");
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) >= 1 &&
              logits.size(1) < (1ll << 31), "ce: logits must be [N, V]");
  TORCH_CHECK(target.dim() == 1 && target.size(0) == logits.size(0),
              "ce: target must be [N]");
  // the kernels use 16-byte loads only when V % 8 == 0; then every row
  // is aligned exactly when the base is
  TORCH_CHECK(logits.size(1) % 8 != 0 || aligned16(logits),
              "ce: logits must be 16-byte aligned");
}

std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor target) {
  ce_check(logits, target);
  long long N = logits.size(0);
  int V = (int)logits.size(1);
  auto loss = at::empty({N}, logits.options().dtype(at::kFloat));
  auto mx = at::empty({N}, logits.options().dtype(at::kFloat));
  auto lse = at::empty({N}, logits.options().dtype(at::kFloat));
  hipLaunchKernelGGL(ce_fwd_bf16, dim3((unsigned)N), dim3(256), 0,
                     cur_stream(), (const short*)logits.data_ptr(),
                     target.data_ptr<int>(), loss.data_ptr<float>(),
                     mx.data_ptr<float>(), lse.data_ptr<float>(), N, V);
  return {loss, mx, lse};
}

at::Tensor ce_bwd(at::Tensor logits, at::Tensor target, at::Tensor mx,
                  at::Tensor lse, at::Tensor dloss) {
  ce_check(logits, target);
  CHECK_IN(mx); CHECK_IN(lse); CHECK_IN(dloss);
  long long N = logits.size(0);
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.numel() == N &&
              dloss.scalar_type() == at::kFloat && dloss.numel() == N,
              "ce: lse and dloss must be fp32 [N]");
  int V = (int)logits.size(1);
  auto dl = at::empty_like(logits);
  hipLaunchKernelGGL(ce_bwd_bf16, dim3((unsigned)N), dim3(256), 0,
                     cur_stream(), (const short*)logits.data_ptr(),
                     target.data_ptr<int>(), mx.data_ptr<float>(),
                     lse.data_ptr<float>(), dloss.data_ptr<float>(),
                     (short*)dl.data_ptr(), N, V);
  return dl;
}


// Layout of a [B,H,T,D] tensor: 0 = contiguous BHTD; 1 = a transpose view
// of token-row storage, strides (T*rs, D, rs, 1): [B,T,H,D] storage (the
// model's natural layout, rs = H*D) or a column section of a wider row,
// such as the q, k or v part of one packed [B,T,(Hq+2Hkv)*D] GEMM output
// (rs > H*D, then rs % 8 == 0, a 16-byte-aligned start and offsets that fit
// the kernels' 32-bit staging arithmetic are required); -1 = other.
// *rs is the token-row stride in elements (D for layout 0).
static inline int attn_layout(const at::Tensor& t, long long* rs) {
  if (t.stride(3) != 1) return -1;
  long long H = t.size(1), T = t.size(2), D = t.size(3);
  *rs = D;
  if (t.stride(2) == D && t.stride(1) == T * D && t.stride(0) == H * T * D)
    return 0;
  const long long r = t.stride(2);
  if (t.stride(1) != D || t.stride(0) != T * r || r < H * D) return -1;
  *rs = r;
  if (r == H * D) return 1;
  if (r % 8 == 0 && aligned16(t) && T * r < (1ll << 31) &&
      64 * r < (1ll << 30))
    return 1;
  return -1;
}

std::vector<at::Tensor> flash_attn_fwd(at::Tensor q, at::Tensor k,
                                        at::Tensor v, bool causal,
                                        int64_t q_offset, bool want_lse) {
  TORCH_CHECK(q.is_cuda() && k.is_cuda() && v.is_cuda(),
              "flash_attn tensors must be on GPU");
  long long q_rs, k_rs, v_rs;
  int bthd = attn_layout(q, &q_rs);
  TORCH_CHECK(bthd >= 0 && attn_layout(k, &k_rs) == bthd &&
                  attn_layout(v, &v_rs) == bthd && k_rs == v_rs,
              "q/k/v must share a BHTD-contiguous or BTHD-view layout");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16, "q must be bf16");
  TORCH_CHECK(q.size(3) == 128, "head_dim must be 128");
  TORCH_CHECK(q.size(2) % 128 == 0, "T must be a multiple of 128 (pad)");
  int B = (int)q.size(0), Hq = (int)q.size(1), T = (int)q.size(2);
  int Hkv = (int)k.size(1), Tk = (int)k.size(2);
  TORCH_CHECK(Hq % Hkv == 0, "GQA requires Hq % Hkv == 0");
  TORCH_CHECK(!bthd || T % 256 == 0,
              "BTHD-view layout needs T % 256 == 0: only the 256-row "
              "kernel reads it");
  // O matches q's layout so the model's out.transpose().reshape stays
  // a free view
  auto o = bthd
               ? at::empty({B, T, Hq, (int)q.size(3)}, q.options())
                     .permute({0, 2, 1, 3})
               : at::empty_like(q);
  const long long o_rs = bthd ? (long long)Hq * q.size(3) : q.size(3);
  at::Tensor lse;
  float* lse_ptr = nullptr;
  if (want_lse) {
    lse = at::empty({B, Hq, T}, q.options().dtype(at::kFloat));
    lse_ptr = lse.data_ptr<float>();
  }
  float scale = 1.0f / sqrtf((float)q.size(3));
  const short* qp = (const short*)q.data_ptr();
  const short* kp = (const short*)k.data_ptr();
  const short* vp = (const short*)v.data_ptr();
  short* op = (short*)o.data_ptr();
  const int c = causal ? 1 : 0, qo = (int)q_offset;
  if (T % 256 == 0)
    // 256 query rows per block: 8 waves on the two-phase ping-pong schedule
    hipLaunchKernelGGL(flash_attn_fwd_v7_bf16, dim3(T / 256, B * Hq),
                       dim3(512), 0, cur_stream(), qp, kp, vp, op, lse_ptr,
                       B, Hq, Hkv, T, Tk, c, qo, scale, bthd, (int)q_rs,
                       (int)o_rs, (int)k_rs);
  else
    hipLaunchKernelGGL(flash_attn_fwd_v5_bf16, dim3(T / 128, B * Hq),
                       dim3(256), 0, cur_stream(), qp, kp, vp, op, lse_ptr,
                       B, Hq, Hkv, T, Tk, c, qo, scale);
  if (want_lse) return {o, lse};
  return {o};
}

// `dqkv`, when given, is a packed gradient buffer [B, T, (Hq+2Hkv)*D] (unit
// column stride, 16-byte-aligned rows): dq, dk and dv are written into its
// three column sections and returned as views of it. It needs the BTHD-view
// layout (only the 256-row kernels write through a row stride).
std::vector<at::Tensor> flash_attn_bwd(at::Tensor q, at::Tensor k,
                                        at::Tensor v, at::Tensor o,
                                        at::Tensor d_o, at::Tensor lse,
                                        bool causal,
                                        c10::optional<at::Tensor> dqkv) {
  TORCH_CHECK(q.is_cuda(), "flash_attn_bwd tensors must be on GPU");
  long long q_rs, k_rs, v_rs, o_rs, do_rs;
  int bthd = attn_layout(q, &q_rs);
  TORCH_CHECK(bthd >= 0 && attn_layout(k, &k_rs) == bthd &&
                  attn_layout(v, &v_rs) == bthd &&
                  attn_layout(o, &o_rs) == bthd &&
                  attn_layout(d_o, &do_rs) == bthd && k_rs == v_rs,
              "q/k/v/o/dO must share a BHTD or BTHD-view layout");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16, "q must be bf16");
  TORCH_CHECK(q.size(3) == 128, "head_dim must be 128");
  TORCH_CHECK(q.size(2) % 128 == 0, "T must be a multiple of 128");
  TORCH_CHECK(q.size(2) == k.size(2),
              "bwd requires T == Tk (training self-attention)");
  int B = (int)q.size(0), Hq = (int)q.size(1), T = (int)q.size(2);
  int Hkv = (int)k.size(1);
  TORCH_CHECK(Hq % Hkv == 0, "GQA requires Hq % Hkv == 0");
  TORCH_CHECK(!bthd || T % 256 == 0,
              "BTHD-view layout needs T % 256 == 0: only the 256-row "
              "kernels read it");
  int D = (int)q.size(3);
  // fa_bwd_prep reads o and dO as plain [B,T,Hq,D] rows
  TORCH_CHECK(!bthd || (o_rs == (long long)Hq * D && do_rs == o_rs),
              "o and dO must be [B,T,Hq,D] storage in the BTHD-view layout");
  at::Tensor dq, dk, dv;
  long long dq_rs = q_rs, dkv_rs = k_rs;
  if (dqkv.has_value()) {
    const at::Tensor& g = *dqkv;
    const long long W = (long long)(Hq + 2 * Hkv) * D;
    TORCH_CHECK(bthd == 1, "dqkv needs q/k/v in the BTHD-view layout");
    TORCH_CHECK(g.is_cuda() && g.scalar_type() == at::kBFloat16 &&
                    g.dim() == 3 && g.size(0) == B && g.size(1) == T &&
                    g.size(2) == W,
                "dqkv must be bf16 [B, T, (Hq+2Hkv)*D] on the GPU");
    const long long r = g.stride(1);
    TORCH_CHECK(g.stride(2) == 1 && g.stride(0) == T * r && r >= W &&
                    r % 8 == 0 && aligned16(g) && T * r < (1ll << 31) &&
                    64 * r < (1ll << 30),
                "dqkv rows must be 16-byte aligned, at stride >= "
                "(Hq+2Hkv)*D with T * stride < 2^31");
    auto section = [&](long long col, int H) {
      return g.narrow(2, col, (long long)H * D)
          .view({B, T, H, D})
          .permute({0, 2, 1, 3});
    };
    dq = section(0, Hq);
    dk = section((long long)Hq * D, Hkv);
    dv = section((long long)(Hq + Hkv) * D, Hkv);
    dq_rs = dkv_rs = r;
  } else {
    auto mk_like = [&](const at::Tensor& t, int H) {
      return bthd
                 ? at::empty({B, T, H, D}, t.options()).permute({0, 2, 1, 3})
                 : at::empty_like(t);
    };
    dq = mk_like(q, Hq);
    dk = mk_like(k, Hkv);
    dv = mk_like(v, Hkv);
    if (bthd) {
      dq_rs = (long long)Hq * D;
      dkv_rs = (long long)Hkv * D;
    }
  }
  auto dsum = at::empty({B, Hq, T}, q.options().dtype(at::kFloat));
  float scale = 1.0f / sqrtf((float)q.size(3));
  long long rows = (long long)B * Hq * T;
  const short* qp = (const short*)q.data_ptr();
  const short* kp = (const short*)k.data_ptr();
  const short* vp = (const short*)v.data_ptr();
  const short* dop = (const short*)d_o.data_ptr();
  const float* lsep = lse.data_ptr<float>();
  float* dsp = dsum.data_ptr<float>();
  short* dqp = (short*)dq.data_ptr();
  short* dkp = (short*)dk.data_ptr();
  short* dvp = (short*)dv.data_ptr();
  const int c = causal ? 1 : 0;
  hipStream_t st = cur_stream();
  hipLaunchKernelGGL(fa_bwd_prep_bf16, dim3((rows + 3) / 4), dim3(256), 0,
                     st, dop, (const short*)o.data_ptr(), dsp, rows, Hq, T,
                     bthd);
  if (T % 256 == 0) {
    // 256-row blocks, either layout. dq: 64-row K/V tiles, split (issue
    // early / write late) staging. dkv: key on the MFMA lane, so P and dS
    // feed the dV^T / dK^T products from registers; its grid has the key
    // block as the slow dimension (heaviest causal block first).
    hipLaunchKernelGGL(fa_bwd_dq_v5_bf16, dim3(T / 256, B * Hq), dim3(512),
                       0, st, qp, kp, vp, dop, lsep, dsp, dqp, B, Hq, Hkv, T,
                       c, scale, bthd, (int)q_rs, (int)o_rs, (int)k_rs,
                       (int)dq_rs);
    hipLaunchKernelGGL(fa_bwd_dkv_v6_bf16, dim3(B * Hkv, T / 256), dim3(512),
                       0, st, qp, kp, vp, dop, lsep, dsp, dkp, dvp, B, Hq,
                       Hkv, T, c, scale, bthd, (int)q_rs, (int)o_rs, (int)k_rs,
                       (int)dkv_rs);
  } else {
    // 128-row blocks, contiguous BHTD only (checked above): K/V
    // register-resident, 64-row double-buffered q/dO tiles; dV and dK are
    // two instances of fa_bwd_dkv_v3_bf16 so that each fits 2 waves/SIMD.
    const dim3 blk(256);
    hipLaunchKernelGGL(fa_bwd_dq_v3_bf16, dim3(T / 128, B * Hq), blk, 0, st,
                       qp, kp, vp, dop, lsep, dsp, dqp, B, Hq, Hkv, T, c,
                       scale, /*bthd=*/0);
    hipLaunchKernelGGL(fa_bwd_dkv_v3_bf16<false>, dim3(T / 128, B * Hkv), blk,
                       0, st, qp, kp, vp, dop, lsep, dsp, dvp, B, Hq, Hkv, T,
                       c, scale);
    hipLaunchKernelGGL(fa_bwd_dkv_v3_bf16<true>, dim3(T / 128, B * Hkv), blk,
                       0, st, qp, kp, vp, dop, lsep, dsp, dkp, B, Hq, Hkv, T,
                       c, scale);
  }
  return {dq, dk, dv};
}

// In-place RoPE of the q and k sections of a packed [B, T, rs-strided] QKV
// buffer whose rows begin with Hq q heads, then Hkv k heads, then v.
void rope_qk_inplace(at::Tensor qkv, at::Tensor cosT, at::Tensor sinT,
                     int64_t n_heads, int64_t n_kv_heads, int64_t sign) {
  CHECK_IN(cosT); CHECK_IN(sinT);
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 &&
                  qkv.dim() == 3,
              "rope_qk_inplace: qkv must be a bf16 [B, T, W] GPU tensor");
  TORCH_CHECK(sign == 1 || sign == -1, "rope_qk_inplace: sign must be +-1");
  TORCH_CHECK(n_heads >= 1 && n_kv_heads >= 1 &&
                  qkv.size(2) % (n_heads + 2 * n_kv_heads) == 0,
              "rope_qk_inplace: W must be (Hq + 2 Hkv) * D");
  const long long B = qkv.size(0), T = qkv.size(1), W = qkv.size(2);
  const int D = (int)(W / (n_heads + 2 * n_kv_heads));
  const long long rs = qkv.stride(1);
  TORCH_CHECK(D > 0 && D % 16 == 0, "rope_qk_inplace: D must be a multiple "
                                    "of 16");
  TORCH_CHECK(qkv.stride(2) == 1 && rs >= W && rs % 8 == 0 &&
                  (B == 1 || qkv.stride(0) == T * rs) && aligned16(qkv),
              "rope_qk_inplace: rows must be 16-byte aligned with a uniform "
              "stride >= W");
  TORCH_CHECK(cosT.scalar_type() == at::kFloat &&
                  sinT.scalar_type() == at::kFloat && cosT.dim() == 2 &&
                  cosT.size(0) >= T && cosT.size(1) == D / 2 &&
                  sinT.sizes() == cosT.sizes() && aligned16(cosT) &&
                  aligned16(sinT),
              "rope_qk_inplace: cosT/sinT must be 16-byte-aligned fp32 "
              "[>= T, D/2]");
  const int n_rot = (int)(n_heads + n_kv_heads);
  const long long total = B * T * n_rot * (D / 16);
  if (total == 0) return;
  hipLaunchKernelGGL(rope_qk_inplace_bf16, dim3(grid_for(total)), dim3(256), 0,
                     cur_stream(), (short*)qkv.data_ptr(),
                     cosT.data_ptr<float>(), sinT.data_ptr<float>(), B * T, D,
                     n_rot, (int)T, (int)sign, rs);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("flash_attn_fwd", &flash_attn_fwd);
  m.def("flash_attn_bwd", &flash_attn_bwd, py::arg("q"), py::arg("k"),
        py::arg("v"), py::arg("o"), py::arg("d_o"), py::arg("lse"),
        py::arg("causal"), py::arg("dqkv") = py::none());
  m.def("rope_qk_inplace", &rope_qk_inplace);
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("gemv", &gemv);
  m.def("gemm_wgrad", &gemm_wgrad, py::arg("dy"), py::arg("x"),
        py::arg("out") = py::none());
  m.def("gemm_wgrad_grouped", &gemm_wgrad_grouped);
  m.def("paged_attn_decode", &paged_attn_decode, py::arg("q"),
        py::arg("k_cache"), py::arg("v_cache"), py::arg("block_table"),
        py::arg("seq_lens"), py::arg("num_splits"),
        py::arg("workspace") = py::none(), py::arg("k_scale") = 1.0,
        py::arg("v_scale") = 1.0);
  m.def("paged_attn_reduce", &paged_attn_reduce);
  m.def("rope_append_paged", &rope_append_paged, py::arg("q"), py::arg("k"),
        py::arg("v"), py::arg("cosT"), py::arg("sinT"), py::arg("pos"),
        py::arg("block_table"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("k_scale") = 1.0, py::arg("v_scale") = 1.0);
  m.def("kv_append_paged", &kv_append_paged);
  m.def("paged_attn_prefill", &paged_attn_prefill, py::arg("q"),
        py::arg("k_cache"), py::arg("v_cache"), py::arg("block_table"),
        py::arg("ctx_lens"), py::arg("q_lens"), py::arg("k_scale") = 1.0,
        py::arg("v_scale") = 1.0);
  m.def("rmsnorm_bwd", &rmsnorm_bwd);
  m.def("rmsnorm_bwd_two_pass", &rmsnorm_bwd_two_pass);
  m.def("rmsnorm_bwd_res", &rmsnorm_bwd_res, py::arg("dy"), py::arg("x"),
        py::arg("w"), py::arg("inv"), py::arg("g_res") = py::none(),
        py::arg("grid") = 0);
  m.def("add_rmsnorm_fwd", &add_rmsnorm_fwd);
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("rope_apply", &rope_apply);
  m.def("adamw_step", &adamw_step);
  m.def("gae", &gae);
  m.def("vtrace", &vtrace);
  m.def("img_normalize", &img_normalize);
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_bwd", &ce_bwd);
  m.attr("gfx_arch") = "gfx950";
  // the largest grid of the one-pass RMSNorm backward (tests size N by it)
  m.attr("rmsnorm_bwd_grid") = RMS_BWD_GRID;
}
