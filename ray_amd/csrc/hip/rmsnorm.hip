// Fused RMSNorm forward/backward for CDNA4 (gfx950).
//
// Memory-bound: bf16 loads vectorized as short8 (16 B/lane — guide G13),
// one 256-thread block per row, wave+LDS reduction, fp32 math.
// Replaces the separate pow/mean/rsqrt/mul chain torch would launch
// (the reference delegates all GPU math to torch — SURVEY.md §2.9).
#include "common.h"

// y[n,h] = x[n,h] * rsqrt(mean_h(x^2)+eps) * w[h]; saves inv_rms[n].
extern "C" __global__ __launch_bounds__(256) void rmsnorm_fwd_bf16(
    const short* __restrict__ x, const short* __restrict__ w,
    short* __restrict__ y, float* __restrict__ inv_rms, int H, float eps) {
  long long row = blockIdx.x;
  const short* xr = x + row * (long long)H;
  short* yr = y + row * (long long)H;
  __shared__ float lds[8];

  float acc = 0.f;
  int base = threadIdx.x * 8;
  int stride = blockDim.x * 8;
  for (int i = base; i < H; i += stride) {
    short8 v = *reinterpret_cast<const short8*>(xr + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf2f(v[j]);
      acc += f * f;
    }
  }
  float ssq = block_sum<256>(acc, lds);
  float inv = rsqrtf(ssq / (float)H + eps);
  if (threadIdx.x == 0) inv_rms[row] = inv;

  for (int i = base; i < H; i += stride) {
    short8 v = *reinterpret_cast<const short8*>(xr + i);
    short8 wv = *reinterpret_cast<const short8*>(w + i);
    short8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(bf2f(v[j]) * inv * bf2f(wv[j]));
    *reinterpret_cast<short8*>(yr + i) = o;
  }
}

// dx[n,h] = inv*(dy*w) - x[n,h]*inv^3/H * sum_h(dy*w*x)
extern "C" __global__ __launch_bounds__(256) void rmsnorm_bwd_dx_bf16(
    const short* __restrict__ dy, const short* __restrict__ x,
    const short* __restrict__ w, const float* __restrict__ inv_rms,
    short* __restrict__ dx, int H) {
  long long row = blockIdx.x;
  const short* dyr = dy + row * (long long)H;
  const short* xr = x + row * (long long)H;
  short* dxr = dx + row * (long long)H;
  float inv = inv_rms[row];
  __shared__ float lds[8];

  float dot = 0.f;
  int base = threadIdx.x * 8;
  int stride = blockDim.x * 8;
  for (int i = base; i < H; i += stride) {
    short8 dv = *reinterpret_cast<const short8*>(dyr + i);
    short8 xv = *reinterpret_cast<const short8*>(xr + i);
    short8 wv = *reinterpret_cast<const short8*>(w + i);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      dot += bf2f(dv[j]) * bf2f(wv[j]) * bf2f(xv[j]);
  }
  dot = block_sum<256>(dot, lds);
  float k = dot * inv * inv * inv / (float)H;

  for (int i = base; i < H; i += stride) {
    short8 dv = *reinterpret_cast<const short8*>(dyr + i);
    short8 xv = *reinterpret_cast<const short8*>(xr + i);
    short8 wv = *reinterpret_cast<const short8*>(w + i);
    short8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = f2bf(bf2f(dv[j]) * bf2f(wv[j]) * inv - bf2f(xv[j]) * k);
    *reinterpret_cast<short8*>(dxr + i) = o;
  }
}

// dw[h] = sum_n dy[n,h] * x[n,h] * inv_rms[n]
// Column-tile kernel: each block owns 256 columns; loop over rows with
// coalesced loads (thread t reads column col0+t). fp32 output.
// Grid: (ceil(H/256), ROW_SPLITS). Each block reduces its row-range for
// its 256-column tile, then one atomicAdd per column (device-scope,
// guide G12). dw must be zeroed by the caller.
extern "C" __global__ __launch_bounds__(256) void rmsnorm_bwd_dw_bf16(
    const short* __restrict__ dy, const short* __restrict__ x,
    const float* __restrict__ inv_rms, float* __restrict__ dw,
    long long N, int H) {
  int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= H) return;
  long long chunk = (N + gridDim.y - 1) / gridDim.y;
  long long n0 = blockIdx.y * chunk;
  long long n1 = min(n0 + chunk, N);
  float acc = 0.f;
  for (long long n = n0; n < n1; ++n) {
    long long idx = n * H + col;
    acc += bf2f(dy[idx]) * bf2f(x[idx]) * inv_rms[n];
  }
  if (gridDim.y == 1)
    dw[col] = acc;
  else
    atomicAdd(dw + col, acc);
}

// ---------------------------------------------------------------------
// One-pass backward and fused residual-add forward.
//
// A 256-thread block covers a row in chunks of 2048 columns; thread t owns
// columns 2048c + 8t .. + 7 of chunk c and keeps them in registers, so dy
// and x are read once. The per-thread sums run in the same order as the
// kernels above (chunk, then element), and the element expressions are the
// same, so y, inv and dx keep their bits.
// ---------------------------------------------------------------------

#define RMS_CHUNK 2048
// blocks of the one-pass backward: each walks rows blockIdx.x, +grid, ...
// and leaves one fp32 [H] partial of dw. 1024 blocks are 4 per CU; the
// partial image is 2*1024/N of the dy bytes (6.25 % at N = 32768).
#define RMS_BWD_GRID 1024
// a block takes at least this many rows when there are few (one block, one
// sequential fma chain per column, for N <= 4: then dw has the bits of the
// two-pass kernel, whose single row split adds the rows in that order)
#define RMS_BWD_MIN_ROWS 4

// dx (optionally + g_res, rounded as a bf16 add of the two tensors) and
// per-block dw partials part[gridDim.x][H].
template <int CHUNKS, bool RES>
__global__ __launch_bounds__(256) void rmsnorm_bwd_onepass_bf16(
    const short* __restrict__ dy, const short* __restrict__ x,
    const short* __restrict__ w, const float* __restrict__ inv_rms,
    const short* __restrict__ g_res, short* __restrict__ dx,
    float* __restrict__ part, long long N, int H) {
  __shared__ float lds[8];
  const int col0 = threadIdx.x * 8;
  short8 wv[CHUNKS];
  float acc[CHUNKS][8];
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const int col = c * RMS_CHUNK + col0;
    wv[c] = short8{0, 0, 0, 0, 0, 0, 0, 0};
    if (col < H) wv[c] = *reinterpret_cast<const short8*>(w + col);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[c][j] = 0.f;
  }

  for (long long row = blockIdx.x; row < N; row += gridDim.x) {
    const long long ro = row * (long long)H;
    const float inv = inv_rms[row];
    short8 dv[CHUNKS], xv[CHUNKS];
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      const int col = c * RMS_CHUNK + col0;
      dv[c] = short8{0, 0, 0, 0, 0, 0, 0, 0};
      xv[c] = short8{0, 0, 0, 0, 0, 0, 0, 0};
      if (col < H) {
        dv[c] = *reinterpret_cast<const short8*>(dy + ro + col);
        xv[c] = *reinterpret_cast<const short8*>(x + ro + col);
      }
    }
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c)
      if (c * RMS_CHUNK + col0 < H) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          dot += bf2f(dv[c][j]) * bf2f(wv[c][j]) * bf2f(xv[c][j]);
      }
    dot = block_sum<256>(dot, lds);
    const float k = dot * inv * inv * inv / (float)H;

#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      const int col = c * RMS_CHUNK + col0;
      if (col < H) {
        short8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          o[j] = f2bf(bf2f(dv[c][j]) * bf2f(wv[c][j]) * inv -
                      bf2f(xv[c][j]) * k);
          acc[c][j] += bf2f(dv[c][j]) * bf2f(xv[c][j]) * inv;
        }
        if (RES) {
          const short8 g = *reinterpret_cast<const short8*>(g_res + ro + col);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = f2bf(bf2f(o[j]) + bf2f(g[j]));
        }
        *reinterpret_cast<short8*>(dx + ro + col) = o;
      }
    }
  }

  float* pr = part + (long long)blockIdx.x * H;
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const int col = c * RMS_CHUNK + col0;
    if (col < H) {
      *reinterpret_cast<float4v*>(pr + col) =
          float4v{acc[c][0], acc[c][1], acc[c][2], acc[c][3]};
      *reinterpret_cast<float4v*>(pr + col + 4) =
          float4v{acc[c][4], acc[c][5], acc[c][6], acc[c][7]};
    }
  }
}

// dw[h] = sum_g part[g][h] in a fixed order: a block owns 32 columns,
// thread (ry, cx) adds rows ry + 8k into accumulator k % 4 (32 short
// chains per column instead of one long one: four loads in flight, and
// less rounding error), then the chains are added pairwise. No atomics, so
// two calls give the same bits.
extern "C" __global__ __launch_bounds__(256) void rmsnorm_dw_reduce_f32(
    const float* __restrict__ part, float* __restrict__ dw, int G, int H) {
  __shared__ float lds[8][32];
  const int cx = threadIdx.x & 31;
  const int ry = threadIdx.x >> 5;
  const int col = blockIdx.x * 32 + cx;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (col < H) {
    const float* p = part + col;
    int g = ry;
    for (; g + 24 < G; g += 32) {
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] += p[(long long)(g + 8 * k) * H];
    }
    // at most three rows are left
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (g + 8 * k < G) a[k] += p[(long long)(g + 8 * k) * H];
  }
  lds[ry][cx] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  if (ry == 0 && col < H)
    dw[col] = ((lds[0][cx] + lds[1][cx]) + (lds[2][cx] + lds[3][cx])) +
              ((lds[4][cx] + lds[5][cx]) + (lds[6][cx] + lds[7][cx]));
}

// s = bf16(x + r); h = s * rsqrt(mean(s^2) + eps) * w, from the rounded s;
// saves inv_rms. One block per row, s held in registers.
template <int CHUNKS>
__global__ __launch_bounds__(256) void add_rmsnorm_fwd_bf16(
    const short* __restrict__ x, const short* __restrict__ r,
    const short* __restrict__ w, short* __restrict__ s_out,
    short* __restrict__ y, float* __restrict__ inv_rms, int H, float eps) {
  __shared__ float lds[8];
  const long long ro = (long long)blockIdx.x * H;
  const int col0 = threadIdx.x * 8;
  short8 sv[CHUNKS];
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const int col = c * RMS_CHUNK + col0;
    if (col < H) {
      const short8 a = *reinterpret_cast<const short8*>(x + ro + col);
      const short8 b = *reinterpret_cast<const short8*>(r + ro + col);
#pragma unroll
      for (int j = 0; j < 8; ++j) sv[c][j] = f2bf(bf2f(a[j]) + bf2f(b[j]));
      *reinterpret_cast<short8*>(s_out + ro + col) = sv[c];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf2f(sv[c][j]);
        acc += f * f;
      }
    }
  }
  const float ssq = block_sum<256>(acc, lds);
  const float inv = rsqrtf(ssq / (float)H + eps);
  if (threadIdx.x == 0) inv_rms[blockIdx.x] = inv;
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const int col = c * RMS_CHUNK + col0;
    if (col < H) {
      const short8 wv = *reinterpret_cast<const short8*>(w + col);
      short8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = f2bf(bf2f(sv[c][j]) * inv * bf2f(wv[j]));
      *reinterpret_cast<short8*>(y + ro + col) = o;
    }
  }
}
