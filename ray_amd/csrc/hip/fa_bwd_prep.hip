// Flash-attention backward, first kernel of both paths (algorithm: Dao
// 2023 §3): Dsum[b,h,q] = sum_d dO[q][d] * O[q][d] (fp32), the row
// constant the dQ and dK kernels subtract from dP.
#include "fa_bwd_frag.h"

extern "C" __global__ __launch_bounds__(256) void fa_bwd_prep_bf16(
    const short* __restrict__ dO, const short* __restrict__ O,
    float* __restrict__ Dsum, long long total_rows, int Hq, int T,
    int bthd) {
  // Dsum is ALWAYS [B,Hq,T]-indexed; when O/dO storage is [B,T,H,D]
  // the storage row (b,t,h) maps to dsum index (b*Hq+h)*T + t.
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= total_rows) return;
  const int lane = threadIdx.x & 63;
  const short* dop = dO + row * FB3_D + 2 * lane;
  const short* op = O + row * FB3_D + 2 * lane;
  float acc = bf2f(dop[0]) * bf2f(op[0]) + bf2f(dop[1]) * bf2f(op[1]);
  acc = wave_sum(acc);
  if (lane == 0) {
    long long idx = row;
    if (bthd) {
      long long b = row / ((long long)T * Hq);
      long long rem = row % ((long long)T * Hq);
      long long t = rem / Hq, h = rem % Hq;
      idx = (b * Hq + h) * T + t;
    }
    Dsum[idx] = acc;
  }
}
