"""FP8 weight-only decode linear (csrc/hip/linear_w8.hip) against the best
bf16 path for the same shape (ops.linear_sb: the GEMV kernel or hipBLASLt),
alternated in one process, on the five Llama-3-8B decode shapes.

    python tools/linear_w8_bench.py [--rows 1,2,4,8,16,32] [--iters 50]
                                    [--tiles 0]

Each repetition times --iters back-to-back calls between two device
events; a row shows the median of 7 repetitions with [min, max], in µs per
call, and the weight-byte rate: N*K bytes for fp8, 2*N*K for bf16 (the
bytes the algorithm must read; x, y and the scales are left out). The
bound of this operation is bytes: at 8 TB/s of HBM the least time is
weight bytes / 8e12. --tiles adds rows for a forced 16- or 32-channel
block tile (0 is the shape rule of csrc/ops.hip).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from ray_amd import ops

SHAPES = [("qkv", 6144, 4096), ("o_proj", 4096, 4096),
          ("gate/up", 14336, 4096), ("down", 4096, 14336),
          ("lm_head", 128256, 4096)]
HBM_PEAK = 8e12  # bytes/s
REPS = 7


def timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters  # µs per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,2,4,8,16,32")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--tiles", default="0")
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.HAVE_HIP_OPS, "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    tiles = [int(t) for t in args.tiles.split(",")]
    print(f"{'shape':>8} {'N':>6} {'K':>5} {'M':>2}  path       "
          f"median µs [min, max]       TB/s  of 8 TB/s")
    with torch.no_grad():
        for name, N, K in SHAPES:
            w = torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02
            wq, scale = ops.quantize_weight_fp8(w)
            for M in [int(r) for r in args.rows.split(",")]:
                x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
                paths = [("bf16", 2 * N * K, lambda: ops.linear_sb(x, w))]
                for t in tiles:
                    paths.append((
                        "fp8" if t == 0 else f"fp8 t{t}", N * K,
                        lambda t=t: ops._K.linear_w8(x, wq, scale, t)))
                for _, _, fn in paths:  # warm up this shape on each path
                    timed(fn, 10)
                times = [[] for _ in paths]
                for _ in range(REPS):  # alternate the paths
                    for ts, (_, _, fn) in zip(times, paths):
                        ts.append(timed(fn, args.iters))
                for ts, (label, nbytes, _) in zip(times, paths):
                    ts.sort()
                    med = ts[REPS // 2]
                    rate = nbytes / (med * 1e-6)
                    print(f"{name:>8} {N:6d} {K:5d} {M:2d}  {label:<9}  "
                          f"{med:8.2f} [{ts[0]:8.2f}, {ts[-1]:8.2f}]  "
                          f"{rate / 1e12:5.2f}  {100 * rate / HBM_PEAK:5.1f}%")
                fp8, bf = times[1], times[0]
                print(f"{'':>8} fp8 slowest {'<' if fp8[-1] < bf[0] else '>='}"
                      f" bf16 fastest: {fp8[-1]:.2f} vs {bf[0]:.2f} µs")


if __name__ == "__main__":
    main()
