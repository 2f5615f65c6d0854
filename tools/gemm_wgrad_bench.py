"""A/B of the hand-written weight-gradient GEMM against torch's
`dy.t() @ x` at the flagship step's six weight shapes (M = 32768 tokens).

Both sides run in one process on the same standard-normal operands,
interleaved repetition by repetition. Per side: median / min / max over
REPS repetitions of CALLS back-to-back calls, and PF/s at the median.
A shape belongs in ops._WGRAD_TABLE only if the kernel's slowest
repetition beats torch's fastest (last column).

Standalone runs ride the boost clock; these numbers pick the dispatch
table, they are not the step result.

    python tools/gemm_wgrad_bench.py [--m 32768] [--reps 7] [--calls 20]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ray_amd import ops  # noqa: E402

# gate, up and down first: three quarters of the family's time
SHAPES = [
    ("gate/up", 14336, 4096, 1),
    ("down", 4096, 14336, 1),
    ("gate+up grouped", 14336, 4096, 2),
    ("o_proj", 4096, 4096, 1),
    ("qkv", 6144, 4096, 1),
    ("lm_head", 128256, 4096, 1),
]


def _time(fn, calls):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only", default=None, help="substring of a shape name")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_wgrad_bench needs a GPU")
    dev = torch.device("cuda")
    M = args.m
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    print(f"M={M} reps={args.reps} calls/rep={args.calls}  (ms per call: "
          "median [min, max], PF/s at median)")
    for name, N, K, groups in SHAPES:
        if args.only and args.only not in name:
            continue
        calls = max(2, args.calls // 8) if N > 100000 else args.calls
        dys = [torch.randn((M, N), generator=gen, device=dev,
                           dtype=torch.bfloat16) for _ in range(groups)]
        x = torch.randn((M, K), generator=gen, device=dev,
                        dtype=torch.bfloat16)
        if groups == 1:
            ours = lambda: ops.gemm_wgrad(dys[0], x)  # noqa: E731
            ref = lambda: dys[0].t() @ x  # noqa: E731
        else:
            ours = lambda: ops.gemm_wgrad_grouped(dys[0], dys[1], x)  # noqa: E731
            ref = lambda: [d.t() @ x for d in dys]  # noqa: E731
        for _ in range(3):
            ours()
            ref()
        torch.cuda.synchronize()
        t_ours, t_ref = [], []
        for _ in range(args.reps):
            t_ours.append(_time(ours, calls))
            t_ref.append(_time(ref, calls))
        flop = 2.0 * M * N * K * groups

        def fmt(ts):
            med = statistics.median(ts)
            return (f"{med:8.3f} [{min(ts):8.3f}, {max(ts):8.3f}] "
                    f"{flop / med / 1e12:5.3f} PF/s")

        wins = max(t_ours) < min(t_ref)
        print(f"{name:16s} N={N:6d} K={K:5d} x{groups}  ours {fmt(t_ours)}"
              f"  torch {fmt(t_ref)}  table={'yes' if wins else 'no'}",
              flush=True)
        del dys, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
