"""FP8 and MXFP4 weight-only decode linears (csrc/hip/linear_w8.hip,
csrc/hip/linear_w4.hip) against the best bf16 path for the same shape
(ops.linear_sb: the GEMV kernel or hipBLASLt), alternated in one process, on
the five Llama-3-8B decode shapes.

    python tools/linear_w8_bench.py [--rows 1,2,4,8,16,32] [--iters 50]
                                    [--tiles 0] [--w4 0:0]

Each repetition times --iters back-to-back calls between two device
events; a row shows the median of 7 repetitions with [min, max], in µs per
call, and the weight-byte rate: N*K bytes for fp8, 2*N*K for bf16 and
N*K*17/32 for mxfp4 (the bytes the algorithm must read; x, y and the fp8
scales are left out). An mxfp4 row also shows x-bytes per weight byte, the
L2 traffic its tile costs: 4 * 16*ceil(M/16) / tile. The
bound of this operation is bytes: at 8 TB/s of HBM the least time is
weight bytes / 8e12. --tiles adds rows for a forced 16- or 32-channel
block tile (0 is the shape rule of csrc/ops.hip); --w4 adds mxfp4 rows for
forced tile:split pairs, comma-separated (tile 64 or 128, split 1, 2, 4, 8;
0:0 is the launcher's rule).

    python tools/linear_w8_bench.py --gemm [--rows 64,128,256,512,1024,2048]
                                    [--iters 20] [--split 0] [--rows-tile 0]
                                    [--models llama3-8b,llama3-1b]
                                    [--weights fp8|mxfp4]

--gemm measures the W8A16 GEMM for 33+ rows (csrc/hip/linear_w8_gemm.hip) on
the projection shapes of --models, three paths alternated the same way:
"fallback" is what ops.linear_w8 does for a shape that _W8_GEMM_TABLE does
not list (dequantise to bf16, then F.linear) and is the admission
yardstick; "gemm" is the kernel (--split and --rows-tile add rows for forced
values, 0 is the launcher's rule); "bf16" is F.linear on a resident bf16
weight, the price of not using fp8 at all, for information. All three are
rated on N*K weight bytes. It ends with the peak extra memory of one lm_head
call at 64 rows on the fallback and on the kernel. --weights mxfp4 measures
the W4A16 GEMM (csrc/hip/linear_w4_gemm.hip) the same way: the fallback is
what ops.linear_w4 does for a shape that _W4_GEMM_TABLE does not list
(ops._K.dequant_mxfp4, then F.linear), and the rate is on N*K*17/32 bytes.
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


def alternate(paths, iters):
    """Sorted times of REPS alternated repetitions for each (label, fn)."""
    for _, fn in paths:  # warm up this shape on each path
        timed(fn, 5)
    times = [[] for _ in paths]
    for _ in range(REPS):
        for ts, (_, fn) in zip(times, paths):
            ts.append(timed(fn, iters))
    return [sorted(ts) for ts in times]


def model_shapes(names):
    """(label, N, K) of the distinct projection shapes of the configs."""
    from ray_amd.models.llama import CONFIGS

    out = []
    for name in names:
        c = CONFIGS[name]
        d = c.hidden_size // c.num_heads
        for label, N, K in [
                ("qkv", (c.num_heads + 2 * c.num_kv_heads) * d, c.hidden_size),
                ("o_proj", c.hidden_size, c.num_heads * d),
                ("gate/up", c.intermediate_size, c.hidden_size),
                ("down", c.hidden_size, c.intermediate_size),
                ("lm_head", c.vocab_size, c.hidden_size)]:
            if (N, K) not in [(n, k) for _, n, k in out]:
                out.append((f"{name[-2:]} {label}", N, K))
    return out


def fallback(x, wq, scale):
    return torch.nn.functional.linear(
        x, (wq.float() * scale[:, None]).to(x.dtype))


def fallback_w4(x, wq, scales):
    return torch.nn.functional.linear(x, ops._K.dequant_mxfp4(wq, scales))


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20, y


def main_gemm(args, dev):
    rows = [int(r) for r in (args.rows or "64,128,256,512,1024,2048").split(",")]
    forced = [(int(s), int(t)) for s in args.split.split(",")
              for t in args.rows_tile.split(",")]
    print(f"{'shape':>10} {'N':>6} {'K':>5} {'M':>4}  path           "
          f"median µs [min, max]         TB/s  of 8 TB/s")
    for name, N, K in model_shapes(args.models.split(",")):
        w = torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02
        if args.weights == "mxfp4":
            wq, scale = ops.quantize_weight_mxfp4(w)
            fb_fn, kernel, nbytes = fallback_w4, ops._K.linear_w4_gemm, \
                N * K * 17 // 32
        else:
            wq, scale = ops.quantize_weight_fp8(w)
            fb_fn, kernel, nbytes = fallback, ops._K.linear_w8_gemm, N * K
        for M in rows:
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            paths = [("fallback", lambda: fb_fn(x, wq, scale))]
            for sp, rt in forced:
                label = "gemm" + (f" s{sp}" if sp else "") + (
                    f" r{rt}" if rt else "")
                paths.append((label, lambda sp=sp, rt=rt: kernel(
                    x, wq, scale, sp, rt)))
            paths.append(("bf16", lambda: torch.nn.functional.linear(x, w)))
            times = alternate(paths, args.iters)
            for ts, (label, _) in zip(times, paths):
                rate = nbytes / (ts[REPS // 2] * 1e-6)
                print(f"{name:>10} {N:6d} {K:5d} {M:4d}  {label:<13}  "
                      f"{ts[REPS // 2]:9.2f} [{ts[0]:9.2f}, {ts[-1]:9.2f}]  "
                      f"{rate / 1e12:5.2f}  {100 * rate / HBM_PEAK:5.1f}%")
            for ts, (label, _) in zip(times[1:-1], paths[1:-1]):
                print(f"{'':>10} {label} slowest "
                      f"{'<' if ts[-1] < times[0][0] else '>='} fallback "
                      f"fastest: {ts[-1]:.2f} vs {times[0][0]:.2f} µs")
        if name.endswith("lm_head"):
            x = torch.randn(64, K, device=dev, dtype=torch.bfloat16)
            fb, _ = peak_extra(lambda: fb_fn(x, wq, scale))
            kn, _ = peak_extra(lambda: kernel(x, wq, scale))
            print(f"{name:>10} peak extra memory of one call at M = 64: "
                  f"fallback {fb:.1f} MiB, gemm {kn:.1f} MiB "
                  f"(y itself is {64 * N * 2 / 2 ** 20:.1f} MiB)")
        del w, wq, scale


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=None)
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--tiles", default="0")
    ap.add_argument("--w4", default="0:0")
    ap.add_argument("--gemm", action="store_true")
    ap.add_argument("--split", default="0")
    ap.add_argument("--rows-tile", default="0")
    ap.add_argument("--models", default="llama3-8b,llama3-1b")
    ap.add_argument("--weights", default="fp8", choices=["fp8", "mxfp4"])
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.HAVE_HIP_OPS, "needs the GPU"
    if args.gemm:
        args.iters = args.iters or 20
        torch.manual_seed(0)
        with torch.no_grad():
            return main_gemm(args, torch.device("cuda", 0))
    args.rows = args.rows or "1,2,4,8,16,32"
    args.iters = args.iters or 50
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    tiles = [int(t) for t in args.tiles.split(",")]
    w4s = [tuple(int(v) for v in p.split(":")) for p in args.w4.split(",")]
    print(f"{'shape':>8} {'N':>6} {'K':>5} {'M':>2}  path       "
          f"median µs [min, max]       TB/s  of 8 TB/s")
    with torch.no_grad():
        for name, N, K in SHAPES:
            w = torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02
            wq, scale = ops.quantize_weight_fp8(w)
            w4, s4 = ops.quantize_weight_mxfp4(w)
            for M in [int(r) for r in args.rows.split(",")]:
                x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
                paths = [("bf16", 2 * N * K, lambda: ops.linear_sb(x, w))]
                for t in tiles:
                    paths.append((
                        "fp8" if t == 0 else f"fp8 t{t}", N * K,
                        lambda t=t: ops._K.linear_w8(x, wq, scale, t)))
                for t, sp in w4s:
                    tile = t or 128  # the launcher's default
                    paths.append((
                        "mxfp4" + (f" t{t}s{sp}" if t or sp else ""),
                        N * K * 17 // 32,
                        lambda t=t, sp=sp: ops._K.linear_w4(x, w4, s4, t, sp),
                        4 * 16 * ((M + 15) // 16) / tile))
                for _, _, fn, *_ in paths:  # warm up this shape on each path
                    timed(fn, 10)
                times = [[] for _ in paths]
                for _ in range(REPS):  # alternate the paths
                    for ts, (_, _, fn, *_) in zip(times, paths):
                        ts.append(timed(fn, args.iters))
                for ts, (label, nbytes, _, *xr) in zip(times, paths):
                    ts.sort()
                    med = ts[REPS // 2]
                    rate = nbytes / (med * 1e-6)
                    print(f"{name:>8} {N:6d} {K:5d} {M:2d}  {label:<9}  "
                          f"{med:8.2f} [{ts[0]:8.2f}, {ts[-1]:8.2f}]  "
                          f"{rate / 1e12:5.2f}  {100 * rate / HBM_PEAK:5.1f}%"
                          + (f"  x/w {xr[0]:.2f}" if xr else ""))
                fp8, bf = times[1], times[0]
                print(f"{'':>8} fp8 slowest {'<' if fp8[-1] < bf[0] else '>='}"
                      f" bf16 fastest: {fp8[-1]:.2f} vs {bf[0]:.2f} µs")
                for ts, (label, *_) in zip(times[len(tiles) + 1:],
                                           paths[len(tiles) + 1:]):
                    print(f"{'':>8} {label} slowest "
                          f"{'<' if ts[-1] < fp8[0] else '>='} fp8 fastest: "
                          f"{ts[-1]:.2f} vs {fp8[0]:.2f} µs")


if __name__ == "__main__":
    main()
