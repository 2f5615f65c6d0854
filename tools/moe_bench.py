"""Mixture-of-experts FFN (csrc/hip/moe.hip) against the torch composition
that ops.moe_ffn sends large M to (per expert: index_select, three bf16
hipBLASLt GEMMs, index_add_; it reads the routing on the host), alternated in
one process on the Mixtral-8x7B shapes (H 4096, I 14336, E 8, top 2).

    python tools/moe_bench.py [--rows 1,4,16,64,256,1024,4096] [--iters 20]

Each repetition times --iters back-to-back calls between two device events;
a row shows the median of 7 repetitions with [min, max], in µs per call, for
the four kernel launches after the router (align, gate/up, down, combine),
the router launch alone and the composition on the same routing. "GB/s" is
the bytes of the distinct experts the rows chose (3 * H * I * 2 each) over
the kernels' time: the rate at which decode reads its weights.

    python tools/moe_bench.py --step [--batches 1,8,32] [--layers 4]
                              [--iters 20]

--step times the graph-captured PagedDecoder step of mixtral-8x7b cut to
--layers layers (random weights) at context 512, in ms per step. Run it under
`rocprofv3 --kernel-trace --stats` for the MoE kernels' share.
"""
import argparse
import dataclasses
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from ray_amd import ops

H, I, E, K = 4096, 14336, 8, 2
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
    for _, fn in paths:
        timed(fn, 3)
    times = [[] for _ in paths]
    for _ in range(REPS):
        for ts, (_, fn) in zip(times, paths):
            ts.append(timed(fn, iters))
    return [sorted(ts) for ts in times]


def main_op(args, dev):
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape, fan_in):
        return (torch.randn(*shape, generator=g, device=dev)
                * fan_in ** -0.5).bfloat16()

    Wr, Wg, Wu = rnd(E, H, fan_in=H), rnd(E, I, H, fan_in=H), rnd(E, I, H,
                                                                  fan_in=H)
    Wd = rnd(E, H, I, fan_in=I)
    m = REPS // 2
    print(f"H={H} I={I} E={E} top {K}; µs per call, median [min, max]")
    print(f"{'M':>5} {'experts':>7} {'route':>8} {'kernels':>28} {'GB/s':>7} "
          f"{'composition':>28} {'ratio':>6}")
    for M in [int(r) for r in args.rows.split(",")]:
        x = torch.randn(M, H, generator=g, device=dev).bfloat16()
        idx, w, lists = ops.moe_route(x, Wr, K, with_lists=True)
        used = idx.unique().numel()
        y = ops.moe_experts(x, idx, w, Wg, Wu, Wd)
        yc = ops._moe_compose(x, idx, w, Wg, Wu, Wd, None)
        rel = ((y.float() - yc.float()).norm() / yc.float().norm()).item()
        iters = max(3, args.iters // max(1, M // 256))
        r, kern, comp = alternate([
            ("route", lambda: ops.moe_route(x, Wr, K)),
            ("kernels", lambda: ops.moe_experts(x, idx, w, Wg, Wu, Wd)),
            ("composition",
             lambda: ops._moe_compose(x, idx, w, Wg, Wu, Wd, None))], iters)
        gbs = used * 3 * H * I * 2 / (kern[m] * 1e-6) / 1e9
        print(f"{M:5d} {used:7d} {r[m]:8.1f} {kern[m]:10.1f} [{kern[0]:7.1f},"
              f"{kern[-1]:8.1f}] {gbs:7.0f} {comp[m]:10.1f} [{comp[0]:7.1f},"
              f"{comp[-1]:8.1f}] {comp[m] / kern[m]:5.2f}x  "
              f"(rel. difference {rel:.1e})", flush=True)


def main_step(args, dev):
    from ray_amd.llm.paged import PagedDecoder
    from ray_amd.models.llama import CONFIGS, LlamaModel

    torch.manual_seed(0)
    cfg = dataclasses.replace(CONFIGS["mixtral-8x7b"], num_layers=args.layers)
    with torch.device(dev):
        model = LlamaModel(cfg).eval()
    model.cosT, model.sinT = model.cosT.to(dev), model.sinT.to(dev)
    ctx = 512
    m = REPS // 2
    print(f"mixtral-8x7b, {args.layers} layers, context {ctx}; ms per "
          "captured step, median [min, max]")
    for B in [int(b) for b in args.batches.split(",")]:
        dec = PagedDecoder(model, B, ctx + 64, dev)
        for slot in range(B):
            dec.reserve_slot(slot, ctx + 64)
        dec.seq_lens.fill_(ctx + 1)
        dec.capture()
        tok = torch.arange(B, device=dev) * 37 % cfg.vocab_size
        pos = torch.full((B,), ctx, device=dev)
        ts = alternate([("step", lambda: dec.decode(tok, pos))],
                       args.iters)[0]
        print(f"B={B:3d} {ts[m] / 1e3:8.3f} [{ts[0] / 1e3:.3f}, "
              f"{ts[-1] / 1e3:.3f}]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,4,16,64,256,1024,4096")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--layers", type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.HAVE_HIP_OPS
    dev = torch.device("cuda", 0)
    with torch.no_grad():
        (main_step if args.step else main_op)(args, dev)


if __name__ == "__main__":
    main()
