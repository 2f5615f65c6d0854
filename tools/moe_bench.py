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

    python tools/moe_bench.py --weights mxfp4 [--rows ...] [--split 0]

With MXFP4 expert weights (csrc/hip/moe_w4.hip) a row times the W4 kernels,
the bf16 kernels on the dequantised weights and the composition with its
per-expert dequantise, on the same routing in the same alternated
repetitions. "GB/s" counts 3 * H * I * 17/32 bytes per distinct expert.

    python tools/moe_bench.py --step [--batches 1,8,32] [--layers 4]
                              [--iters 20] [--weights mxfp4]

--step times the graph-captured PagedDecoder step of mixtral-8x7b cut to
--layers layers (random weights; --weights mxfp4 quantises projections and
experts as weight_dtype="mxfp4" does) at context 512, in ms per step. Run it
under `rocprofv3 --kernel-trace --stats` for the MoE kernels' share.
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


def main_op_w4(args, dev):
    """The W4 kernels, the bf16 kernels and the composition with per-expert
    dequantise on the same routing, alternated. The bf16 weights are the
    dequantised MXFP4 ones, so the two kernel paths compute the same FFN."""
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape, fan_in):
        return (torch.randn(*shape, generator=g, device=dev)
                * fan_in ** -0.5).bfloat16()

    def both(n, kk):
        wq, s = ops.quantize_expert_weights_mxfp4(rnd(E, n, kk, fan_in=kk))
        w = torch.stack([ops._K.dequant_mxfp4(wq[e], s[e]) for e in range(E)])
        return wq, s, w

    Wr = rnd(E, H, fan_in=H)
    (gq, gs, Wg), (uq, us, Wu), (dq, ds, Wd) = both(I, H), both(I, H), both(
        H, I)
    sc = (gs, us, ds)
    m = REPS // 2

    def fmt(ts):
        return f"{ts[m]:9.1f} [{ts[0]:7.1f},{ts[-1]:8.1f}]"

    print(f"H={H} I={I} E={E} top {K}, MXFP4 expert weights, split "
          f"{args.split}; µs per call, median [min, max]")
    print(f"{'M':>5} {'experts':>7} {'w4 kernels':>27} {'GB/s':>6} "
          f"{'bf16 kernels':>27} {'bf16/w4':>7} {'w4 slowest < bf16 fastest'}"
          f" {'composition + dequantise':>27} {'comp/w4':>7}")
    for M in [int(r) for r in args.rows.split(",")]:
        x = torch.randn(M, H, generator=g, device=dev).bfloat16()
        idx, w, lists = ops.moe_route(x, Wr, K, with_lists=True)
        used = idx.unique().numel()

        def w4():
            return ops.moe_experts(x, idx, w, gq, uq, dq, lists=lists,
                                   scales=sc, split=args.split)

        def bf():
            return ops.moe_experts(x, idx, w, Wg, Wu, Wd, lists=lists)

        def comp():
            return ops._moe_compose(x, idx, w, gq, uq, dq, None, sc)

        y, yb = w4().float(), bf().float()
        rel = ((y - yb).norm() / yb.norm()).item()
        iters = max(3, args.iters // max(1, M // 256))
        t4, tb, tc = alternate([("w4", w4), ("bf16", bf), ("comp", comp)],
                               iters)
        gbs = used * 3 * H * I * 17 / 32 / (t4[m] * 1e-6) / 1e9
        print(f"{M:5d} {used:7d} {fmt(t4)} {gbs:6.0f} {fmt(tb)} "
              f"{tb[m] / t4[m]:6.2f}x {str(t4[-1] < tb[0]):>25} {fmt(tc)} "
              f"{tc[m] / t4[m]:6.2f}x  (w4 - bf16: {rel:.1e} of the norm; "
              f"keeps kernels: {t4[-1] < tc[0]})", flush=True)


def main_step(args, dev):
    from ray_amd.llm.paged import PagedDecoder
    from ray_amd.models.llama import CONFIGS, LlamaModel

    torch.manual_seed(0)
    cfg = dataclasses.replace(CONFIGS["mixtral-8x7b"], num_layers=args.layers)
    with torch.device(dev):
        model = LlamaModel(cfg).eval()
    model.cosT, model.sinT = model.cosT.to(dev), model.sinT.to(dev)
    if args.weights == "mxfp4":  # what the engine does for weight_dtype
        from ray_amd.models.llama import (quantize_experts_mxfp4,
                                          quantize_linears_mxfp4)
        quantize_experts_mxfp4(quantize_linears_mxfp4(model))
    ctx = 512
    m = REPS // 2
    print(f"mixtral-8x7b, {args.layers} layers, weights {args.weights}, "
          f"context {ctx}; ms per captured step, median [min, max]")
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
    ap.add_argument("--weights", choices=("bf16", "mxfp4"), default="bf16")
    ap.add_argument("--split", type=int, default=0,
                    help="mxfp4: K slices of the down kernel (0: the rule)")
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.HAVE_HIP_OPS
    dev = torch.device("cuda", 0)
    with torch.no_grad():
        if args.step:
            main_step(args, dev)
        elif args.weights == "mxfp4":
            main_op_w4(args, dev)
        else:
            main_op(args, dev)


if __name__ == "__main__":
    main()
