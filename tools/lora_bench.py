"""Batched per-row LoRA (csrc/hip/lora.hip) against the torch composition
that ops.lora_add falls back to (per adapter: index_select, two matmuls,
index_add_), alternated in one process, on the Llama-3-8B projection shapes.

    python tools/lora_bench.py [--rows 1,8,32,64,512] [--ranks 16,64]
                               [--iters 50] [--slots 64]

Each repetition times --iters back-to-back calls between two device events;
a row shows the median of 7 repetitions with [min, max], in µs per call. The
mixes are 1, 4 and M distinct adapters among the rows (capped at the slot
count for "M": --slots, 64 at most), rows dealt round-robin.

    python tools/lora_bench.py --step [--batches 1,8,32] [--iters 20]
                               [--model llama3-8b]

--step times the graph-captured PagedDecoder step of --model (random
weights) without adapter slots, then with 8 slots of rank 16 and all rows at
-1, one adapter in every row, and 8 distinct adapters (B of them when
B < 8), and prints the overhead over the step without slots in ms per step
and as a share of it.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from ray_amd import ops

SHAPES = [("qkv", 6144, 4096), ("o_proj", 4096, 4096),
          ("gate/up", 14336, 4096), ("down", 4096, 14336)]
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


def composition(y, x, A, B, scale, idx):
    """What a user runs without the kernels: bf16 matmuls per adapter. The
    .unique() is a device-to-host copy, as in any such loop."""
    for s in idx.unique().tolist():
        if s < 0:
            continue
        rows = (idx == s).nonzero().flatten()
        h = x.index_select(0, rows) @ A[s].t()
        y.index_add_(0, rows, (h @ B[s].t()) * scale[s].to(y.dtype))
    return y


def main_op(args, dev):
    rows = [int(r) for r in args.rows.split(",")]
    ranks = [int(r) for r in args.ranks.split(",")]
    S = args.slots
    print(f"{'shape':8} {'R':>3} {'M':>4} {'mix':>4}  "
          f"{'kernel µs [min, max]':>26}  {'torch µs [min, max]':>28}  ratio")
    for label, N, K in SHAPES:
        for R in ranks:
            A = torch.randn(S, R, K, device=dev).bfloat16()
            B = torch.randn(S, N, R, device=dev).bfloat16()
            scale = torch.ones(S, device=dev)
            for M in rows:
                x = torch.randn(M, K, device=dev).bfloat16()
                y = torch.zeros(M, N, device=dev).bfloat16()
                for mix in sorted({1, min(4, M, S), min(M, S)}):
                    idx = (torch.arange(M, device=dev) % mix).int()
                    paths = [
                        ("kernel", lambda: ops._K.lora_add(
                            y, x, A, B, scale, idx)),
                        ("torch", lambda: composition(
                            y, x, A, B, scale, idx)),
                    ]
                    iters = args.iters if M < 512 else max(5, args.iters // 5)
                    k, t = alternate(paths, iters)
                    m = REPS // 2
                    print(f"{label:8} {R:3d} {M:4d} {mix:4d}  "
                          f"{k[m]:8.1f} [{k[0]:6.1f},{k[-1]:7.1f}]  "
                          f"{t[m]:10.1f} [{t[0]:7.1f},{t[-1]:8.1f}]  "
                          f"{t[m] / k[m]:5.1f}x", flush=True)


def main_step(args, dev):
    from ray_amd.llm.paged import PagedDecoder
    from ray_amd.models.llama import CONFIGS, LlamaModel, add_lora_slots

    torch.manual_seed(0)
    cfg = CONFIGS[args.model]
    model = LlamaModel(cfg).to(dev).eval()
    model.cosT, model.sinT = model.cosT.to(dev), model.sinT.to(dev)
    batches = [int(b) for b in args.batches.split(",")]
    ctx = 512

    def step_ms(B, mixes):
        """Median [min, max] ms per captured step for each adapter mix."""
        dec = PagedDecoder(model, B, ctx + 64, dev)
        for slot in range(B):
            dec.reserve_slot(slot, ctx + 64)
        dec.seq_lens.fill_(ctx + 1)
        dec.capture()
        tok = torch.zeros(B, dtype=torch.long, device=dev)
        pos = torch.full((B,), ctx, device=dev)
        fns = []
        for mix in mixes:
            def fn(mix=mix):
                if mix is not None:
                    dec.slot_lora.copy_(mix)
                dec.decode(tok, pos)
            fns.append((str(mix), fn))
        return [[t / 1e3 for t in ts] for ts in alternate(fns, args.iters)]

    base = {B: step_ms(B, [None])[0] for B in batches}
    add_lora_slots(model, 8, 16)
    for mod in model.modules():
        if isinstance(mod, ops.LoraLinear):
            mod.lora_A.normal_(std=0.02)
            mod.lora_B.normal_(std=0.02)
            mod.lora_scale.fill_(1.0)
    m = REPS // 2
    print(f"{args.model}, context {ctx}, 8 slots of rank 16; ms per step, "
          f"median [min, max]")
    for B in batches:
        ar = torch.arange(B, device=dev)
        mixes = [torch.full((B,), -1, device=dev, dtype=torch.int32),
                 torch.zeros(B, device=dev, dtype=torch.int32),
                 (ar % 8).int()]
        rows = step_ms(B, mixes)
        b = base[B]
        print(f"B={B:3d} no slots        {b[m]:8.3f} [{b[0]:.3f}, {b[-1]:.3f}]")
        for name, ts in zip(("all rows -1", "1 adapter", f"{min(B, 8)} adapters"),
                            rows):
            over = ts[m] - b[m]
            print(f"B={B:3d} {name:15} {ts[m]:8.3f} [{ts[0]:.3f}, {ts[-1]:.3f}]"
                  f"  +{over:.3f} ms/step = +{over / B:.4f} ms/token, "
                  f"{100 * over / b[m]:.1f}% of the step", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,8,32,64,512")
    ap.add_argument("--ranks", default="16,64")
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--model", default="llama3-8b")
    args = ap.parse_args()
    if args.iters is None:
        args.iters = 20 if args.step else 50
    assert torch.cuda.is_available() and ops.HAVE_HIP_OPS
    dev = torch.device("cuda", 0)
    with torch.no_grad():
        (main_step if args.step else main_op)(args, dev)


if __name__ == "__main__":
    main()
