"""Batched sampling: ops.sample against the per-row loop and a batched torch
top-p, and ContinuousBatchingEngine.step() with device_sampling off / on.

  python tools/sample_bench.py            # table (a), the op alone
  python tools/sample_bench.py --engine   # table (b), engine steps

Device events around each call (a) or a host clock around step(), which ends
in its own device-to-host copy (b); warm-up first; the paths of one row of a
table alternate in one process; median of 7 with [min, max]. A path "wins"
when its slowest repetition is below the other's fastest. Needs a GPU.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from ray_amd import ops

REPS = 7
V = 128256
SETS = [("greedy", 0.0, 0, 1.0), ("T0.8", 0.8, 0, 1.0),
        ("T0.8 k50", 0.8, 50, 1.0), ("T0.8 p0.9", 0.8, 0, 0.9)]


def fmt(ts):
    return f"{statistics.median(ts):8.1f} [{min(ts):7.1f}, {max(ts):7.1f}]"


def row_loop(logits, T, k, p):
    """What the engine does today, per slot: argmax or softmax +
    multinomial, each ending in .item(). It has no top-k / top-p."""
    out = []
    for r in range(logits.shape[0]):
        if T <= 0:
            out.append(int(logits[r].argmax(-1).item()))
        else:
            probs = torch.softmax(logits[r].float() / T, dim=-1)
            out.append(int(torch.multinomial(probs, 1).item()))
    return out


def torch_batched(logits, T, k, p, u):
    """The same rules as one batch of torch ops, with a full sort."""
    if T <= 0:
        return logits.argmax(-1)
    xs, order = torch.sort(logits.float(), dim=-1, descending=True)
    w = torch.exp((xs - xs[:, :1]) / T)
    if k > 0:
        w = torch.where(xs >= xs[:, k - 1 : k], w, 0.0)
    if p < 1:
        c = torch.cumsum(w, -1)
        first = (c >= p * c[:, -1:]).int().argmax(-1, keepdim=True)
        w = torch.where(xs >= xs.gather(1, first), w, 0.0)
    # back to index order for the inverse CDF
    w = torch.zeros_like(w).scatter_(1, order, w)
    c = torch.cumsum(w, -1)
    return (c > u[:, None] * c[:, -1:]).int().argmax(-1)


def timed(fn):
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def bench_op():
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    print(f"(a) ops.sample, V = {V}, bf16; us per call, median of {REPS} "
          "[min, max]")
    print(f"{'B':>3} {'set':<10} {'kernel':>26} {'per-row loop':>26} "
          f"{'torch sort':>26}  kernel wins over loop / sort")
    for B in (1, 8, 32, 64):
        logits = (torch.randn(B, V, generator=g) * 4).bfloat16().to(dev)
        u = torch.rand(B, generator=g).to(dev)
        for name, T, k, p in SETS:
            Tt = torch.full((B,), T, device=dev)
            kt = torch.full((B,), k, dtype=torch.int32, device=dev)
            pt = torch.full((B,), p, device=dev)
            paths = [lambda: ops.sample(logits, Tt, kt, pt, u),
                     lambda: row_loop(logits, T, k, p),
                     lambda: torch_batched(logits, T, k, p, u)]
            for fn in paths:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            ts = [[] for _ in paths]
            for _ in range(REPS):
                for i, fn in enumerate(paths):
                    ts[i].append(timed(fn))
            wins = " / ".join("yes" if max(ts[0]) < min(t) else "no"
                              for t in ts[1:])
            print(f"{B:>3} {name:<10} {fmt(ts[0])} {fmt(ts[1])} "
                  f"{fmt(ts[2])}  {wins}")


def engine_steps(eng, B, T, p, steps):
    """Fill every slot, then time `steps` decode steps one by one."""
    for i in range(B):
        eng.submit([7 + i, 11, 13, 17], max_new_tokens=256, temperature=T,
                   top_p=p)
    for _ in range(4):
        eng.step()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.step()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def bench_engine(model_id, steps):
    from ray_amd.llm import ContinuousBatchingEngine, LLMConfig

    print(f"(b) ContinuousBatchingEngine.step(), {model_id}, paged, fp8 "
          f"weights; ms per step (median of {steps} steps), median of "
          f"{REPS} [min, max]")
    print(f"{'B':>3} {'set':<10} {'device_sampling off':>26} "
          f"{'device_sampling on':>26}  gap ms  on wins")
    for B in (1, 8, 32):
        # top_p 0.9 off the device goes through ops.sample per row, since
        # the host path has no top-p; T 0.8 alone is the multinomial loop
        for name, T, p in (("greedy", 0.0, None), ("T0.8", 0.8, None),
                           ("T0.8 p0.9", 0.8, 0.9)):
            ts = [[], []]
            for rep in range(REPS + 1):  # the first repetition warms up
                for i, on in enumerate((False, True)):
                    eng = ENGINES.get((B, on))
                    if eng is None:
                        eng = ENGINES[(B, on)] = ContinuousBatchingEngine(
                            LLMConfig(model_id=model_id, max_seq_len=512,
                                      max_batch_size=B, kv_cache="paged",
                                      weight_dtype="fp8",
                                      device_sampling=on))
                    # drop what the last measurement left in the slots
                    eng._queue.clear()
                    for s in range(eng.B):
                        if eng._slots[s] is not None:
                            eng._retire(s)
                    eng._finished.clear()
                    t = engine_steps(eng, B, T, p, steps)
                    if rep:
                        ts[i].append(t)
            gap = statistics.median(ts[0]) - statistics.median(ts[1])
            print(f"{B:>3} {name:<10} {fmt(ts[0])} {fmt(ts[1])}  "
                  f"{gap:6.3f}  {'yes' if max(ts[1]) < min(ts[0]) else 'no'}")
        ENGINES.clear()


ENGINES: dict = {}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sample_bench needs a GPU"
    if args.engine:
        bench_engine(args.model, args.steps)
    else:
        bench_op()
