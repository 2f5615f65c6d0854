"""Split-KV verify attention (csrc/hip/paged_attn_verify.hip) against the
two ways to serve a verify step without it, on identical inputs and
alternated in one process: one ops.paged_attention_prefill call, and Tq
ops.paged_attention_decode calls (call i with seq_lens = ctx + i + 1).

    python tools/paged_verify_bench.py [--batches 1,4,16,64]
        [--ctx 512,4096,16384] [--tq 2,4,8] [--dtypes bf16,fp8] [--iters 20]

Shapes are llama3-8b's (Hq 32, Hkv 8, D 128). Each repetition times --iters
back-to-back calls between two device events; a row shows the median of 5
repetitions with [min, max] in µs per call, and the KV bytes the sequences
hold over the verify kernel's median time. Before timing, the three paths'
outputs are compared.

    python tools/paged_verify_bench.py --step [--batches 1,4,16,64]
        [--spec 3,7] [--step-ctx 4096] [--model llama3-8b]

--step times the graph-captured PagedDecoder.verify step of --model (random
weights, K + 1 rows per slot) against the captured single-token step of the
same decoder, and prints t_verify / t_single - 1: the mean number of
accepted draft tokens per step above which speculation is a net win.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from ray_amd import ops

HQ, HKV, D, PAGE = 32, 8, 128, 16
REPS = 5


def timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters  # µs per call


def alternate(fns, iters):
    """Sorted times of REPS alternated repetitions for each fn."""
    for fn in fns:
        timed(fn, 3)
    times = [[] for _ in fns]
    for _ in range(REPS):
        for ts, fn in zip(times, fns):
            ts.append(timed(fn, iters))
    return [sorted(ts) for ts in times]


def fmt(ts, p=1):
    return f"{ts[REPS // 2]:9.{p}f} [{ts[0]:8.{p}f},{ts[-1]:9.{p}f}]"


def main_kernel(args, dev):
    print(f"{'kv':>4} {'B':>3} {'ctx':>6} {'Tq':>2}  "
          f"{'verify µs [min, max]':>30} {'prefill µs [min, max]':>30} "
          f"{'Tq x decode µs [min, max]':>30}  prefill/verify decode/verify "
          f"verify TB/s max|diff|")
    for name in args.dtypes.split(","):
        dtype = torch.float8_e4m3fn if name == "fp8" else torch.bfloat16
        for B in args.batches:
            for ctx in args.ctx:
                pages = -(-(ctx + max(args.tq)) // PAGE)
                kc = torch.randn(B * pages + 1, HKV, PAGE, D,
                                 device=dev).to(dtype)
                vc = torch.randn(B * pages + 1, HKV, PAGE, D,
                                 device=dev).to(dtype)
                bt = (torch.randperm(B * pages, device=dev).int() + 1).view(
                    B, pages)
                for Tq in args.tq:
                    q = torch.randn(B, Tq, HQ, D, device=dev).bfloat16()
                    cl = torch.full((B,), ctx, dtype=torch.int32, device=dev)
                    ql = torch.full((B,), Tq, dtype=torch.int32, device=dev)
                    rows = [(q[:, i].contiguous(), cl + i + 1)
                            for i in range(Tq)]

                    def verify():
                        return ops.paged_attention_verify(q, kc, vc, bt, cl,
                                                          ql)

                    def prefill():
                        return ops.paged_attention_prefill(q, kc, vc, bt, cl,
                                                           ql)

                    def decode():
                        return [ops.paged_attention_decode(qi, kc, vc, bt, sl)
                                for qi, sl in rows]

                    out = verify().float()
                    err = max(float((out - other.float()).abs().max())
                              for other in (prefill(),
                                            torch.stack(decode(), 1)))
                    v, p, d = alternate([verify, prefill, decode], args.iters)
                    m = REPS // 2
                    kv_bytes = 2 * B * (ctx + Tq) * HKV * D * kc.element_size()
                    print(f"{name:>4} {B:3d} {ctx:6d} {Tq:2d}  {fmt(v)} "
                          f"{fmt(p)} {fmt(d)}  {p[m] / v[m]:14.2f} "
                          f"{d[m] / v[m]:13.2f} {kv_bytes / v[m] / 1e6:11.2f} "
                          f"{err:9.1e}", flush=True)
                del kc, vc


def main_step(args, dev):
    from ray_amd.llm.paged import PagedDecoder
    from ray_amd.models.llama import CONFIGS, LlamaModel

    torch.manual_seed(0)
    with torch.device(dev):
        model = LlamaModel(CONFIGS[args.model]).eval()
    model.cosT, model.sinT = model.cosT.to(dev), model.sinT.to(dev)
    ctx = args.step_ctx
    print(f"{args.model}, context {ctx}; captured steps, ms per step, median "
          f"[min, max]")
    for K in args.spec:
        for B in args.batches:
            dec = PagedDecoder(model, B, ctx + 64, dev, spec_tokens=K)
            for slot in range(B):
                dec.reserve_slot(slot, ctx + 64)
            dec.seq_lens.fill_(ctx + 1)
            dec.capture()
            tok = torch.zeros(B, dtype=torch.long, device=dev)
            pos = torch.full((B,), ctx, device=dev)
            toks = torch.zeros(B, K + 1, dtype=torch.long, device=dev)
            cl = torch.full((B,), ctx, dtype=torch.int32, device=dev)
            ql = torch.full((B,), K + 1, dtype=torch.int32, device=dev)
            one, ver = alternate([lambda: dec.decode(tok, pos),
                                  lambda: dec.verify(toks, cl, ql)],
                                 args.iters)
            m = REPS // 2
            print(f"K={K} B={B:3d}  single {fmt([t / 1e3 for t in one], 3)}  "
                  f"verify {fmt([t / 1e3 for t in ver], 3)}  break-even "
                  f"{ver[m] / one[m] - 1:.3f} accepted tokens/step",
                  flush=True)
            del dec


def ints(s):
    return [int(x) for x in s.split(",")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=ints, default=[1, 4, 16, 64])
    ap.add_argument("--ctx", type=ints, default=[512, 4096, 16384])
    ap.add_argument("--tq", type=ints, default=[2, 4, 8])
    ap.add_argument("--dtypes", default="bf16,fp8")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--spec", type=ints, default=[3, 7])
    ap.add_argument("--step-ctx", type=int, default=4096)
    ap.add_argument("--model", default="llama3-8b")
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.HAVE_HIP_OPS
    dev = torch.device("cuda", 0)
    with torch.no_grad():
        (main_step if args.step else main_kernel)(args, dev)


if __name__ == "__main__":
    main()
