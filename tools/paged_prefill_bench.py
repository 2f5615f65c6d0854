"""Paged prefill attention: (a) the kernel alone against the composite
the code had before it (gather the pages to contiguous K/V, then
ops.flash_attention with q_offset), and (b) PagedDecoder.prefill_slot
for a shared prefix plus a tail, cold and warm.

    python tools/paged_prefill_bench.py [--shapes 3072:1024,0:4096]
        [--model llama3-8b] [--prefix 2048] [--tail 128] [--skip-model]
        [--kv-dtype bf16,fp8]

(a) reports median [min, max] microseconds per call over --reps timed
repetitions of --iters back-to-back calls after warm-up, and the
achieved rate on the causal FLOPs 4*Hq*D*(visible q-k pairs).
(b) reports median [min, max] milliseconds per prefill_slot call over
--reps prompts; every prompt has a fresh random prefix, prefilled once
cold and once more (with another tail) warm.
With --kv-dtype fp8 the kernel rows run on an fp8 cache (the composite
reads the dequantised values as bf16, which is exact), and the model
rows are cold and warm prefill into an fp8 pool.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from ray_amd import ops


def time_us(fn, iters, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


def bench_kernel(args, dev, kv_dtype):
    Hq, Hkv, D = args.hq, args.hkv, args.d
    page = ops.PAGE_SIZE
    tag = "" if kv_dtype == "bf16" else f" kv_dtype={kv_dtype}"
    print(f"# (a) kernel: Hq={Hq} Hkv={Hkv} D={D} B=1 iters={args.iters} "
          f"reps={args.reps}{tag}; us per call: median [min, max]")
    for spec in args.shapes.split(","):
        ctx, Tq = (int(x) for x in spec.split(":"))
        L = ctx + Tq
        n_pages = -(-L // page)
        num_pages = n_pages + 1
        torch.manual_seed(0)
        kc = torch.randn(num_pages, Hkv, page, D, device=dev,
                         dtype=torch.bfloat16)
        vc = torch.randn_like(kc)
        if kv_dtype == "fp8":
            kc, vc = ops.quantize_kv_fp8(kc), ops.quantize_kv_fp8(vc)
        # shuffled page assignment, as a long-running pool would have
        bt = (torch.randperm(num_pages - 1) + 1).to(torch.int32).view(
            1, n_pages).to(dev)
        q = torch.randn(1, Tq, Hq, D, device=dev, dtype=torch.bfloat16)
        cl = torch.tensor([ctx], dtype=torch.int32, device=dev)
        ql = torch.tensor([Tq], dtype=torch.int32, device=dev)
        pages = bt[0].long()

        def paged():
            return ops.paged_attention_prefill(q, kc, vc, bt, cl, ql)

        def composite():
            # [P,Hkv,page,D] -> [1,L,Hkv,D] storage read as [1,Hkv,L,D]:
            # the layout flash_attention takes without another copy
            k = kc[pages].permute(0, 2, 1, 3).reshape(1, -1, Hkv, D)[:, :L]
            v = vc[pages].permute(0, 2, 1, 3).reshape(1, -1, Hkv, D)[:, :L]
            if kv_dtype == "fp8":
                k, v = k.to(torch.bfloat16), v.to(torch.bfloat16)
            o = ops.flash_attention(q.transpose(1, 2), k.transpose(1, 2),
                                    v.transpose(1, 2), causal=True,
                                    q_offset=ctx)
            return o.transpose(1, 2)

        err = float((paged().float() - composite().float()).abs().max())
        p_med, p_min, p_max = time_us(paged, args.iters, args.reps)
        c_med, c_min, c_max = time_us(composite, args.iters, args.reps)
        pairs = Tq * ctx + Tq * (Tq + 1) // 2
        tflops = 4.0 * Hq * D * pairs / (p_med * 1e-6) / 1e12
        print(f"ctx={ctx:5d} Tq={Tq:5d}  "
              f"paged {p_med:8.1f} [{p_min:8.1f},{p_max:8.1f}] us "
              f"{tflops:6.1f} TFLOP/s  "
              f"gather+flash {c_med:8.1f} [{c_min:8.1f},{c_max:8.1f}] us  "
              f"composite/paged {c_med / p_med:5.2f}x  "
              f"max|diff| {err:.2e}")
        del kc, vc


def bench_model_fp8(args, dev, model):
    """Cold and warm prefill_slot into an fp8 pool."""
    from ray_amd.llm.paged import PagedDecoder

    cfg = model.cfg
    n = args.prefix + args.tail
    print(f"# (b) {args.model} prefill_slot, kv_dtype=fp8: prefix "
          f"{args.prefix} + tail {args.tail} tokens, reps={args.reps}; ms "
          f"per call: median [min, max]")
    cached = PagedDecoder(model, 1, n + 64, dev, prefix_caching=True,
                          kv_dtype=torch.float8_e4m3fn)
    rows = {"cold": [], "warm": []}

    def once(prefix):
        tail = torch.randint(0, cfg.vocab_size, (args.tail,), device=dev)
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        cached.prefill_slot(0, torch.cat([prefix, tail]))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    with torch.no_grad():
        for rep in range(args.reps + 1):  # rep 0 warms both paths up
            prefix = torch.randint(0, cfg.vocab_size, (args.prefix,),
                                   device=dev)
            t = [once(prefix), once(prefix)]
            if rep:
                for ms, v in zip(rows.values(), t):
                    ms.append(v)
    for name, ms in rows.items():
        print(f"{name:32s} {statistics.median(ms):8.2f} [{min(ms):8.2f},"
              f"{max(ms):8.2f}] ms")


def bench_model(args, dev, kv_dtypes):
    from ray_amd.llm.paged import PagedDecoder
    from ray_amd.models.llama import CONFIGS, LlamaModel

    cfg = CONFIGS[args.model]
    torch.manual_seed(0)
    with torch.device(dev):
        model = LlamaModel(cfg, dtype=torch.bfloat16).eval()
    model.cosT = model.cosT.to(dev)
    model.sinT = model.sinT.to(dev)
    if "bf16" not in kv_dtypes:
        return bench_model_fp8(args, dev, model)
    n = args.prefix + args.tail
    max_T = n + 64
    print(f"# (b) {args.model} prefill_slot: prefix {args.prefix} + tail "
          f"{args.tail} tokens, reps={args.reps}; ms per call: "
          f"median [min, max]")

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def prompt(prefix):
        tail = torch.randint(0, cfg.vocab_size, (args.tail,), device=dev)
        return torch.cat([prefix, tail])

    def fmt(ms):
        return (f"{statistics.median(ms):8.2f} [{min(ms):8.2f},"
                f"{max(ms):8.2f}] ms")

    plain = PagedDecoder(model, 1, max_T, dev)
    cached = PagedDecoder(model, 1, max_T, dev, prefix_caching=True)
    chunked = PagedDecoder(model, 1, max_T, dev, prefix_caching=True,
                           prefill_chunk=args.chunk)
    rows = {"whole-prompt path (flags off)": [], "cold": [], "warm": [],
            f"cold, chunks of {args.chunk}": []}
    with torch.no_grad():
        for rep in range(args.reps + 1):  # rep 0 warms every path up
            prefix = torch.randint(0, cfg.vocab_size, (args.prefix,),
                                   device=dev)
            t = [
                timed(lambda: plain.prefill_slot(0, prompt(prefix))),
                timed(lambda: cached.prefill_slot(0, prompt(prefix))),
                timed(lambda: cached.prefill_slot(0, prompt(prefix))),
                timed(lambda: chunked.prefill_slot(0, prompt(prefix))),
            ]
            if rep:
                for ms, v in zip(rows.values(), t):
                    ms.append(v)
    hit = cached.prefix_hit_tokens
    want = (args.reps + 1) * (args.prefix // ops.PAGE_SIZE) * ops.PAGE_SIZE
    assert hit == want, (hit, want)
    for name, ms in rows.items():
        print(f"{name:32s} {fmt(ms)}")
    cold, warm = (statistics.median(rows[k]) for k in ("cold", "warm"))
    print(f"warm computes {n - args.prefix // 16 * 16} of {n} tokens: "
          f"cold/warm {cold / warm:5.2f}x")
    if "fp8" in kv_dtypes:
        del plain, cached, chunked
        bench_model_fp8(args, dev, model)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3072:1024,0:4096",
                    help="ctx:Tq pairs, comma-separated")
    ap.add_argument("--hq", type=int, default=32)
    ap.add_argument("--hkv", type=int, default=8)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--prefix", type=int, default=2048)
    ap.add_argument("--tail", type=int, default=128)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--kv-dtype", default="bf16",
                    help="comma-separated cache formats: bf16, fp8")
    args = ap.parse_args()
    kv_dtypes = args.kv_dtype.split(",")
    assert set(kv_dtypes) <= {"bf16", "fp8"}, kv_dtypes
    assert torch.cuda.is_available(), "paged_prefill_bench needs a GPU"
    dev = torch.device("cuda", 0)
    for kv_dtype in kv_dtypes:
        bench_kernel(args, dev, kv_dtype)
    if not args.skip_model:
        bench_model(args, dev, kv_dtypes)


if __name__ == "__main__":
    main()
