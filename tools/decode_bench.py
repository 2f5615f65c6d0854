"""Serving decode throughput: llama3-8b bf16, hipGraph-captured decode
(GraphedDecoder) vs eager, across batch sizes.

    python tools/decode_bench.py [--model llama3-8b] [--tokens 128]
                                 [--ctx N[,N...]] [--paged] [--reps R]
                                 [--kv-dtype bf16,fp8]

--ctx N starts decoding at context length N (default 64, i.e. tokens
64..72+tokens); --paged adds a row per batch for the graph-captured
PagedDecoder (paged KV cache + fused decode attention) at the same
positions, once per --kv-dtype (fp8: one-byte OCP e4m3fn pages).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from ray_amd.models.llama import CONFIGS, GraphedDecoder, LlamaModel


def bench(dec, cfg, B, n_tokens, prefill=64):
    dev = dec.device
    tok = torch.randint(0, cfg.vocab_size, (B,), device=dev)
    for p in range(prefill, prefill + 8):  # warmup
        logits = dec.decode(tok, p)
        tok = logits.argmax(-1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p in range(prefill + 8, prefill + 8 + n_tokens):
        logits = dec.decode(tok, p)
        tok = logits.argmax(-1)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench_paged(dec, cfg, B, n_tokens, prefill=64):
    """Same loop as bench() for a PagedDecoder whose slots all sit at
    the same position."""
    dev = dec.device
    tok = torch.randint(0, cfg.vocab_size, (B,), device=dev)
    pos = torch.zeros(B, dtype=torch.long, device=dev)

    def step(p):
        dec.seq_lens.fill_(p + 1)
        pos.fill_(p)
        return dec.decode(tok, pos).argmax(-1)

    for p in range(prefill, prefill + 8):  # warmup
        tok = step(p)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p in range(prefill + 8, prefill + 8 + n_tokens):
        tok = step(p)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--ctx", default="64",
                    help="context length(s) at which decoding starts, "
                         "comma-separated")
    ap.add_argument("--paged", action="store_true",
                    help="also time the captured PagedDecoder")
    ap.add_argument("--reps", type=int, default=1,
                    help="timed repetitions of each captured row; the row "
                         "shows the median and [min, max] ms/step")
    ap.add_argument("--kv-dtype", default="bf16",
                    help="--paged cache formats, comma-separated: bf16, fp8")
    args = ap.parse_args()
    kv_dtypes = args.kv_dtype.split(",")
    assert set(kv_dtypes) <= {"bf16", "fp8"}, kv_dtypes

    dev = torch.device("cuda", 0)
    cfg = CONFIGS[args.model]
    torch.manual_seed(0)
    model = LlamaModel(cfg, dtype=torch.bfloat16).to(dev).eval()
    model.cosT = model.cosT.to(dev)
    model.sinT = model.sinT.to(dev)

    def timed(fn):
        ms = sorted(fn() / args.tokens * 1e3 for _ in range(args.reps))
        med = ms[len(ms) // 2]
        spread = f" [{ms[0]:.2f}, {ms[-1]:.2f}]" if args.reps > 1 else ""
        return med, spread

    for ctx in [int(c) for c in args.ctx.split(",")]:
        max_T = max(512, ctx + 8 + args.tokens + 8)
        if args.ctx != "64":
            print(f"# ctx {ctx} (max_T {max_T})")
        for B in [int(b) for b in args.batches.split(",")]:
            dec = GraphedDecoder(model, B, max_T, dev)
            n_eager = max(args.tokens // 4, 16)
            dt_eager = bench(dec, cfg, B, n_eager, ctx)
            dec.capture()
            ms, spread = timed(lambda: bench(dec, cfg, B, args.tokens, ctx))
            print(f"batch {B:3d}: hipGraph {B / ms * 1e3:9.1f} tok/s "
                  f"({ms:6.2f} ms/step{spread})   "
                  f"eager {B * n_eager / dt_eager:9.1f} tok/s "
                  f"({dt_eager / n_eager * 1e3:6.2f} ms/step)")
            del dec
            if not args.paged:
                continue
            from ray_amd.llm.paged import PagedDecoder

            for kv_dtype in kv_dtypes:
                pd = PagedDecoder(
                    model, B, max_T, dev,
                    kv_dtype=torch.float8_e4m3fn if kv_dtype == "fp8"
                    else None)
                for k, v in zip(pd.pool.k, pd.pool.v):
                    # like the contiguous decoders' zero caches
                    k.view(torch.uint8).zero_()
                    v.view(torch.uint8).zero_()
                for slot in range(B):
                    pd.reserve_slot(slot, max_T)
                pd.capture()
                pms, pspread = timed(
                    lambda: bench_paged(pd, cfg, B, args.tokens, ctx))
                name = "paged" if kv_dtype == "bf16" else "paged fp8"
                print(f"batch {B:3d}: {name} hipGraph "
                      f"{B / pms * 1e3:9.1f} tok/s "
                      f"({pms:6.2f} ms/step{pspread})   "
                      f"splits {pd.num_splits}  "
                      f"GraphedDecoder/paged {ms / pms:5.2f}x")
                del pd


if __name__ == "__main__":
    main()
