"""Paged decode-attention kernel alone vs what the contiguous decoders
do today: F.scaled_dot_product_attention with an additive mask over an
equally sized contiguous [B, Hkv, capacity, D] cache.

    python tools/paged_attn_bench.py [--batches 1,8,32] [--lens 1024,4096]
        [--kv-dtype bf16,fp8]

Reports median / min / max microseconds per call over --reps timed
repetitions (each of --iters back-to-back calls, after warm-up) and
the achieved KV read rate 2*B*Hkv*seq_len*D*(bytes per cache element)
per call. With an fp8 cache the reference reads the dequantised values
as bf16 (exact), so max|diff| is kernel arithmetic alone.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from ray_amd import ops

HIPBLASLT_STREAM_TBS = 5.7  # ops.linear_sb docstring: measured weight stream


def time_us(fn, iters, reps, warmup=10):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--lens", default="1024,4096")
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--hq", type=int, default=32)
    ap.add_argument("--hkv", type=int, default=8)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--splits", type=int, default=0,
                    help="0 = the op's default choice")
    ap.add_argument("--kv-dtype", default="bf16",
                    help="comma-separated cache formats: bf16, fp8")
    args = ap.parse_args()
    kv_dtypes = args.kv_dtype.split(",")
    assert set(kv_dtypes) <= {"bf16", "fp8"}, kv_dtypes

    dev = torch.device("cuda", 0)
    Hq, Hkv, D, cap = args.hq, args.hkv, args.d, args.capacity
    page = ops.PAGE_SIZE
    max_pages = cap // page
    torch.manual_seed(0)
    print(f"# Hq={Hq} Hkv={Hkv} D={D} capacity={cap} iters={args.iters} "
          f"reps={args.reps}; us per call: median [min, max]")
    for kv_dtype, B in [(k, int(b)) for k in kv_dtypes
                        for b in args.batches.split(",")]:
        if args.kv_dtype != "bf16":
            print(f"# kv_dtype={kv_dtype}")
        num_pages = B * max_pages + 1
        kc = torch.randn(num_pages, Hkv, page, D, device=dev,
                         dtype=torch.bfloat16)
        vc = torch.randn_like(kc)
        if kv_dtype == "fp8":
            kc, vc = ops.quantize_kv_fp8(kc), ops.quantize_kv_fp8(vc)
        # shuffled page assignment, as a long-running pool would have
        perm = (torch.randperm(num_pages - 1) + 1).to(torch.int32)
        bt = perm.view(B, max_pages).to(dev)
        q = torch.randn(B, Hq, D, device=dev, dtype=torch.bfloat16)
        # the same K/V, contiguous, for the reference
        ck = (kc[bt.long()].permute(0, 2, 1, 3, 4)
              .reshape(B, Hkv, cap, D).contiguous().to(torch.bfloat16))
        cv = (vc[bt.long()].permute(0, 2, 1, 3, 4)
              .reshape(B, Hkv, cap, D).contiguous().to(torch.bfloat16))
        q4 = q.view(B, Hq, 1, D)
        for L in [int(x) for x in args.lens.split(",")]:
            sl = torch.full((B,), L, dtype=torch.int32, device=dev)
            mask = torch.full((B, 1, 1, cap), float("-inf"), device=dev,
                              dtype=torch.float32)
            mask[..., :L] = 0.0
            S = args.splits or ops.default_num_splits(B, Hkv, cap, dev)
            ws = torch.empty(B * Hq * S * (D + 2), dtype=torch.float32,
                             device=dev)

            def paged():
                return ops.paged_attention_decode(q, kc, vc, bt, sl,
                                                  num_splits=S, workspace=ws)

            def sdpa():
                # as GraphedDecoder/BatchedDecoder call it, cast included
                return F.scaled_dot_product_attention(
                    q4, ck, cv, attn_mask=mask.to(q.dtype), enable_gqa=True)

            err = float((paged().float()
                         - sdpa().view(B, Hq, D).float()).abs().max())
            p_med, p_min, p_max = time_us(paged, args.iters, args.reps)
            s_med, s_min, s_max = time_us(sdpa, args.iters, args.reps)
            kv_bytes = 2 * B * Hkv * L * D * kc.element_size()
            tbs = kv_bytes / (p_med * 1e-6) / 1e12
            print(f"B={B:3d} seq_len={L:5d} splits={S:3d}  "
                  f"paged {p_med:8.1f} [{p_min:8.1f},{p_max:8.1f}] us "
                  f"{tbs * 1e3:7.1f} GB/s "
                  f"({tbs / HIPBLASLT_STREAM_TBS * 100:4.1f}% of "
                  f"{HIPBLASLT_STREAM_TBS} TB/s)  "
                  f"sdpa+mask {s_med:8.1f} [{s_min:8.1f},{s_max:8.1f}] us  "
                  f"sdpa/paged {s_med / p_med:5.2f}x  "
                  f"max|diff| {err:.2e}")
        del kc, vc, ck, cv


if __name__ == "__main__":
    main()
