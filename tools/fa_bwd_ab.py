"""Attention backward of this build against an earlier build of
ray_amd/_hip_ops.so, loaded side by side in one process:

  python tools/fa_bwd_ab.py --parent-so PATH [--skip-bits] [--skip-time]

Same bits: dq, dk and dv of the two builds must be torch.equal at the shapes
of tests/test_fa_bwd_dq_order.py and of tests/test_fa_bwd_v6.py and at
B2 Hq32 Hkv8 T4096, each on contiguous [B,H,T,D] tensors, on BTHD views and
on the column sections of a packed buffer with the packed gradient, and at
three shapes of the 128-row path on contiguous tensors. Timing:
the backward unit (the binding launches fa_bwd_prep, the dq and the dkv
kernel together), the two builds alternating, median [min, max]
microseconds per call over 2 x 7 repetitions of 20 calls (device events);
the margin is the parent's own max - min.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.glue_bench import fmt, load_ext, time_us  # noqa: E402

D = 128
PAD = 128

# (B, Hq, Hkv, T, causal)
BIT_SHAPES = [
    # tests/test_fa_bwd_dq_order.py
    (1, 4, 2, 768, True), (1, 5, 5, 1280, True), (1, 4, 4, 256, True),
    (1, 8, 2, 512, False), (2, 4, 1, 2048, True),
    # tests/test_fa_bwd_v6.py (its T256 and T512 shapes are above)
    (2, 8, 2, 768, True), (2, 4, 1, 1024, True),
    (2, 32, 8, 4096, True),
    # the 128-row kernels (T % 256 != 0): contiguous [B,H,T,D] only
    (2, 8, 2, 384, True), (1, 4, 4, 384, False), (1, 4, 2, 128, True),
]

# (B, Hq, Hkv, T, layout), causal
TIME_SHAPES = [
    (8, 32, 8, 4096, "bhtd"), (8, 32, 8, 4096, "view"),
    (8, 32, 8, 4096, "packed"), (16, 32, 8, 2048, "bhtd"),
    (2, 32, 8, 8192, "bhtd"), (8, 32, 32, 4096, "bhtd"),
    (8, 32, 8, 3968, "bhtd"),  # the 128-row kernels
]


def _rand(*shape):
    return torch.randn(*shape, device="cuda", dtype=torch.bfloat16)


def _operands(ops, B, Hq, Hkv, T, layout):
    """q, k, v, dO in one layout and, for "packed", a gradient buffer
    factory (None otherwise)."""
    if layout == "bhtd":
        return [_rand(B, H, T, D) for H in (Hq, Hkv, Hkv, Hq)], None
    q, k, v, g = (_rand(B, T, H, D).transpose(1, 2)
                  for H in (Hq, Hkv, Hkv, Hq))
    if layout == "view":
        return [q, k, v, g], None
    W = (Hq + 2 * Hkv) * D
    qkv = _rand(B, T, W + 2 * PAD)[..., PAD:PAD + W]
    qs, ks, vs = ops._qkv_sections(qkv, Hq, Hkv)
    qs.copy_(q), ks.copy_(k), vs.copy_(v)

    def grad_buffer():
        return torch.full((B, T, W + 2 * PAD), float("nan"), device="cuda",
                          dtype=torch.bfloat16)[..., PAD:PAD + W]
    return [qs, ks, vs, g], grad_buffer


def same_bits(K, P, ops):
    bad = 0
    torch.manual_seed(11)
    for B, Hq, Hkv, T, causal in BIT_SHAPES:
        for layout in ("bhtd", "view", "packed") if T % 256 == 0 \
                else ("bhtd",):
            (q, k, v, g), buf = _operands(ops, B, Hq, Hkv, T, layout)
            out, lse = K.flash_attn_fwd(q, k, v, causal, 0, True)
            res = []
            for ext in (K, P):
                args = (q, k, v, out, g, lse, causal)
                res.append(ext.flash_attn_bwd(*args, buf()) if buf
                           else ext.flash_attn_bwd(*args))
            same = [torch.equal(a, b) for a, b in zip(*res)]
            finite = all(bool(torch.isfinite(t).all()) for t in res[0])
            ok = all(same) and finite
            bad += not ok
            what = " ".join(n for n, s in zip(("dq", "dk", "dv"), same)
                            if not s)
            print(f"{'same' if ok else 'DIFFERENT ' + what:9s} "
                  f"B{B} Hq{Hq} Hkv{Hkv} T{T} "
                  f"{'causal' if causal else 'full'} {layout}"
                  + ("" if finite else " (not finite)"), flush=True)
    return bad


def timing(K, P, ops):
    print(f"{'backward unit (causal)':34s} {'parent us':>32s} {'new us':>32s}"
          f" {'new-parent':>10s} {'margin':>7s}")
    for B, Hq, Hkv, T, layout in TIME_SHAPES:
        (q, k, v, g), buf = _operands(ops, B, Hq, Hkv, T, layout)
        out, lse = K.flash_attn_fwd(q, k, v, True, 0, True)
        gb = buf() if buf else None

        def run(ext):
            if gb is not None:
                return lambda: ext.flash_attn_bwd(q, k, v, out, g, lse, True,
                                                  gb)
            return lambda: ext.flash_attn_bwd(q, k, v, out, g, lse, True)
        tp, tn = [], []
        for _ in range(2):
            tp += time_us(run(P))
            tn += time_us(run(K))
        print(f"B{B} Hq{Hq}/Hkv{Hkv} T{T} {layout}".ljust(34)
              + f" {fmt(tp)} {fmt(tn)}"
              f" {statistics.median(tn) - statistics.median(tp):+10.1f}"
              f" {max(tp) - min(tp):7.1f}", flush=True)
        del q, k, v, g, out, lse, gb
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-so", required=True)
    ap.add_argument("--skip-bits", action="store_true")
    ap.add_argument("--skip-time", action="store_true")
    args = ap.parse_args()
    from ray_amd import ops
    K = ops._K
    P = load_ext(os.path.abspath(args.parent_so))
    bad = 0
    if not args.skip_bits:
        bad = same_bits(K, P, ops)
        print(f"{bad} cases differ")
    if not args.skip_time:
        timing(K, P, ops)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
