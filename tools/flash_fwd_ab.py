"""Forward attention of this build against an earlier build of
ray_amd/_hip_ops.so, loaded side by side in one process:

  python tools/flash_fwd_ab.py --parent-so PATH [--skip-bits] [--skip-time]

Same bits: out and LSE of the two builds must be torch.equal at the shapes
of tests/test_flash_fwd_v7.py (every layout, q_offset, ragged Tk, the
defer-max inputs) and at B2 Hq32 Hkv8 T4096. Timing: the shapes of
tools/flash_sweep.py, the two builds alternating, median [min, max]
microseconds per call over 7 repetitions of 20 calls (device events); the
margin is the parent's own max - min.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.glue_bench import fmt, load_ext, time_us  # noqa: E402

D = 128


def _rand(*shape):
    return torch.randn(*shape, device="cuda", dtype=torch.bfloat16)


def same_bits(K, P, ops):
    bad = 0

    def check(label, q, k, v, causal, q_offset=0):
        nonlocal bad
        o_n, l_n = K.flash_attn_fwd(q, k, v, causal, q_offset, True)
        o_p, l_p = P.flash_attn_fwd(q, k, v, causal, q_offset, True)
        ok = torch.equal(o_n, o_p) and torch.equal(l_n, l_p)
        bad += not ok
        print(f"{'same' if ok else 'DIFFERENT':9s} {label}", flush=True)

    torch.manual_seed(11)
    for Tk in (40, 64, 128, 192, 300, 320, 1024):
        check(f"non-causal T256 Tk{Tk}", _rand(1, 4, 256, D),
              _rand(1, 2, Tk, D), _rand(1, 2, Tk, D), False)
    for B, Hq, Hkv, T in ((1, 4, 2, 256), (2, 8, 2, 512), (1, 4, 4, 768),
                          (2, 32, 8, 4096)):
        q, k, v = _rand(B, Hq, T, D), _rand(B, Hkv, T, D), _rand(B, Hkv, T, D)
        check(f"causal B{B} Hq{Hq} Hkv{Hkv} T{T} BHTD", q, k, v, True)
        qt, kt, vt = (t.transpose(1, 2).contiguous().transpose(1, 2)
                      for t in (q, k, v))
        check(f"causal B{B} Hq{Hq} Hkv{Hkv} T{T} BTHD view", qt, kt, vt, True)
        W = (Hq + 2 * Hkv) * D
        for pad in (0, 128):
            wide = _rand(B, T, W + 2 * pad)
            qkv = wide[..., pad:pad + W] if pad else wide
            qs, ks, vs = ops._qkv_sections(qkv, Hq, Hkv)
            qs.copy_(q), ks.copy_(k), vs.copy_(v)
            check(f"causal B{B} Hq{Hq} Hkv{Hkv} T{T} packed, pad {pad}",
                  qs, ks, vs, True)
    for Tk in (320, 576):
        check(f"causal T256 Tk{Tk} q_offset {Tk - 256}", _rand(1, 4, 256, D),
              _rand(1, 2, Tk, D), _rand(1, 2, Tk, D), True, Tk - 256)
    torch.manual_seed(7)
    q = torch.randn(1, 4, 512, D).to(torch.bfloat16).cuda()
    k = torch.randn(1, 2, 512, D).to(torch.bfloat16)
    v = torch.randn(1, 2, 512, D).to(torch.bfloat16).cuda()
    for j in (70, 200, 235, 300, 497):
        k[:, :, j] *= 6
    k = k.cuda()
    for causal in (False, True):
        check(f"defer-max inputs, causal {causal}", q, k, v, causal)
    return bad


def timing(K, P):
    print(f"{'shape (causal, BHTD)':28s} {'parent us':>32s} {'new us':>32s}"
          f" {'new-parent':>10s} {'margin':>7s}")
    for B, Hq, Hkv, T in ((16, 32, 8, 2048), (8, 32, 8, 4096),
                          (2, 32, 8, 8192), (8, 32, 32, 4096),
                          (8, 16, 16, 4096), (8, 32, 8, 256)):
        q, k, v = _rand(B, Hq, T, D), _rand(B, Hkv, T, D), _rand(B, Hkv, T, D)
        tp, tn = [], []
        for _ in range(2):
            tp += time_us(lambda: P.flash_attn_fwd(q, k, v, True, 0, True))
            tn += time_us(lambda: K.flash_attn_fwd(q, k, v, True, 0, True))
        tf = 2 * B * Hq * T * T * D / statistics.median(tn) / 1e6
        print(f"B{B} Hq{Hq}/Hkv{Hkv} T{T}".ljust(28) + f" {fmt(tp)} {fmt(tn)}"
              f" {statistics.median(tn) - statistics.median(tp):+10.1f}"
              f" {max(tp) - min(tp):7.1f}  new {tf:.0f} TF/s", flush=True)


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
        print(f"{bad} shapes differ")
    if not args.skip_time:
        timing(K, P)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
