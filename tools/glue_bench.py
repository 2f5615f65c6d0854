"""Kernel-level timings behind the fused RoPE / packed-QKV attention /
add+RMSNorm paths, at the flagship shapes (B 8, T 4096, Hq 32, Hkv 8, D 128,
hidden 4096).

  python tools/glue_bench.py [--parent-so PATH]

Median [min, max] microseconds per call over 7 repetitions of 20
back-to-back calls after warm-up (device events). With --parent-so (an
earlier build of ray_amd/_hip_ops.so) the attention forward and backward of
that build and of this one run alternating in one process, on the same
[B,T,H,D] tensors; the packed rows are this build reading and writing the
column sections of one [B,T,(Hq+2Hkv)*D] buffer.
"""
import argparse
import importlib.machinery
import importlib.util
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS, CALLS = 7, 20


def load_ext(path):
    loader = importlib.machinery.ExtensionFileLoader("_hip_ops", path)
    spec = importlib.util.spec_from_file_location("_hip_ops", path,
                                                  loader=loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


def time_us(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / CALLS)
    return out


def fmt(ts):
    return (f"{statistics.median(ts):9.1f} [{min(ts):9.1f}, {max(ts):9.1f}]")


def row(label, ts, nbytes=None):
    extra = ""
    if nbytes is not None:
        extra = f"  {nbytes / statistics.median(ts) / 1e6:6.2f} TB/s"
    print(f"{label:58s} {fmt(ts)}{extra}", flush=True)


def attn_section(args, ops, K, qkv, dims, bf):
    B, T, Hq, Hkv, D, W = dims
    print("== attention, B8 Hq32 Hkv8 T4096 D128 causal (us/call) ==")
    q4, k4, v4 = (t.transpose(1, 2) for t in (
        qkv[..., :Hq * D].reshape(B, T, Hq, D).contiguous(),
        qkv[..., Hq * D:(Hq + Hkv) * D].reshape(B, T, Hkv, D).contiguous(),
        qkv[..., (Hq + Hkv) * D:].reshape(B, T, Hkv, D).contiguous()))
    qp, kp, vp = ops._qkv_sections(qkv, Hq, Hkv)
    d_o = torch.randn(B, T, Hq, D, **bf).transpose(1, 2)
    out, lse = K.flash_attn_fwd(q4, k4, v4, True, 0, True)
    builds = [("new", K)]
    if args.parent_so:
        builds.insert(0, ("parent", load_ext(os.path.abspath(args.parent_so))))
    res = {}
    for rnd in range(2):            # alternate the builds, two rounds
        for name, ext in builds:
            res.setdefault((name, "fwd"), []).extend(time_us(
                lambda: ext.flash_attn_fwd(q4, k4, v4, True, 0, True)))
            res.setdefault((name, "bwd"), []).extend(time_us(
                lambda: ext.flash_attn_bwd(q4, k4, v4, out, d_o, lse, True)))
    for (name, what), ts in res.items():
        row(f"{name:7s} {what} on [B,T,H,D] storage"
            + (" (prep + dq + dkv)" if what == "bwd" else ""), ts)
    if args.parent_so:
        for what in ("fwd", "bwd"):
            p, n = res[("parent", what)], res[("new", what)]
            print(f"  {what}: new - parent = "
                  f"{statistics.median(n) - statistics.median(p):+.1f} us, "
                  f"parent max - min = {max(p) - min(p):.1f} us")
    o2, l2 = K.flash_attn_fwd(qp, kp, vp, True, 0, True)
    assert torch.equal(o2, out) and torch.equal(l2, lse)
    g = torch.empty(B, T, W, **bf)
    row("new     fwd on packed sections",
        time_us(lambda: K.flash_attn_fwd(qp, kp, vp, True, 0, True)))
    row("new     bwd on packed sections, packed gradient",
        time_us(lambda: K.flash_attn_bwd(qp, kp, vp, out, d_o, lse, True, g)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-so", default=None)
    ap.add_argument("--attn-only", action="store_true",
                    help="stop after the attention section")
    ap.add_argument("--skip-attn", action="store_true",
                    help="leave the attention section out")
    args = ap.parse_args()
    from ray_amd import ops
    K = ops._K
    dev = torch.device("cuda")
    torch.manual_seed(0)
    B, T, Hq, Hkv, D, Hd = 8, 4096, 32, 8, 128, 4096
    W = (Hq + 2 * Hkv) * D
    bf = dict(device=dev, dtype=torch.bfloat16)

    qkv = torch.randn(B, T, W, **bf)
    if not args.skip_attn:
        attn_section(args, ops, K, qkv, (B, T, Hq, Hkv, D, W), bf)
    if args.attn_only:
        return 0

    print("== RoPE and the copies around it (us/call) ==")
    cosT, sinT = (t.to(dev) for t in ops.rope_tables(T, D))
    qs = qkv[..., :Hq * D].view(B, T, Hq, D)
    ks = qkv[..., Hq * D:(Hq + Hkv) * D].view(B, T, Hkv, D)
    vs = qkv[..., (Hq + Hkv) * D:].view(B, T, Hkv, D)
    nq, nk = B * T * Hq * D * 2, B * T * Hkv * D * 2
    row("rope_fwd q slice -> contiguous", time_us(
        lambda: K.rope_apply(qs, cosT, sinT, Hq, T, 1)), 2 * nq)
    row("rope_fwd k slice -> contiguous", time_us(
        lambda: K.rope_apply(ks, cosT, sinT, Hkv, T, 1)), 2 * nk)
    row("v.contiguous()", time_us(lambda: vs.contiguous()), 2 * nk)
    row("rope_qk_inplace (q and k sections, one launch)", time_us(
        lambda: K.rope_qk_inplace(qkv, cosT, sinT, Hq, Hkv, 1)),
        2 * (nq + nk))
    parts = [torch.randn(B, T, n, **bf) for n in (Hq * D, Hkv * D, Hkv * D)]
    row("torch.cat of dq, dk, dv", time_us(lambda: torch.cat(parts, -1)),
        2 * B * T * W * 2)

    print("== RMSNorm, N 32768 x H 4096 (us/call) ==")
    N = B * T
    x = torch.randn(N, Hd, **bf)
    r = torch.randn(N, Hd, **bf)
    dy = torch.randn(N, Hd, **bf)
    gs = torch.randn(N, Hd, **bf)
    w = torch.ones(Hd, **bf)
    nb = N * Hd * 2
    _, inv = K.rmsnorm_fwd(x, w, 1e-5)
    row("x + r (torch)", time_us(lambda: x + r), 3 * nb)
    row("rmsnorm_fwd", time_us(lambda: K.rmsnorm_fwd(x, w, 1e-5)), 2 * nb)
    row("add_rmsnorm_fwd", time_us(
        lambda: K.add_rmsnorm_fwd(x, r, w, 1e-5)), 4 * nb)
    row("rmsnorm_bwd two-pass (dx, then dw)", time_us(
        lambda: K.rmsnorm_bwd_two_pass(dy, x, w, inv)), 3 * nb)
    for grid in (256, 512, 1024, 2048):
        row(f"rmsnorm_bwd one-pass, grid {grid}", time_us(
            lambda: K.rmsnorm_bwd_res(dy, x, w, inv, None, grid)), 3 * nb)
        row(f"rmsnorm_bwd one-pass + g_res, grid {grid}", time_us(
            lambda: K.rmsnorm_bwd_res(dy, x, w, inv, gs, grid)), 4 * nb)
    return 0


if __name__ == "__main__":
    sys.exit(main())
