"""Edge-shape tests for the small HIP ops: RMSNorm, SwiGLU, RoPE, fused cross
entropy, fused AdamW, the decode GEMV, the GAE / V-trace scans and the image
normalize (csrc/hip/{rmsnorm,elementwise,cross_entropy,gemv,rl_scans}.hip).

Every GPU test compares a kernel with an fp64 reference computed from the same
bf16 / fp32 inputs. The references are the plain torch functions in this file;
the CPU tests at the top check them, and check that the two bound helpers
reject a set of injected kernel defects.

Bounds
------
bf16 outputs of elementwise ops (`check_bf16`):
|got - ref| <= 2^-8 |ref| + 2^-133 + a.
Round-to-nearest-even gives 2^-9; the factor 2 covers an fp32 evaluation error
that lands on the neighbouring bf16 value. Below 2^-126 bf16 is subnormal with
a fixed spacing of 2^-133, so there the same two half-steps are 2^-133 (a
correctly rounded 3.4e-39 is 1 % off). `a` is the fp32 error of the part
that cancels: RoPE 2^-20 (|x1|+|x2|); image normalize 1e-6; SwiGLU 1e-30 |b|
(1e-30 |dy b| and 1e-30 |dy| in backward: `__expf` overflows past |a| ~ 88
where the true value is below 1e-36 |b|); RMSNorm dx
2^-20 (|dy w inv| + |x k|); CE dlogits 2^-20 |dl| at the target column (the
p dl - dl subtraction) plus 2^-125 (|dl| + 1) everywhere (`__expf` returns 0
for results below the smallest normal fp32, 2^-126); the bf16 AdamW parameter
2^-20 sum|terms| of p.

bf16 outputs of fp32 reductions (RMSNorm dw, GEMV):
2^-8 |ref| + n 2^-24 sum|terms|, n the number of summands.

fp32 outputs (`check_f32`): CE loss / lse, the RMSNorm inv, GAE, V-trace,
AdamW p / m / v / master. The same formula is evaluated with plain torch ops in
fp32 on the GPU; with every error divided by the element's sum|terms| (from
the fp64 reference), the kernel's largest error must be at most 4x torch's
largest, with a floor of 2^-22. The factor 4 allows 2-ulp intrinsics against
libm's 1 ulp and another summation order. Dividing by sum|terms| per element
keeps one huge row (a 3e38 logit) from hiding the others.

lm_head_cross_entropy is a bf16 GEMM pipeline: its loss, dx and dW errors
against the fp64 reference must be at most 1.1x those of the same chunked
computation done with torch bf16 ops (as in test_gemm_wgrad.py).

Measured on an MI355X (largest scaled error over all cases, kernel / torch
fp32, and the case that came closest to its bound):
  CE lse        9.3e-08 / 8.3e-08   (4,4107) randn: 9.3e-08 / 3.4e-08
  CE row loss   1.0e-07 / 1.0e-07   (4,4107) randn: 8.9e-08 / 3.2e-08
  CE mean loss  1.1e-07 / 1.2e-07   (4,4107) randn: 7.1e-08 / 2.5e-08
  RMSNorm inv   1.3e-07 / 1.1e-07   (129,4096): 1.1e-07 / 7.1e-08
  GAE adv       1.1e-07 / 1.3e-07   vtarg 1.4e-07 / 1.5e-07
  V-trace vs    1.8e-07 / 1.6e-07   pg 2.8e-07 / 1.6e-07; (7,257) pg:
                                    2.8e-07 / 1.1e-07, 0.64 of its bound
  AdamW         p 2.5e-07 / 2.7e-07, m 4.2e-07 / 4.2e-07, v 5.2e-07 / 5.2e-07
  AdamW t=1000  p 1.4e-07 / 1.4e-07 (m and v exact in both)
  lm_head       loss 9.79e-06 / 9.79e-06, dx rel 1.80e-03 / 1.80e-03,
                dW rel 2.46e-03 / 2.46e-03 (ours / torch bf16, identical)
AdamW's m and p are sums over all steps so far; their sum|terms| is carried
from step to step (`adamw_formula`), so an m that has cancelled keeps the scale
of its summands. Most of the AdamW error, torch's too, is beta in fp32:
1 - fp32(0.9) and 1 - fp32(0.95) are 2.4e-07 off.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from ray_amd import ops

REL = 2.0 ** -8
BF16_SUBNORMAL_STEP = 2.0 ** -133          # spacing of bf16 below 2^-126
BF16_OVER = 2.0 ** 128 * (1 - 2.0 ** -9)   # rounds to inf in bf16
F32_FLOOR = 2.0 ** -22
CPU = torch.device("cpu")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if not ops.HAVE_HIP_OPS:
        raise RuntimeError("HIP extension not built")
    return torch.device("cuda")


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _randn(shape, seed, dev, scale=1.0, dtype=torch.bfloat16):
    """Seeded on the CPU so that every device sees the same values."""
    t = torch.randn(shape, generator=_gen(seed), dtype=torch.float32) * scale
    return t.to(dtype).to(dev)


def _rne(ref):
    """fp64 -> bf16, round to nearest even."""
    return ref.to(torch.bfloat16)


# --------------------------------------------------------------------------
# bound helpers
# --------------------------------------------------------------------------


def check_bf16(got, ref, a=0.0, tag=""):
    """|got - ref| <= 2^-8 |ref| + 2^-133 + a elementwise; `a` a number or a
    tensor.
    Where ref is beyond the bf16 range, inf of the right sign passes too."""
    assert got.dtype == torch.bfloat16, (tag, got.dtype)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    ref = ref.double().to(got.device)
    assert torch.isfinite(ref).all(), (tag, "reference not finite")
    g = got.double()
    a = torch.as_tensor(a, dtype=torch.float64, device=got.device)
    bound = REL * ref.abs() + BF16_SUBNORMAL_STEP + a
    err = (g - ref).abs()
    ok = err <= bound
    over = ref.abs() + bound >= BF16_OVER
    ok |= over & torch.isinf(g) & (torch.sign(g) == torch.sign(ref))
    if not ok.all():
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(
            f"{tag}: {bad.shape[0]} of {ok.numel()} outside the bound; first "
            f"at {i}: got {g[i].item()!r} ref {ref[i].item()!r} "
            f"bound {bound[i].item()!r}")
    return (err / bound.clamp_min(1e-300)).max().item()


def check_sum_bf16(got, ref, terms, n, tag=""):
    """bf16 result of an n-term fp32 sum; terms = sum |summand| (fp64)."""
    return check_bf16(got, ref, n * 2.0 ** -24 * terms.double(), tag)


def check_f32(got, ref, t32, terms, tag=""):
    """Kernel error <= max(4 x torch fp32 error, 2^-22), both divided by
    sum|terms| per element. Returns (kernel, torch)."""
    assert got.dtype == torch.float32 and t32.dtype == torch.float32, tag
    assert got.shape == ref.shape == t32.shape, (tag, got.shape, ref.shape)
    ref = ref.double().to(got.device)
    assert torch.isfinite(ref).all(), (tag, "reference not finite")
    scale = terms.double().to(got.device).expand_as(ref).clamp_min(1e-300)
    ek = ((got.double() - ref).abs() / scale).max().item()
    et = ((t32.double().to(got.device) - ref).abs() / scale).max().item()
    print(f"f32 {tag}: kernel {ek:.3e} torch {et:.3e}")
    bound = max(4 * et, F32_FLOOR)
    if not ek <= bound:      # also catches nan
        raise AssertionError(f"{tag}: kernel {ek:.3e} torch {et:.3e} "
                             f"bound {bound:.3e}")
    return ek, et


def _errs(got, ref):
    got = got.double()
    rel = ((got - ref).norm() / ref.norm()).item()
    mx = ((got - ref).abs().max() / ref.abs().max()).item()
    return rel, mx


# --------------------------------------------------------------------------
# references (dtype- and device-generic: fp64 for the reference, fp32 for
# torch's own evaluation of the same formula)
# --------------------------------------------------------------------------


def rms_ref(x, w, eps, dy=None, dtype=torch.float64):
    H = x.shape[-1]
    xf = x.reshape(-1, H).to(dtype)
    wf = w.to(dtype)
    inv = (xf.pow(2).mean(-1) + eps).rsqrt()
    out = {"inv": inv, "y": (xf * inv[:, None] * wf).view(x.shape)}
    if dy is not None:
        g = dy.reshape(-1, H).to(dtype) * wf
        k = (g * xf).sum(-1) * inv.pow(3) / H
        t1, t2 = g * inv[:, None], xf * k[:, None]
        out["dx"] = (t1 - t2).view(x.shape)
        out["a_dx"] = (2.0 ** -20 * (t1.abs() + t2.abs())).view(x.shape)
        prod = dy.reshape(-1, H).to(dtype) * xf * inv[:, None]
        out["dw"] = prod.sum(0)
        out["dw_terms"] = prod.abs().sum(0)
        out["prod"] = prod
    return out


def swiglu_ref(a, b, dy):
    a, b, dy = a.double(), b.double(), dy.double()
    s = torch.sigmoid(a)
    silu = a * s
    dsilu = s * (1 + a * (1 - s))
    return {"y": silu * b, "a_y": 1e-30 * b.abs(),
            "da": dy * b * dsilu, "a_da": 1e-30 * (dy * b).abs(),
            "db": dy * silu, "a_db": 1e-30 * dy.abs()}


def rope_ref64(x, cosT, sinT, sign=1):
    B, T, Hn, D = x.shape
    half = D // 2
    x1, x2 = x[..., :half].double(), x[..., half:].double()
    c = cosT[:T].double().view(1, T, 1, half)
    s = sign * sinT[:T].double().view(1, T, 1, half)
    y = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    a = 2.0 ** -20 * (x1.abs() + x2.abs())
    return y, torch.cat([a, a], -1)


def ce_rows(logits, tgt, dtype=torch.float64):
    """Per-row (loss, mx, lse, terms_loss, terms_lse); tgt < 0 is ignored."""
    x = logits.to(dtype)
    mx = x.max(-1).values
    lse_m = (x - mx[:, None]).exp().sum(-1).log()
    lse = lse_m + mx
    valid = tgt >= 0
    xt = x.gather(1, tgt.clamp(min=0).long()[:, None])[:, 0]
    zero = torch.zeros_like(lse)
    loss = torch.where(valid, lse - xt, zero)
    return (loss, mx, lse, torch.where(valid, lse.abs() + xt.abs(), zero),
            lse_m.abs() + mx.abs())


def ce_mean(logits, tgt, dtype=torch.float64):
    loss, _, _, terms, _ = ce_rows(logits, tgt, dtype)
    nvalid = (tgt >= 0).sum().clamp(min=1).to(dtype)
    return loss.sum() / nvalid, terms.sum() / nvalid


def ce_dlogits_ref(logits, tgt, upstream, shift=0):
    """fp64 (softmax - onehot) * upstream / nvalid and the bound's `a`;
    `shift` moves the one-hot (the injected defect)."""
    x = logits.double()
    N, V = x.shape
    valid = tgt >= 0
    nvalid = valid.sum().clamp(min=1).double()
    dl = torch.where(valid, upstream / nvalid, torch.zeros_like(nvalid))
    onehot = torch.zeros_like(x)
    rows = valid.nonzero()[:, 0]
    onehot[rows, (tgt[rows].long() + shift) % V] = 1.0
    ref = (torch.softmax(x, -1) - onehot) * dl[:, None]
    a = 2.0 ** -20 * onehot * dl[:, None].abs() \
        + 2.0 ** -125 * (dl[:, None].abs() + 1)
    return ref, a


def adamw_formula(p, g, m, v, lr, b1, b2, eps, wd, t, scale, tm=None,
                  tp=None):
    """One AdamW step with every quantity in p's dtype (tensors m, v, p
    are replaced, not updated). Returns p, m, v and their sum|terms|.
    m is a signed sum over all steps so far and p a sum of updates built
    from it: `tm` and `tp` carry their sum|terms| from the step before, so
    that an m that has cancelled keeps the scale of what it was summed from
    (v is a sum of squares and is its own sum|terms|)."""
    def S(z):
        return torch.tensor(z, dtype=p.dtype, device=p.device)

    lr, b1, b2, eps, wd, scale, one = map(S, (lr, b1, b2, eps, wd, scale, 1.0))
    gf = g.to(p.dtype) * scale
    m2 = b1 * m + (one - b1) * gf
    v2 = b2 * v + (one - b2) * gf * gf
    bc1 = one - b1.pow(t)
    bc2 = one - b2.pow(t)
    upd = (m2 / bc1) / ((v2 / bc2).sqrt() + eps)
    p2 = p - lr * (upd + wd * p)
    tm = b1 * (m.abs() if tm is None else tm) + (one - b1) * gf.abs()
    tp = p.abs() if tp is None else tp
    tp = tp + lr * ((tm / bc1) / ((v2 / bc2).sqrt() + eps) + wd * tp)
    return p2, m2, v2, {"m": tm, "v": v2, "p": tp}


def gemv_ref(x, w):
    xd, wd = x.double(), w.double()
    return xd @ wd.t(), xd.abs() @ wd.abs().t()


def gae_scan(r, v, cont, gamma, lam):
    """Returns adv, vtarg and their sum|terms|, in r's dtype."""
    T, B = r.shape
    adv, tadv = torch.empty_like(r), torch.empty_like(r)
    run = torch.zeros(B, dtype=r.dtype, device=r.device)
    trun = torch.zeros_like(run)
    for t in reversed(range(T)):
        gc = gamma * cont[t]
        run = r[t] + gc * v[t + 1] - v[t] + gamma * lam * cont[t] * run
        trun = (r[t].abs() + gc * v[t + 1].abs() + v[t].abs()
                + gamma * lam * cont[t] * trun)
        adv[t], tadv[t] = run, trun
    return adv, adv + v[:-1], tadv, tadv + v[:-1].abs()


def vtrace_scan(log_rhos, r, v, cont, gamma, rho_clip, c_clip, pg_clip):
    """Returns vs, pg and their sum|terms|, in r's dtype."""
    T, B = r.shape
    rhos = log_rhos.exp()
    rho, cs = rhos.clamp(max=rho_clip), rhos.clamp(max=c_clip)
    rpg = rhos.clamp(max=pg_clip)
    vs, tvs = torch.empty_like(r), torch.empty_like(r)
    diff = torch.zeros(B, dtype=r.dtype, device=r.device)
    tdiff = torch.zeros_like(diff)
    for t in reversed(range(T)):
        gc = gamma * cont[t]
        diff = rho[t] * (r[t] + gc * v[t + 1] - v[t]) + gc * cs[t] * diff
        tdiff = (rho[t] * (r[t].abs() + gc * v[t + 1].abs() + v[t].abs())
                 + gc * cs[t] * tdiff)
        vs[t], tvs[t] = v[t] + diff, v[t].abs() + tdiff
    pg, tpg = torch.empty_like(r), torch.empty_like(r)
    for t in range(T):
        gc = gamma * cont[t]
        nxt = v[t + 1] if t == T - 1 else vs[t + 1]
        tnxt = v[t + 1].abs() if t == T - 1 else tvs[t + 1]
        pg[t] = rpg[t] * (r[t] + gc * nxt - v[t])
        tpg[t] = rpg[t] * (r[t].abs() + gc * tnxt + v[t].abs())
    return vs, pg, tvs, tpg


def img_ref(x_u8, mean, std):
    out = (x_u8.double() / 255.0 - mean.double().view(1, 1, 1, -1)) \
        / std.double().view(1, 1, 1, -1)
    return out.permute(0, 3, 1, 2).contiguous()


# --------------------------------------------------------------------------
# seeded inputs shared by the CPU self-checks and the GPU tests
# --------------------------------------------------------------------------


def _rms_inputs(shape, seed, dev, xscale=1.0):
    H = shape[-1]
    return (_randn(shape, seed, dev, xscale), _randn((H,), seed + 1, dev),
            _randn(shape, seed + 2, dev))


CE_KINDS = ["randn", "randn20", "const", "outlier", "neginf"]


def _ce_target_choices(V):
    V8 = V // 8 * 8
    c = [0, V - 1]
    if V8 >= 1:
        c.append(V8 - 1)
    if V8 < V:
        c.append(V8)
    return c + [-100]


def _ce_logits(N, V, kind, seed, dev):
    g = _gen(seed)
    x = torch.randn(N, V, generator=g)
    if kind == "randn20":
        x *= 20
    elif kind == "const":
        x[:] = (torch.arange(N) * 0.75 - 1.0)[:, None]
    elif kind == "outlier":
        x[0, (2 * V) // 3] = 3e38
    elif kind == "neginf":
        mask = torch.rand(N, V, generator=g) < 0.3
        for c in _ce_target_choices(V)[:-1]:   # targets and the max stay finite
            mask[:, c] = False
        x[mask] = float("-inf")
    return x.to(torch.bfloat16).to(dev)


def _ce_targets(N, V, rot, dev):
    c = _ce_target_choices(V)
    return torch.tensor([c[(r + rot) % len(c)] for r in range(N)],
                        dtype=torch.int64, device=dev)


def _scan_inputs(T, B, seed, dev, dtype=torch.float32):
    g = _gen(seed)
    r = torch.randn(T, B, generator=g)
    v = torch.randn(T + 1, B, generator=g)
    cont = (torch.rand(T, B, generator=g) > 0.1).float()
    cont[0, ::3] = 0.0
    cont[T - 1, ::2] = 0.0
    log_rhos = 1.5 * torch.randn(T, B, generator=g)
    return [t.to(dtype).to(dev) for t in (log_rhos, r, v, cont)]


LR, EPS = 1e-2, 1e-8
# exact in fp32, so that the fp32 evaluation carries no error of beta's own
# (1 - fp32(0.999) is 1.3e-5 off, more than one step of the exponent moves p)
BETAS_EXACT = (0.875, 1 - 2.0 ** -10)

VTRACE_CLIPS = dict(rho_clip=0.7, c_clip=1.3, pg_clip=2.0)


def _img_inputs(shape, seed, dev):
    C = shape[-1]
    x = torch.randint(0, 256, shape, generator=_gen(seed), dtype=torch.uint8)
    mean = torch.tensor([0.485, 0.456, 0.406, 0.5][:C], dtype=torch.float64)
    std = torch.tensor([0.229, 0.224, 0.225, 0.25][:C], dtype=torch.float64)
    return x.to(dev), mean.to(dev), std.to(dev)


# --------------------------------------------------------------------------
# CPU self-checks: the references, and the helpers against injected defects
# --------------------------------------------------------------------------


def test_check_bf16_accepts_rounded_reference_and_rejects_two_ulps():
    x, w, dy = _rms_inputs((3, 264), 10, CPU)
    ref = rms_ref(x, w, 1e-5, dy)
    check_bf16(_rne(ref["y"]), ref["y"], 0.0, "y")
    check_bf16(_rne(ref["dx"]), ref["dx"], ref["a_dx"], "dx")
    bad = _rne(ref["y"]).clone()
    bits = bad.view(torch.int16)
    bits[1, 100] += 2                      # two bf16 ulps
    with pytest.raises(AssertionError):
        check_bf16(bad, ref["y"], 0.0, "y")
    with pytest.raises(AssertionError):    # nan never passes
        bad2 = _rne(ref["y"]).clone()
        bad2[0, 0] = float("nan")
        check_bf16(bad2, ref["y"], 0.0, "y")
    # subnormal bf16: the rounded reference passes, two steps off does not
    tiny = torch.tensor([-3.43430469604038e-39, 5e-40], dtype=torch.float64)
    check_bf16(_rne(tiny), tiny)
    with pytest.raises(AssertionError):
        check_bf16(_rne(tiny + 2.5 * BF16_SUBNORMAL_STEP), tiny)
    # beyond the bf16 range: inf of the right sign only
    big = torch.tensor([1e39, -1e39], dtype=torch.float64)
    check_bf16(torch.tensor([math.inf, -math.inf]).bfloat16(), big)
    with pytest.raises(AssertionError):
        check_bf16(torch.tensor([-math.inf, -math.inf]).bfloat16(), big)


def test_rms_reference_matches_autograd():
    x, w, dy = _rms_inputs((5, 64), 11, CPU)
    xd = x.double().requires_grad_()
    wd = w.double().requires_grad_()
    y = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-3) * wd
    y.backward(dy.double())
    ref = rms_ref(x, w, 1e-3, dy)
    assert torch.allclose(ref["y"], y.detach(), rtol=1e-12, atol=0)
    assert torch.allclose(ref["dx"], xd.grad, rtol=1e-10, atol=1e-14)
    assert torch.allclose(ref["dw"], wd.grad, rtol=1e-10, atol=1e-14)


def test_rms_dw_bound_rejects_missing_row_chunk():
    N, H = 130, 264
    x, w, dy = _rms_inputs((N, H), 12, CPU)
    ref = rms_ref(x, w, 1e-5, dy)
    check_sum_bf16(_rne(ref["dw"]), ref["dw"], ref["dw_terms"], N, "dw")
    # row_splits = 2, chunk = 65: the second block's rows never added
    partial = ref["prod"][:65].sum(0)
    with pytest.raises(AssertionError):
        check_sum_bf16(_rne(partial), ref["dw"], ref["dw_terms"], N, "dw")


def test_swiglu_reference_matches_autograd():
    a = _randn((64,), 13, CPU).double().requires_grad_()
    b = _randn((64,), 14, CPU).double().requires_grad_()
    dy = _randn((64,), 15, CPU).double()
    (F.silu(a) * b).backward(dy)
    ref = swiglu_ref(a.detach(), b.detach(), dy)
    assert torch.allclose(ref["y"], (F.silu(a) * b).detach(), rtol=1e-12)
    assert torch.allclose(ref["da"], a.grad, rtol=1e-10, atol=1e-14)
    assert torch.allclose(ref["db"], b.grad, rtol=1e-10, atol=1e-14)


def test_rope_reference_is_a_rotation_and_backward_its_inverse():
    B, T, Hn, D = 2, 5, 3, 32
    cosT, sinT = ops.rope_tables(T + 7, D)
    x = _randn((B, T, Hn, D), 16, CPU)
    y, a = rope_ref64(x, cosT[7:], sinT[7:])
    assert torch.allclose(y, ops.rope_ref(x.double(), cosT[7:].double(),
                                          sinT[7:].double()), rtol=1e-12)
    back, _ = rope_ref64(y, cosT[7:], sinT[7:], sign=-1)
    assert torch.allclose(back, x.double(), atol=1e-6)   # fp32 tables
    check_bf16(_rne(y), y, a, "rope")
    # a forward rotation is not the backward one
    with pytest.raises(AssertionError):
        check_bf16(_rne(y), rope_ref64(x, cosT[7:], sinT[7:], sign=-1)[0], a)


def test_ce_reference_and_lse_defect():
    N, V = 3, 1001
    logits = _ce_logits(N, V, "randn", 17, CPU)
    tgt = _ce_targets(N, V, 0, CPU)                 # 0, V-1, V8-1
    loss, mx, lse, t_loss, t_lse = ce_rows(logits, tgt)
    want = F.cross_entropy(logits.double(), tgt, reduction="none")
    assert torch.allclose(loss, want, rtol=1e-12)
    loss32, _, lse32, _, _ = ce_rows(logits, tgt, torch.float32)
    check_f32(lse.float(), lse, lse32, t_lse, "lse")
    check_f32(loss.float(), loss, loss32, t_loss, "loss")
    # the last 8 columns left out of the sum
    short = torch.logsumexp(logits.double()[:, :V - 8], -1)
    with pytest.raises(AssertionError):
        check_f32(short.float(), lse, lse32, t_lse, "lse")
    # constant rows: loss = log V whatever the constant
    const = _ce_logits(N, V, "const", 18, CPU)
    assert torch.allclose(ce_rows(const, tgt)[0],
                          torch.full((N,), math.log(V), dtype=torch.float64))
    # ignored rows and the mean over valid rows
    tgt2 = torch.tensor([5, -100, 7])
    m, _ = ce_mean(logits, tgt2)
    assert ce_rows(logits, tgt2)[0][1] == 0
    assert torch.allclose(m, F.cross_entropy(logits.double(), tgt2,
                                             ignore_index=-100))
    assert ce_mean(logits, torch.full((N,), -100))[0] == 0


def test_ce_dlogits_reference_and_onehot_defect():
    N, V = 3, 1001
    logits = _ce_logits(N, V, "randn", 19, CPU)
    tgt = torch.tensor([0, -100, 991])
    ld = logits.double().requires_grad_()
    (3.5 * F.cross_entropy(ld, tgt, ignore_index=-100)).backward()
    ref, a = ce_dlogits_ref(logits, tgt, 3.5)
    assert torch.allclose(ref, ld.grad, rtol=1e-10, atol=1e-16)
    assert (ref[1] == 0).all()
    check_bf16(_rne(ref), ref, a, "dlogits")
    shifted, _ = ce_dlogits_ref(logits, tgt, 3.5, shift=1)
    with pytest.raises(AssertionError):
        check_bf16(_rne(shifted), ref, a, "dlogits")


def test_adamw_reference_matches_torch_optimizer():
    p0 = _randn((50,), 20, CPU, dtype=torch.float64)
    pt = p0.clone().requires_grad_()
    opt = torch.optim.AdamW([pt], lr=1e-2, betas=(0.9, 0.95), eps=1e-8,
                            weight_decay=0.1)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for t in range(1, 4):
        g = _randn((50,), 20 + t, CPU, dtype=torch.float64)
        pt.grad = g / 64
        opt.step()
        p, m, v, terms = adamw_formula(p, g, m, v, 1e-2, 0.9, 0.95, 1e-8,
                                       0.1, t, 1 / 64)
    assert torch.allclose(p, pt.detach(), rtol=1e-9, atol=1e-12)
    p32 = p.float()
    check_f32(p32, p, p32, terms["p"], "adamw p")


def test_adamw_bound_rejects_a_wrong_power():
    """The step-1000 case: bias correction with t - 1 in place of t."""
    p0 = _randn((1000,), 500, CPU).float()
    g = _randn((1000,), 501, CPU).float()
    z = torch.zeros(1000)
    args = (LR, *BETAS_EXACT, EPS, 0.1)
    p, _, _, terms = adamw_formula(p0.double(), g.double(), z.double(),
                                   z.double(), *args, 1000, 1.0)
    p32 = adamw_formula(p0, g, z, z, *args, 1000, 1.0)[0]
    check_f32(p.float(), p, p32, terms["p"], "adamw t=1000")
    off = adamw_formula(p0.double(), g.double(), z.double(), z.double(),
                        *args, 999, 1.0)[0]
    with pytest.raises(AssertionError):
        check_f32(off.float(), p, p32, terms["p"], "adamw t=999")


def test_gemv_bound_rejects_the_other_rows_x():
    x = _randn((2, 512), 21, CPU)
    w = _randn((5, 512), 22, CPU)
    ref, terms = gemv_ref(x, w)
    check_sum_bf16(_rne(ref), ref, terms, 512, "gemv")
    swapped = _rne(ref).clone()
    swapped[0] = _rne(ref)[1]              # row 0 computed from x[1]
    with pytest.raises(AssertionError):
        check_sum_bf16(swapped, ref, terms, 512, "gemv")


def test_gae_reference_matches_scalar_loop():
    T, B = 7, 5
    _, r, v, cont = _scan_inputs(T, B, 23, CPU, torch.float64)
    for gamma, lam in ((0.9, 0.8), (0.99, 0.0), (0.99, 1.0)):
        adv, vt, tadv, _ = gae_scan(r, v, cont, gamma, lam)
        adv_o, vt_o = ops.gae_ref(r, v, cont, gamma, lam)
        for b in range(B):
            run = 0.0
            for t in reversed(range(T)):
                c = cont[t, b].item()
                delta = r[t, b].item() + gamma * c * v[t + 1, b].item() \
                    - v[t, b].item()
                run = delta + gamma * lam * c * run
                assert abs(adv[t, b].item() - run) < 1e-12
                assert abs(adv_o[t, b].item() - run) < 1e-12
                assert abs(vt[t, b].item() - run - v[t, b].item()) < 1e-12
        assert (tadv >= adv.abs() - 1e-12).all()


def _clip_fractions_ok(log_rhos):
    rhos = log_rhos.double().exp()
    for c in VTRACE_CLIPS.values():
        frac = (rhos > c).double().mean().item()
        assert 0.1 <= frac <= 0.9, (c, frac)


def test_vtrace_reference_matches_scalar_loop_and_clip_swap_is_caught():
    T, B = 7, 257
    f32 = _scan_inputs(T, B, 24, CPU)
    lr_, r, v, cont = [t.double() for t in f32]
    _clip_fractions_ok(lr_)
    gamma, (rc, cc, pc) = 0.99, VTRACE_CLIPS.values()
    vs, pg, tvs, tpg = vtrace_scan(lr_, r, v, cont, gamma, rc, cc, pc)
    vs_o, pg_o = ops.vtrace_ref(lr_, r, v, cont, gamma, rc, cc, pc)
    for b in range(0, B, 16):
        vs_l = [0.0] * (T + 1)
        vs_l[T] = v[T, b].item()
        for t in reversed(range(T)):
            ratio = math.exp(lr_[t, b].item())
            c = cont[t, b].item()
            delta = min(rc, ratio) * (r[t, b].item()
                                      + gamma * c * v[t + 1, b].item()
                                      - v[t, b].item())
            vs_l[t] = v[t, b].item() + delta + gamma * c * min(cc, ratio) * (
                vs_l[t + 1] - v[t + 1, b].item())
        for t in range(T):
            ratio = math.exp(lr_[t, b].item())
            pg_l = min(pc, ratio) * (r[t, b].item() + gamma * cont[t, b].item()
                                     * vs_l[t + 1] - v[t, b].item())
            assert abs(vs[t, b].item() - vs_l[t]) < 1e-10
            assert abs(vs_o[t, b].item() - vs_l[t]) < 1e-10
            assert abs(pg[t, b].item() - pg_l) < 1e-10
            assert abs(pg_o[t, b].item() - pg_l) < 1e-10
    # the helper passes an fp32 evaluation and fails swapped clips
    vs32, pg32, _, _ = vtrace_scan(*f32, gamma, rc, cc, pc)
    check_f32(vs.float(), vs, vs32, tvs, "vs")
    check_f32(pg.float(), pg, pg32, tpg, "pg")
    vs_sw, pg_sw, _, _ = vtrace_scan(lr_, r, v, cont, gamma, cc, rc, pc)
    with pytest.raises(AssertionError):
        check_f32(vs_sw.float(), vs, vs32, tvs, "vs")
    with pytest.raises(AssertionError):
        check_f32(pg_sw.float(), pg, pg32, tpg, "pg")


def test_img_reference_and_nhwc_defect():
    x, mean, std = _img_inputs((2, 5, 7, 3), 25, CPU)
    ref = img_ref(x, mean, std)
    assert ref.shape == (2, 3, 5, 7)
    assert abs(ref[1, 2, 4, 6].item()
               - (x[1, 4, 6, 2].item() / 255 - 0.406) / 0.225) < 1e-12
    check_bf16(_rne(ref), ref, 1e-6, "img")
    nhwc = ref.permute(0, 2, 3, 1).contiguous().view(ref.shape)
    with pytest.raises(AssertionError):
        check_bf16(_rne(nhwc), ref, 1e-6, "img")


# --------------------------------------------------------------------------
# RMSNorm
# --------------------------------------------------------------------------


def _rms_check(x, w, dy, eps, tag, x_leaf=None, to_leaf=None):
    """Forward, inv, dx and dw of ops.rmsnorm against fp64. `x_leaf` is the
    tensor whose .grad receives dx when x is a view of it; `to_leaf` maps the
    reference dx into the leaf's layout."""
    ref = rms_ref(x, w, eps, dy)
    leaf = x_leaf if x_leaf is not None else x
    leaf.requires_grad_(True)
    wl = w.detach().clone().requires_grad_(True)
    xin = x if x_leaf is None else to_leaf(leaf)
    y = ops.rmsnorm(xin, wl, eps)
    assert y.shape == x.shape
    check_bf16(y.detach(), ref["y"], 0.0, tag + " y")
    y.backward(dy)
    dx_ref, a_dx = ref["dx"], ref["a_dx"]
    if x_leaf is not None:
        dx_ref, a_dx = to_leaf(dx_ref), to_leaf(a_dx)
    check_bf16(leaf.grad, dx_ref, a_dx, tag + " dx")
    N = x.numel() // x.shape[-1]
    check_sum_bf16(wl.grad, ref["dw"], ref["dw_terms"], N, tag + " dw")
    _, inv = ops._K.rmsnorm_fwd(x.detach().contiguous(), w, eps)
    inv32 = rms_ref(x, w, eps, dtype=torch.float32)["inv"]
    check_f32(inv, ref["inv"], inv32, ref["inv"].abs(), tag + " inv")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [
    (1, 8),            # one lane
    (3, 264),          # partial last column tile
    (64, 2048),        # exactly one full pass, row_splits 1
    (130, 2056),       # thread 0 alone takes a second pass; chunks of 65
    (129, 4096),       # the model's H; chunks of 65 and 64
    (16448, 256),      # row_splits capped at 256, blocks 254/255 empty
    (2, 5, 264),       # 3-D input
])
def test_rmsnorm_shapes(shape):
    dev = _gpu()
    x, w, dy = _rms_inputs(shape, 100, dev)
    _rms_check(x, w, dy, 1e-5, f"rmsnorm {shape}")


@pytest.mark.gpu
def test_rmsnorm_noncontiguous_x_and_dy():
    dev = _gpu()
    _, w, dy = _rms_inputs((3, 264), 110, dev)
    base = _randn((264, 3), 111, dev)
    assert not base.t().is_contiguous()
    # backward used to raise here: forward saved the view, not the copy
    _rms_check(base.detach().t(), w, dy, 1e-5, "rmsnorm x.t()",
               x_leaf=base, to_leaf=lambda t: t.t())
    x = _randn((3, 264), 112, dev)
    dyt = _randn((264, 3), 113, dev).t()
    assert not dyt.is_contiguous()
    _rms_check(x, w, dyt, 1e-5, "rmsnorm dy.t()")


@pytest.mark.gpu
@pytest.mark.parametrize("eps", [1e-5, 1e-2])
def test_rmsnorm_eps_and_zero_row(eps):
    dev = _gpu()
    x, w, dy = _rms_inputs((3, 264), 120, dev)
    x[1] = 0
    _rms_check(x, w, dy, eps, f"rmsnorm eps={eps}")
    xl = x.detach().clone().requires_grad_(True)
    y = ops.rmsnorm(xl, w, eps)
    y.backward(dy)
    assert (y[1] == 0).all()
    assert torch.isfinite(xl.grad).all()
    want = dy[1].double() * w.double() / math.sqrt(eps)
    check_bf16(xl.grad[1], want, 2.0 ** -20 * want.abs(), "zero row dx")


@pytest.mark.gpu
@pytest.mark.parametrize("exp", [-40, 40])
def test_rmsnorm_scaled_inputs(exp):
    dev = _gpu()
    x, w, dy = _rms_inputs((3, 264), 130, dev, xscale=2.0 ** exp)
    _rms_check(x, w, dy, 1e-5, f"rmsnorm x*2^{exp}")


@pytest.mark.gpu
def test_rmsnorm_fp32_weight_raises_or_matches():
    """An fp32 weight used to be read as bf16 bit patterns."""
    dev = _gpu()
    x, _, dy = _rms_inputs((3, 264), 140, dev)
    w32 = _randn((264,), 141, dev, dtype=torch.float32)
    assert not torch.equal(w32, w32.bfloat16().float())
    wb = w32.bfloat16()
    _, inv = ops._K.rmsnorm_fwd(x, wb, 1e-5)
    with pytest.raises(RuntimeError, match="bf16"):
        ops._K.rmsnorm_fwd(x, w32, 1e-5)
    with pytest.raises(RuntimeError, match="bf16"):
        ops._K.rmsnorm_fwd(x.float(), wb, 1e-5)
    for bad in ((dy, x, w32), (dy.float(), x, wb), (dy, x.float(), wb)):
        with pytest.raises(RuntimeError, match="bf16"):
            ops._K.rmsnorm_bwd(*bad, inv)
    with pytest.raises(RuntimeError):       # H % 8 in backward too
        ops._K.rmsnorm_bwd(dy[:, :260].contiguous(), x[:, :260].contiguous(),
                           wb[:260].contiguous(), inv)
    try:
        y = ops.rmsnorm(x, w32, 1e-5)
    except RuntimeError:
        return
    check_bf16(y, rms_ref(x, w32, 1e-5)["y"], 0.0, "rmsnorm fp32 w")
    mod = ops.RMSNorm(264, dtype=torch.float32).to(dev)
    check_bf16(mod(x), rms_ref(x, mod.weight.detach(), 1e-5)["y"], 0.0, "mod")


# --------------------------------------------------------------------------
# SwiGLU
# --------------------------------------------------------------------------


def _swiglu_check(a, b, dy, tag):
    ref = swiglu_ref(a, b, dy)
    al = a.detach().clone().requires_grad_(True)
    bl = b.detach().clone().requires_grad_(True)
    y = ops.swiglu(al, bl)
    check_bf16(y.detach(), ref["y"], ref["a_y"], tag + " y")
    y.backward(dy)
    check_bf16(al.grad, ref["da"], ref["a_da"], tag + " da")
    check_bf16(bl.grad, ref["db"], ref["a_db"], tag + " db")


@pytest.mark.gpu
@pytest.mark.parametrize("numel", [8, 8 * (2048 * 256 + 3)])
def test_swiglu_sizes(numel):
    dev = _gpu()
    a = _randn((numel,), 200, dev, 3.0)
    b = _randn((numel,), 201, dev)
    dy = _randn((numel,), 202, dev)
    _swiglu_check(a, b, dy, f"swiglu n={numel}")


@pytest.mark.gpu
def test_swiglu_every_finite_bf16_a():
    dev = _gpu()
    bits = torch.arange(-32768, 32768, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]           # drop inf / nan
    assert bits.numel() == 65280
    pats = bits.to(torch.int16).view(torch.bfloat16)
    vals = torch.tensor([1, -1, 3.5, -3.5, 2.0 ** -20, -2.0 ** -20,
                         2.0 ** 20, -2.0 ** 20], dtype=torch.bfloat16)
    a = pats.repeat(8)
    b = vals.repeat_interleave(65280)                # every (a, b) pair
    dy = vals[torch.randint(0, 8, (a.numel(),), generator=_gen(203))]
    _swiglu_check(a.to(dev), b.to(dev), dy.to(dev), "swiglu all-a")


# --------------------------------------------------------------------------
# RoPE
# --------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [
    (2, 16, 4, 128),     # model head dim, B > 1 so sr % T matters
    (1, 1, 1, 64),
    (3, 5, 1, 32),
    (2, 520, 8, 128),    # more than 2048*256 pairs
])
@pytest.mark.parametrize("offset", [0, 7])
def test_rope_forward_backward(shape, offset):
    dev = _gpu()
    B, T, Hn, D = shape
    cosF, sinF = ops.rope_tables(T + offset, D, device=dev)
    cosT, sinT = cosF[offset:offset + T], sinF[offset:offset + T]
    x = _randn(shape, 300, dev).requires_grad_(True)
    g = _randn(shape, 301, dev)
    y = ops.rope(x, cosT, sinT)
    ref, a = rope_ref64(x.detach(), cosT, sinT)
    check_bf16(y.detach(), ref, a, f"rope {shape}+{offset}")
    y.backward(g)
    gref, ga = rope_ref64(g, cosT, sinT, sign=-1)
    check_bf16(x.grad, gref, ga, f"rope bwd {shape}+{offset}")


@pytest.mark.gpu
def test_rope_fused_qkv_slices():
    dev = _gpu()
    B, T, Hq, Hkv, D = 2, 16, 4, 2, 128
    cosT, sinT = ops.rope_tables(T, D, device=dev)
    fused = _randn((B, T, (Hq + 2 * Hkv) * D), 310, dev)
    fused[..., (Hq + Hkv) * D:] = float("nan")       # the v part
    fused.requires_grad_(True)
    q = fused[..., :Hq * D].view(B, T, Hq, D)
    k = fused[..., Hq * D:(Hq + Hkv) * D].view(B, T, Hkv, D)
    assert not q.is_contiguous() and not k.is_contiguous()
    yq, yk = ops.rope(q, cosT, sinT), ops.rope(k, cosT, sinT)
    assert yq.is_contiguous() and yk.is_contiguous()
    assert torch.isfinite(yq).all() and torch.isfinite(yk).all()
    rq, aq = rope_ref64(q.detach(), cosT, sinT)
    rk, ak = rope_ref64(k.detach(), cosT, sinT)
    check_bf16(yq.detach(), rq, aq, "rope fused q")
    check_bf16(yk.detach(), rk, ak, "rope fused k")
    gq, gk = _randn(yq.shape, 311, dev), _randn(yk.shape, 312, dev)
    torch.autograd.backward([yq, yk], [gq, gk])
    grad = fused.grad
    rgq, agq = rope_ref64(gq, cosT, sinT, sign=-1)
    rgk, agk = rope_ref64(gk, cosT, sinT, sign=-1)
    check_bf16(grad[..., :Hq * D].reshape(B, T, Hq, D), rgq, agq, "dq")
    check_bf16(grad[..., Hq * D:(Hq + Hkv) * D].reshape(B, T, Hkv, D), rgk,
               agk, "dk")
    assert (grad[..., (Hq + Hkv) * D:] == 0).all()


# --------------------------------------------------------------------------
# Cross entropy
# --------------------------------------------------------------------------

CE_SHAPES = [(1, 8), (3, 7), (3, 1001), (5, 2048), (5, 2056), (4, 4107),
             (2, 128256)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CE_KINDS)
@pytest.mark.parametrize("N,V", CE_SHAPES)
def test_cross_entropy(N, V, kind):
    """Per-row loss / mx / lse, the mean loss and dlogits. Row r of
    rotation `rot` takes target choice (r + rot) of 0, V-1, V8-1, V8 (where
    it exists) and -100, so every row meets every target."""
    dev = _gpu()
    logits = _ce_logits(N, V, kind, 400 + V, dev)
    for rot in range(len(_ce_target_choices(V))):
        tag = f"ce ({N},{V}) {kind} rot{rot}"
        tgt = _ce_targets(N, V, rot, dev)
        loss, mx, lse = ops._K.ce_fwd(logits, tgt.int())
        r_loss, r_mx, r_lse, t_loss, t_lse = ce_rows(logits, tgt)
        k_loss, _, k_lse, _, _ = ce_rows(logits, tgt, torch.float32)
        assert torch.equal(mx.double(), r_mx), tag
        check_f32(lse, r_lse, k_lse, t_lse, tag + " lse")
        check_f32(loss, r_loss, k_loss, t_loss, tag + " loss")

        ll = logits.detach().clone().requires_grad_(True)
        mean = ops.cross_entropy(ll, tgt)
        r_mean, t_mean = ce_mean(logits, tgt)
        k_mean, _ = ce_mean(logits, tgt, torch.float32)
        check_f32(mean.detach(), r_mean, k_mean, t_mean, tag + " mean")
        (3.5 * mean).backward()
        ref, a = ce_dlogits_ref(logits, tgt, 3.5)
        check_bf16(ll.grad, ref, a, tag + " dlogits")
        assert (ll.grad[tgt < 0] == 0).all(), tag


@pytest.mark.gpu
def test_cross_entropy_all_ignored():
    dev = _gpu()
    logits = _ce_logits(5, 2056, "randn", 410, dev).requires_grad_(True)
    tgt = torch.full((5,), -100, device=dev)
    loss = ops.cross_entropy(logits, tgt)
    assert loss.item() == 0.0
    (3.5 * loss).backward()
    assert (logits.grad == 0).all()


def _chunked_torch_bf16(x, w, t, chunk):
    """ops.lm_head_cross_entropy step for step, with torch ops in place of
    the CE kernels: bf16 logits, fp32 softmax, bf16 dlogits, bf16 GEMMs and
    the fp32 accumulation of the per-chunk dW."""
    N = x.shape[0]
    nvalid = (t >= 0).sum().clamp(min=1).float()
    loss = torch.zeros((), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    dw = torch.zeros_like(w, dtype=torch.float32)
    for s in range(0, N, chunk):
        e = min(s + chunk, N)
        lg = (x[s:e] @ w.t()).float()
        tt = t[s:e]
        valid = tt >= 0
        lse = torch.logsumexp(lg, -1)
        xt = lg.gather(1, tt.clamp(min=0)[:, None])[:, 0]
        loss += torch.where(valid, lse - xt, torch.zeros_like(lse)).sum()
        p = torch.softmax(lg, -1)
        p[valid.nonzero()[:, 0], tt[valid]] -= 1.0
        dl = (p * (valid.float() / nvalid)[:, None]).to(x.dtype)
        dx[s:e] = dl @ w
        dw += (dl.t() @ x[s:e]).float()
    return loss / nvalid, dx, dw.to(w.dtype)


@pytest.mark.gpu
def test_lm_head_cross_entropy_against_fp64():
    dev = _gpu()
    N, H, V, chunk = 600, 256, 1000, 256
    x = _randn((N, H), 420, dev)
    w = _randn((V, H), 421, dev, 0.05)
    t = torch.randint(0, V, (N,), generator=_gen(422)).to(dev)
    t[::7] = -100
    t[256:512] = -100                 # one whole chunk ignored
    x1 = x.clone().requires_grad_(True)
    w1 = w.clone().requires_grad_(True)
    loss = ops.lm_head_cross_entropy(x1, w1, t, chunk_rows=chunk)
    loss.backward()

    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    ref = F.cross_entropy(xd @ wd.t(), t, ignore_index=-100)
    ref.backward()
    t_loss, t_dx, t_dw = _chunked_torch_bf16(x, w, t, chunk)

    _, terms = ce_mean(xd.detach() @ wd.detach().t(), t)
    e_ours = abs(loss.item() - ref.item())
    e_torch = abs(t_loss.item() - ref.item())
    print(f"lm_head loss err ours {e_ours:.3e} torch {e_torch:.3e}")
    assert e_ours <= 1.1 * e_torch + F32_FLOOR * terms.item()
    assert (x1.grad[256:512] == 0).all()
    for name, got, theirs, want in (("dx", x1.grad, t_dx, xd.grad),
                                    ("dW", w1.grad, t_dw, wd.grad)):
        ours, them = _errs(got, want), _errs(theirs, want)
        print(f"lm_head {name}: rel ours {ours[0]:.3e} torch {them[0]:.3e} | "
              f"max ours {ours[1]:.3e} torch {them[1]:.3e}")
        assert ours[0] <= 1.1 * them[0], (name, ours, them)
        assert ours[1] <= 1.1 * them[1], (name, ours, them)


# --------------------------------------------------------------------------
# AdamW
# --------------------------------------------------------------------------

ADAMW_N = [1, 1000, 2048 * 256 + 5]


def _adamw_run(dev, n, dtype, scale, wd, betas=(0.9, 0.95), t0=0, steps=5):
    tag = f"adamw {str(dtype)[6:]} n={n} scale={scale} wd={wd} t0={t0}"
    p = _randn((n,), 500, dev, dtype=dtype).requires_grad_(True)
    opt = ops.FusedAdamW([p], lr=LR, betas=betas, eps=EPS, weight_decay=wd)
    opt.t = t0
    st = opt.state[id(p)]
    bf = dtype == torch.bfloat16
    r = [p.detach().double(), torch.zeros(n, dtype=torch.float64, device=dev),
         torch.zeros(n, dtype=torch.float64, device=dev)]
    k = [t.float() for t in r]
    terms = {"m": None, "p": None}
    for step in range(1, steps + 1):
        g = _randn((n,), 500 + step, dev, dtype=dtype)
        p.grad = g.clone()
        opt.step(grad_scale=scale)
        args = (LR, betas[0], betas[1], EPS, wd, t0 + step, scale)
        *r, terms = adamw_formula(r[0], g.double(), r[1], r[2], *args,
                                  tm=terms["m"], tp=terms["p"])
        k = adamw_formula(k[0], g.float(), k[1], k[2], *args)[:3]
        stag = f"{tag} step{step}"
        got_p = st["master"] if bf else p.detach()
        check_f32(got_p, r[0], k[0], terms["p"], stag + " p")
        check_f32(st["m"], r[1], k[1], terms["m"], stag + " m")
        check_f32(st["v"], r[2], k[2], terms["v"], stag + " v")
        if bf:
            assert torch.equal(p.detach().view(torch.int16),
                               st["master"].bfloat16().view(torch.int16)), stag
            check_bf16(p.detach(), r[0], 2.0 ** -20 * terms["p"], stag + " bf")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("scale,wd", [(1.0, 0.0), (1 / 64, 0.1), (1.0, 0.1),
                                      (1 / 64, 0.0)])
@pytest.mark.parametrize("n", ADAMW_N)
def test_adamw_steps(n, scale, wd, dtype):
    _adamw_run(_gpu(), n, dtype, scale, wd)


@pytest.mark.gpu
def test_adamw_bf16_bias_correction_at_step_1000():
    """t = 1000 with beta2 = 1 - 2^-10: 1 - beta2^t = 0.62, so a wrong power
    shows in p (test_adamw_bound_rejects_a_wrong_power)."""
    _adamw_run(_gpu(), 1000, torch.bfloat16, 1.0, 0.1, betas=BETAS_EXACT,
               t0=999, steps=1)


# --------------------------------------------------------------------------
# GEMV
# --------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", [(1, 512), (5, 512), (4097, 1024),
                                 (16389, 512)])   # the last: > 4096 blocks
def test_gemv_direct(N, K):
    dev = _gpu()
    w = _randn((N, K), 600, dev, 0.05)
    for B in (1, 2, 3, 8):
        x = _randn((B, K), 601 + B, dev)
        y = ops._K.gemv(x, w)
        ref, terms = gemv_ref(x, w)
        check_sum_bf16(y, ref, terms, K, f"gemv B={B} ({N},{K})")


class _Spy:
    def __init__(self, real):
        self._real = real
        self.calls = []

    def gemv(self, x, w):
        self.calls.append((tuple(x.shape), tuple(w.shape)))
        return self._real.gemv(x, w)

    def __getattr__(self, name):
        return getattr(self._real, name)


@pytest.mark.gpu
def test_linear_sb_dispatch(monkeypatch):
    dev = _gpu()
    spy = _Spy(ops._K)
    monkeypatch.setattr(ops, "_K", spy)
    w = _randn((8192, 4096), 610, dev, 0.02)
    with torch.no_grad():
        for rows in (1, 2):
            x = _randn((rows, 1, 4096), 611 + rows, dev)
            spy.calls.clear()
            y = ops.linear_sb(x, w)
            assert spy.calls == [((rows, 4096), (8192, 4096))]
            assert y.shape == (rows, 1, 8192)
            ref, terms = gemv_ref(x.view(rows, 4096), w)
            check_sum_bf16(y.view(rows, 8192), ref, terms, 4096,
                           f"linear_sb rows={rows}")
        spy.calls.clear()
        x3 = _randn((3, 1, 4096), 620, dev)
        assert torch.equal(ops.linear_sb(x3, w), F.linear(x3, w))    # rows = 3
        x1 = _randn((1, 1, 4096), 621, dev)
        wn = _randn((8196, 4096), 622, dev, 0.02)
        assert torch.equal(ops.linear_sb(x1, wn), F.linear(x1, wn))  # N
        xk = _randn((1, 1, 4352), 623, dev)
        wk = _randn((8192, 4352), 624, dev, 0.02)
        assert torch.equal(ops.linear_sb(xk, wk), F.linear(xk, wk))  # K % 512
    assert torch.equal(ops.linear_sb(x1, w), F.linear(x1, w))        # grad on
    assert spy.calls == []


# --------------------------------------------------------------------------
# GAE and V-trace
# --------------------------------------------------------------------------

SCAN_SHAPES = [(1, 1), (7, 257), (128, 300)]


@pytest.mark.gpu
@pytest.mark.parametrize("gamma,lam", [(0.9, 0.8), (0.99, 0.0), (0.99, 1.0)])
@pytest.mark.parametrize("T,B", SCAN_SHAPES)
def test_gae(T, B, gamma, lam):
    dev = _gpu()
    _, r, v, cont = _scan_inputs(T, B, 700, dev)
    assert T == 1 or (cont[0] == 0).any() and (cont[T - 1] == 0).any()
    adv, vt = ops.gae(r, v, cont, gamma, lam)
    ra, rv, ta, tv = gae_scan(r.double(), v.double(), cont.double(), gamma, lam)
    ka, kv, _, _ = gae_scan(r, v, cont, gamma, lam)
    tag = f"gae ({T},{B}) g={gamma} l={lam}"
    check_f32(adv, ra, ka, ta, tag + " adv")
    check_f32(vt, rv, kv, tv, tag + " vtarg")


@pytest.mark.gpu
@pytest.mark.parametrize("T,B", SCAN_SHAPES)
def test_vtrace_distinct_clips(T, B):
    dev = _gpu()
    lr_, r, v, cont = _scan_inputs(T, B, 710, dev)
    if T * B >= 100:      # a single element cannot be on both sides
        _clip_fractions_ok(lr_)
    rc, cc, pc = VTRACE_CLIPS.values()
    vs, pg = ops.vtrace(lr_, r, v, cont, 0.99, rc, cc, pc)
    d = [t.double() for t in (lr_, r, v, cont)]
    rvs, rpg, tvs, tpg = vtrace_scan(*d, 0.99, rc, cc, pc)
    kvs, kpg, _, _ = vtrace_scan(lr_, r, v, cont, 0.99, rc, cc, pc)
    check_f32(vs, rvs, kvs, tvs, f"vtrace ({T},{B}) vs")
    check_f32(pg, rpg, kpg, tpg, f"vtrace ({T},{B}) pg")


# --------------------------------------------------------------------------
# image normalize
# --------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1, 1, 3), (2, 5, 7, 3), (1, 3, 3, 1),
                                   (1, 2, 2, 4), (4, 224, 224, 3)])
def test_img_normalize_shapes(shape):
    dev = _gpu()
    x, mean, std = _img_inputs(shape, 800, dev)
    assert mean.dtype == torch.float64
    y = ops.img_normalize(x, mean, std)
    check_bf16(y, img_ref(x, mean, std), 1e-6, f"img {shape}")


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3, 4])
def test_img_normalize_every_byte_value(C):
    dev = _gpu()
    _, mean, std = _img_inputs((1, 16, 16, C), 801, dev)
    x = torch.arange(256, dtype=torch.uint8, device=dev).view(1, 16, 16, 1)
    x = x.expand(1, 16, 16, C).contiguous()
    y = ops.img_normalize(x, mean, std)
    check_bf16(y, img_ref(x, mean, std), 1e-6, f"img bytes C={C}")
