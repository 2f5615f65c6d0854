"""Routed expert kernels over MXFP4 expert weights (csrc/hip/moe_w4.hip)
against the float64 reference on the dequantised weights: quantisation error
is not in the comparison, the bound is that of tests/test_moe.py."""
import functools

import pytest
import torch

from ray_amd import ops

gpu = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _inputs(M, H, I, E):
    """x ~ N(0,1), weights ~ N(0,1) fan_in^-1/2 in bf16, then MXFP4: returns
    x, router, the three (wq, scales), their exact dequantised values, r."""
    g = torch.Generator().manual_seed(0)

    def rnd(*shape, fan_in=1):
        return (torch.randn(*shape, generator=g) * fan_in ** -0.5).bfloat16()

    x, Wr = rnd(M, H), rnd(E, H, fan_in=H)
    q = [ops.quantize_expert_weights_mxfp4(w) for w in (
        rnd(E, I, H, fan_in=H), rnd(E, I, H, fan_in=H), rnd(E, H, I, fan_in=I))]
    deq = [ops.dequantize_mxfp4(wq.flatten(0, 1), s.flatten(0, 1),
                                torch.bfloat16).view(E, wq.shape[1], -1)
           for wq, s in q]
    return x, Wr, q, deq, rnd(M, H)


def _routing(kind, M, E, k):
    g = torch.Generator().manual_seed(1)
    idx = torch.rand(M, E, generator=g).argsort(dim=1)[:, :k]
    if kind == "same2":        # six empty experts, many groups on two
        idx = torch.tensor([[2, 5]]).repeat(M, 1)
    elif kind == "one":        # exactly M pairs on expert 3
        idx = torch.stack([torch.full((M,), 3),
                           torch.arange(M) % 7 + (torch.arange(M) % 7 >= 3)],
                          dim=1)
    w = torch.softmax(torch.randn(M, k, generator=g), dim=1)
    return idx.int(), w


def _check(name, y, x, idx, w, deq, r=None):
    """|y - ref| <= 2^-8 (|ref| + A) + 2^-8 |r|, A = sum_j w_j |h_j| |Wd_e|^T
    in float64 on the dequantised weights."""
    Wg, Wu, Wd = deq
    ref = ops.moe_experts_ref(x, idx, w, Wg, Wu, Wd)
    xd, A = x.double(), torch.zeros(x.shape, dtype=torch.float64)
    for j in range(idx.shape[1]):
        e = idx[:, j].long()
        h = (torch.nn.functional.silu(
            torch.einsum("mh,mih->mi", xd, Wg[e].double()))
            * torch.einsum("mh,mih->mi", xd, Wu[e].double()))
        A += w[:, j:j + 1].double() * torch.einsum(
            "mi,mhi->mh", h.abs(), Wd[e].double().abs())
    bound = 2.0 ** -8 * (ref.abs() + A)
    if r is not None:
        ref = ref + r.double()
        bound = 2.0 ** -8 * (ref.abs() + A) + 2.0 ** -8 * r.double().abs()
    ratio = ((y.cpu().double() - ref).abs() / bound).max().item()
    print(f"moe_experts mxfp4 {name}: max error/bound {ratio:.3f}")
    assert ratio <= 1.0


def _device_args(x, idx, w, q):
    (gq, gs), (uq, us), (dq, ds) = q
    args = [t.to(DEV) for t in (x, idx, w, gq, uq, dq)]
    return args, tuple(t.to(DEV) for t in (gs, us, ds))


SHAPES = [(256, 384), (384, 128), (256, 256)]
CASES = (
    [(f"M{M}-{H}x{I}", M, H, I, 8, 2, "random", False)
     for M in (1, 5, 16, 17, 64, 65, 200) for H, I in SHAPES]
    + [("k1", 33, 256, 384, 8, 1, "random", False),
       ("k4", 33, 384, 128, 8, 4, "random", False),
       ("same2", 200, 256, 256, 8, 2, "same2", False),
       ("one16", 16, 256, 384, 8, 2, "one", False),
       ("one17", 17, 384, 128, 8, 2, "one", False),
       ("E64k8", 33, 256, 256, 64, 8, "random", False),
       ("residual", 65, 256, 384, 8, 2, "random", True)])


@gpu
@pytest.mark.parametrize("name,M,H,I,E,k,kind,res", CASES,
                         ids=[c[0] for c in CASES])
def test_experts(name, M, H, I, E, k, kind, res):
    x, _, q, deq, r = _inputs(M, H, I, E)
    idx, w = _routing(kind, M, E, k)
    args, scales = _device_args(x, idx, w, q)
    rd = r.to(DEV) if res else None
    y = ops.moe_experts(*args, residual=rd, scales=scales)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape
    _check(name, y, x, idx, w, deq, r if res else None)
    assert torch.equal(y, ops.moe_experts(*args, residual=rd, scales=scales))


@gpu
@pytest.mark.parametrize("M", [1, 65])
def test_every_split_gives_the_same_bits(M):
    # I = 1024: the smallest at which each of the 8 tree groups holds a step
    x, _, q, deq, _ = _inputs(M, 256, 1024, 8)
    idx, w = _routing("random", M, 8, 2)
    args, scales = _device_args(x, idx, w, q)
    ys = [ops.moe_experts(*args, scales=scales, split=s)
          for s in (1, 2, 4, 8, 0)]
    _check(f"split M{M}", ys[0], x, idx, w, deq)
    for y in ys[1:]:
        assert torch.equal(y, ys[0])


@gpu
def test_ffn_is_route_then_experts():
    x, Wr, q, _, r = _inputs(65, 256, 384, 8)
    x, Wr, r = (t.to(DEV) for t in (x, Wr, r))
    (gq, gs), (uq, us), (dq, ds) = [[t.to(DEV) for t in p] for p in q]
    scales = (gs, us, ds)
    y = ops.moe_ffn(x, Wr, gq, uq, dq, 2, residual=r, scales=scales)
    idx, w = ops.moe_route(x, Wr, 2)
    assert torch.equal(y, ops.moe_experts(x, idx, w, gq, uq, dq, residual=r,
                                          scales=scales))


def test_cpu_path_and_malformed_shapes():
    x, Wr, q, deq, r = _inputs(65, 256, 384, 8)
    (gq, gs), (uq, us), (dq, ds) = q
    idx, w = ops.moe_route(x, Wr, 2)
    y = ops.moe_ffn(x, Wr, gq, uq, dq, 2, residual=r, scales=(gs, us, ds))
    assert y.dtype == torch.bfloat16
    _check("cpu", y, x, idx, w, deq, r)
    for bad in (dict(w_gate=gq[:, :, :64]),            # wrong K/2
                dict(scales=(gs, us[:, :, :4], ds)),   # wrong scale shape
                dict(scales=(gs, us))):                # two scales
        kw = dict(w_gate=gq, w_up=uq, w_down=dq, scales=(gs, us, ds))
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.moe_ffn(x, Wr, top_k=2, **kw)
