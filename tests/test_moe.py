"""Mixture-of-experts FFN (csrc/hip/moe.hip): the router and the routed
expert kernels against float64 references of the same bf16 inputs."""
import functools

import pytest
import torch

from ray_amd import ops

gpu = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _inputs(M, H, I, E):
    """x ~ N(0,1), weights ~ N(0,1) fan_in^-1/2, a residual, all bf16."""
    g = torch.Generator().manual_seed(0)

    def rnd(*shape, fan_in=1):
        return (torch.randn(*shape, generator=g) * fan_in ** -0.5).bfloat16()

    return (rnd(M, H), rnd(E, H, fan_in=H), rnd(E, I, H, fan_in=H),
            rnd(E, I, H, fan_in=H), rnd(E, H, I, fan_in=I), rnd(M, H))


def _route_case(M, H, E, k, tie=False):
    x, Wr = _inputs(M, H, 128, E)[:2]
    if tie:
        Wr = Wr.clone()
        Wr[5] = Wr[3]
    idx, w = ops.moe_route(x.to(_dev()), Wr.to(_dev()), k)
    assert idx.dtype == torch.int32 and w.dtype == torch.float32
    return x, Wr, idx.cpu().long(), w.cpu().double()


@gpu
@pytest.mark.parametrize("M,H,E,k", [(1, 256, 8, 2), (200, 256, 8, 2),
                                     (200, 384, 64, 8), (65, 256, 4, 1),
                                     (200, 256, 8, 8)])
def test_route(M, H, E, k):
    x, Wr, idx, w = _route_case(M, H, E, k)
    ridx, rw = ops.moe_route_ref(x, Wr, k)
    logits = x.double() @ Wr.double().t()
    S = (x.double().abs() @ Wr.double().abs().t()).amax(dim=1)
    keep = torch.ones(M, dtype=torch.bool)
    if k < E:
        top = logits.sort(dim=1, descending=True).values
        keep = (top[:, k - 1] - top[:, k]) >= 2 * H * 2.0 ** -24 * S
    print(f"moe_route M={M} H={H} E={E} k={k}: {int((~keep).sum())} rows "
          "left out")
    assert (~keep).sum() <= 0.01 * M
    assert (idx >= 0).all() and (idx < E).all()
    assert torch.equal(idx.sort(dim=1).values[keep],
                       ridx.long().sort(dim=1).values[keep])
    by_expert = torch.zeros(M, E, dtype=torch.float64)
    got, ref = by_expert.scatter(1, idx, w), by_expert.scatter(1, ridx.long(),
                                                               rw)
    bound = (k * H * 2.0 ** -24 * S + 2.0 ** -20)[:, None]
    assert ((got - ref).abs() <= bound)[keep].all()
    assert ((w.sum(dim=1) - 1).abs() <= 2.0 ** -20 * k).all()
    # slot order: descending logits
    assert (w[:, :-1] >= w[:, 1:]).all()


@gpu
def test_route_tie_goes_to_lower_index():
    _, _, idx, _ = _route_case(200, 256, 8, 2, tie=True)
    has3, has5 = (idx == 3).any(dim=1), (idx == 5).any(dim=1)
    assert (has3 & ~has5).any()      # the tie sat at the boundary
    assert not (has5 & ~has3).any()
    both = has3 & has5
    assert both.any()
    assert ((idx[both] == 3).int().argmax(dim=1)
            < (idx[both] == 5).int().argmax(dim=1)).all()


def _routing(kind, M, E, k):
    g = torch.Generator().manual_seed(1)
    idx = torch.rand(M, E, generator=g).argsort(dim=1)[:, :k]
    if kind == "same2":        # six empty experts, 13 tiles on each of two
        idx = torch.tensor([[2, 5]]).repeat(M, 1)
    elif kind == "one":        # exactly M pairs on expert 3
        idx = torch.stack([torch.full((M,), 3),
                           torch.arange(M) % 7 + (torch.arange(M) % 7 >= 3)],
                          dim=1)
    w = torch.softmax(torch.randn(M, k, generator=g), dim=1)
    return idx.int(), w


def _experts_reference(x, idx, w, Wg, Wu, Wd):
    """float64 y and A = sum_j w_j |h_j| |Wd_e|^T, h exact."""
    y = ops.moe_experts_ref(x, idx, w, Wg, Wu, Wd)
    xd, A = x.double(), torch.zeros(x.shape, dtype=torch.float64)
    for j in range(idx.shape[1]):
        e = idx[:, j].long()
        h = (torch.nn.functional.silu(
            torch.einsum("mh,mih->mi", xd, Wg[e].double()))
            * torch.einsum("mh,mih->mi", xd, Wu[e].double()))
        A += w[:, j:j + 1].double() * torch.einsum(
            "mi,mhi->mh", h.abs(), Wd[e].double().abs())
    return y, A


def _check_experts(name, y, x, idx, w, Wg, Wu, Wd, r=None):
    ref, A = _experts_reference(x, idx, w, Wg, Wu, Wd)
    bound = 2.0 ** -8 * (ref.abs() + A)
    if r is not None:
        ref = ref + r.double()
        bound = 2.0 ** -8 * (ref.abs() + A) + 2.0 ** -8 * r.double().abs()
    ratio = ((y.cpu().double() - ref).abs() / bound).max().item()
    print(f"moe_experts {name}: max error/bound {ratio:.3f}")
    assert ratio <= 1.0


SHAPES = [(256, 256), (256, 384), (384, 128)]
EXPERT_CASES = (
    [(f"M{M}", M, *SHAPES[i % 3], 8, 2, "random", False)
     for i, M in enumerate((1, 5, 16, 17, 64, 65, 200))]
    + [("k1", 33, 256, 384, 8, 1, "random", False),
       ("k4", 33, 384, 128, 8, 4, "random", False),
       ("same2", 200, 256, 256, 8, 2, "same2", False),
       ("one16", 16, 256, 384, 8, 2, "one", False),
       ("one17", 17, 384, 128, 8, 2, "one", False),
       ("E64k8", 33, 256, 256, 64, 8, "random", False),
       ("residual", 65, 256, 384, 8, 2, "random", True)])


@gpu
@pytest.mark.parametrize("name,M,H,I,E,k,kind,res", EXPERT_CASES,
                         ids=[c[0] for c in EXPERT_CASES])
def test_experts(name, M, H, I, E, k, kind, res):
    x, _, Wg, Wu, Wd, r = _inputs(M, H, I, E)
    idx, w = _routing(kind, M, E, k)
    d = _dev()
    args = [t.to(d) for t in (x, idx, w, Wg, Wu, Wd)]
    rd = r.to(d) if res else None
    y = ops.moe_experts(*args, residual=rd)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape
    _check_experts(name, y, x, idx, w, Wg, Wu, Wd, r if res else None)
    assert torch.equal(y, ops.moe_experts(*args, residual=rd))


@gpu
def test_ffn_is_route_then_experts():
    x, Wr, Wg, Wu, Wd, r = (t.to(_dev()) for t in _inputs(65, 256, 384, 8))
    y = ops.moe_ffn(x, Wr, Wg, Wu, Wd, 2, residual=r)
    idx, w = ops.moe_route(x, Wr, 2)
    assert torch.equal(y, ops.moe_experts(x, idx, w, Wg, Wu, Wd, residual=r))
    assert torch.equal(y, ops.moe_ffn(x, Wr, Wg, Wu, Wd, 2, residual=r))


@pytest.mark.parametrize("H,E,k", [(200, 8, 2), (256, 8, 9), (256, 4, 5),
                                   (256, 65, 2)])
def test_unsupported_shapes_raise(H, E, k):
    x, Wr = torch.zeros(4, H).bfloat16(), torch.zeros(E, H).bfloat16()
    Wg, Wd = torch.zeros(E, 128, H).bfloat16(), torch.zeros(E, H, 128).bfloat16()
    with pytest.raises(ValueError):
        ops.moe_route(x, Wr, k)
    with pytest.raises(ValueError):
        ops.moe_ffn(x, Wr, Wg, Wg, Wd, k)


def test_cpu_path_matches_reference():
    x, Wr, Wg, Wu, Wd, r = _inputs(65, 256, 384, 8)
    idx, w = ops.moe_route(x, Wr, 2)
    y = ops.moe_ffn(x, Wr, Wg, Wu, Wd, 2, residual=r)
    assert y.dtype == torch.bfloat16
    _check_experts("cpu", y, x, idx, w, Wg, Wu, Wd, r)
