"""Batched per-row LoRA kernels (csrc/hip/lora.hip): against the fp64
reference, exact slot routing, untouched rows, determinism and graph
replay under a changing adapter mix."""
import functools

import pytest
import torch

from ray_amd import ops

pytestmark = pytest.mark.gpu

S = 4
SCALE = [0.5, 1.0, -2.0, 1.0]


def _dev():
    return torch.device("cuda", 0)


def _nan_framed(t):
    """t on the GPU as the inner rows of a buffer whose first and last rows
    are NaN."""
    buf = torch.full((t.shape[0] + 2, *t.shape[1:]), float("nan"),
                     dtype=t.dtype)
    buf[1:-1] = t
    return buf.to(_dev())[1:-1]


@functools.lru_cache(maxsize=None)
def _case(M, N, K, R):
    """Operands (x and y0 in NaN-framed buffers, x NaN where idx is -1), the
    fp64 reference and the bound: one bf16 rounding of the result, one of h,
    fp32 accumulation in both products."""
    g = torch.Generator().manual_seed(10000 * M + 10 * N + K + R)
    idx = torch.tensor([2, -1, 0, 2, 3])[torch.arange(M) % 5].int()
    x = torch.randn(M, K, generator=g).bfloat16()
    x[idx < 0] = float("nan")
    A = torch.randn(S, R, K, generator=g).bfloat16()
    B = torch.randn(S, N, R, generator=g).bfloat16()
    y0 = (torch.randn(M, N, generator=g) * K ** 0.5).bfloat16()
    scale = torch.tensor(SCALE)
    ref = ops.lora_ref(y0, x, A, B, scale, idx)
    on = idx >= 0
    s = idx[on].long()
    xd, Ad, Bd = x[on].double(), A[s].double(), B[s].double()
    h = torch.einsum("mk,mrk->mr", xd, Ad)
    habs = torch.einsum("mk,mrk->mr", xd.abs(), Ad.abs())
    bound = 2.0 ** -8 * ref[on].abs() + scale[s].abs().double()[:, None] * (
        2.0 ** -8 * torch.einsum("mr,mnr->mn", h.abs(), Bd.abs())
        + (K + R) * 2.0 ** -23 * torch.einsum("mr,mnr->mn", habs, Bd.abs()))
    # A skipped row or a wrong slot cannot pass: the adapter moves every row
    # by more than the bound in most of its elements. The delta of an element
    # is about |s| sqrt(K R) |z| with z standard normal, and the bound's
    # rounding-of-h term alone is 2^-8 * 0.64 sqrt(R) of that scale (0.02 at
    # R = 64), the fp32 term another 0.64 (K + R) 2^-23 sqrt(K R) (0.04 at
    # K = 2176, R = 64): P(|z| < 0.07) is 5.6%, so with these inputs and
    # this bound the share is 94% to 99% (measured: 0.942 to 0.993), not the
    # 99% first asked for. Asserted: over 90% overall, and in every row at
    # least one element (a skipped row needs all of them inside the bound).
    delta = (ref[on] - y0[on].double()).abs()
    assert (delta > bound).double().mean() > 0.9
    assert (delta > bound).any(dim=1).all()
    d = _dev()
    return (_nan_framed(x), A.to(d), B.to(d), scale.to(d), idx.to(d), y0,
            ref, bound, on)


# 17: a second group of 16 rows of one adapter; 65: a second row chunk.
# (128, 128): one K step, so forced splits leave empty slices; (384, 2176):
# uneven slices and three column tiles.
@pytest.mark.parametrize("split", [0, 1, 4])
@pytest.mark.parametrize("R", [16, 32, 64])
@pytest.mark.parametrize("N,K", [(128, 128), (384, 2176)])
@pytest.mark.parametrize("M", [1, 17, 65])
def test_kernel_against_fp64_reference(M, N, K, R, split):
    x, A, B, scale, idx, y0, ref, bound, on = _case(M, N, K, R)
    y = _nan_framed(y0)
    with torch.no_grad():
        out = ops._K.lora_add(y, x, A, B, scale, idx, split=split)
    assert out.data_ptr() == y.data_ptr()
    y = y.cpu()
    assert torch.equal(y[~on].view(torch.int16), y0[~on].view(torch.int16))
    err = (y[on].double() - ref[on]).abs()
    print(f"max err/bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), (err - bound).max()


def test_slots_route_exactly():
    """x is the identity, so row m of y is scale * B[s] A[s][:, m] for the
    row's own slot s = m % S: integers below 2^8 times a power of two, exact
    in bf16."""
    M = K = N = 128
    R = 16
    g = torch.Generator().manual_seed(7)
    A = torch.randint(-2, 3, (S, R, K), generator=g).float()
    B = torch.randint(-2, 3, (S, N, R), generator=g).float()
    scale = torch.tensor([2.0, 0.5, -4.0, 1.0])
    idx = (torch.arange(M) % S).int()
    want = torch.stack([scale[m % S] * (B[m % S] @ A[m % S][:, m])
                        for m in range(M)])
    assert len({want[m].numpy().tobytes() for m in range(S)}) == S
    d = _dev()
    y = torch.zeros(M, N, dtype=torch.bfloat16, device=d)
    with torch.no_grad():
        ops.lora_add(y, torch.eye(K, dtype=torch.bfloat16, device=d),
                     A.bfloat16().to(d), B.bfloat16().to(d), scale.to(d),
                     idx.to(d))
    assert torch.equal(y.float().cpu(), want)


@pytest.mark.parametrize("M", [1, 65])
def test_rows_without_adapter_are_untouched(M):
    d = _dev()
    y0 = torch.randn(M, 128).bfloat16()
    y = _nan_framed(y0)
    nan = float("nan")
    with torch.no_grad():
        ops.lora_add(y, torch.full((M, 128), nan, dtype=torch.bfloat16,
                                   device=d),
                     torch.full((S, 16, 128), nan, dtype=torch.bfloat16,
                                device=d),
                     torch.full((S, 128, 16), nan, dtype=torch.bfloat16,
                                device=d),
                     torch.ones(S, device=d),
                     torch.full((M,), -1, dtype=torch.int32, device=d))
    assert torch.equal(y.cpu().view(torch.int16), y0.view(torch.int16))


def test_deterministic_and_graph_replay_with_changing_mix():
    """Two eager calls are bit-equal; one captured call serves other mixes
    of adapters (idx changes in place) and other inputs, bit-equal to eager."""
    x, A, B, scale, idx, y0, _, _, _ = _case(65, 384, 2176, 32)
    x = torch.nan_to_num(x)
    y0 = y0.to(_dev())

    def eager(x_, idx_, split=4):
        return ops._K.lora_add(y0.clone(), x_, A, B, scale, idx_,
                                split=split)

    with torch.no_grad():
        assert torch.equal(eager(x, idx, 0), eager(x, idx, 0))
        xs, ys, ids = x.clone(), y0.clone(), idx.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops._K.lora_add(ys, xs, A, B, scale, ids, split=4)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ops._K.lora_add(ys, xs, A, B, scale, ids, split=4)
        mixes = [idx, torch.full_like(idx, 3), idx.flip(0),
                 torch.full_like(idx, -1)]
        for k, mix in zip((1.0, -0.5, 2.0, 1.0), mixes):
            xs.copy_(x * k)
            ids.copy_(mix)
            ys.copy_(y0)
            graph.replay()
            assert torch.equal(ys, eager(xs, ids))
