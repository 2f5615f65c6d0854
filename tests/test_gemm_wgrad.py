"""gemm_wgrad (csrc/hip/gemm_wgrad.hip): dW[N,K] = dy^T x in bf16, and its
wiring into ops.linear / ops.Linear / ops.swiglu_mlp_in and the Llama model.

Numerics bound: the kernel and torch's bf16 `dy.t() @ x` both accumulate in
fp32 and round once to bf16, so both errors against the fp32 reference are
the bf16 rounding (~1e-3 relative). The kernel must be within 1.1x of torch's
own error on every shape, for both metrics.
"""
import os

import pytest
import torch
import torch.nn.functional as F

from ray_amd import ops

G = ops.WGRAD_M_GRANULE

# (M tokens, N, K)
SHAPES = [
    (G, 256, 256),        # prologue + epilogue, no steady-state iteration
    (3 * G, 256, 256),    # three passes through the two-stage ring
    (1024, 512, 256),     # N != K
    (1024, 256, 512),
    (512, 768, 768),      # 9 blocks: > 8 and not a multiple of 8
]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if not ops.HAVE_HIP_OPS:
        raise RuntimeError("HIP extension not built")
    return torch.device("cuda")


def _randn(shape, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, device=dev,
                       dtype=torch.float32).to(torch.bfloat16)


def _errs(got, ref):
    got = got.float()
    rel = ((got - ref).norm() / ref.norm()).item()
    mx = ((got - ref).abs().max() / ref.abs().max()).item()
    return rel, mx


def _check_against_torch(dy, x, got, tag):
    ref = dy.float().t() @ x.float()
    ours = _errs(got, ref)
    theirs = _errs(dy.t() @ x, ref)
    print(f"gemm_wgrad {tag}: rel ours {ours[0]:.3e} torch {theirs[0]:.3e}"
          f" | maxabs/max|ref| ours {ours[1]:.3e} torch {theirs[1]:.3e}")
    assert ours[0] <= 1.1 * theirs[0], (tag, ours, theirs)
    assert ours[1] <= 1.1 * theirs[1], (tag, ours, theirs)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_numerics(M, N, K):
    dev = _gpu()
    dy = _randn((M, N), 1, dev)
    x = _randn((M, K), 2, dev)
    got = ops.gemm_wgrad(dy, x)
    assert got.shape == (N, K) and got.dtype == torch.bfloat16
    _check_against_torch(dy, x, got, f"({M},{N},{K})")


@pytest.mark.gpu
def test_column_slice_operands():
    """Row stride larger than the width: both operands are the column
    slice [:, 256:512] of a [512, 1024] tensor."""
    dev = _gpu()
    dy = _randn((512, 1024), 3, dev)[:, 256:512]
    x = _randn((512, 1024), 4, dev)[:, 256:512]
    assert dy.stride(0) == 1024 and not dy.is_contiguous()
    _check_against_torch(dy, x, ops.gemm_wgrad(dy, x), "slice")


@pytest.mark.gpu
def test_guard_bands():
    """NaN rows and columns around dy and x must never be read into the
    result, and a NaN-prefilled output larger than [N,K] must be written
    inside [N,K] only."""
    dev = _gpu()
    M, N, K = 256, 512, 256
    nan = float("nan")
    dyb = torch.full((M + 16, N + 512), nan, device=dev, dtype=torch.bfloat16)
    xb = torch.full((M + 16, K + 512), nan, device=dev, dtype=torch.bfloat16)
    dyb[8:8 + M, 256:256 + N] = _randn((M, N), 5, dev)
    xb[8:8 + M, 256:256 + K] = _randn((M, K), 6, dev)
    dy = dyb[8:8 + M, 256:256 + N]
    x = xb[8:8 + M, 256:256 + K]
    outb = torch.full((N + 16, K + 16), nan, device=dev, dtype=torch.bfloat16)
    out = outb[8:8 + N, 8:8 + K]
    ops.gemm_wgrad(dy, x, out=out)
    assert torch.isfinite(out).all()
    band = torch.ones_like(outb, dtype=torch.bool)
    band[8:8 + N, 8:8 + K] = False
    assert torch.isnan(outb[band]).all(), "wrote outside [N,K]"
    _check_against_torch(dy.contiguous(), x.contiguous(), out, "guard")


@pytest.mark.gpu
def test_repeatable():
    """20 calls on the same inputs are bitwise identical: the screen for a
    staged LDS buffer read before its DMA landed."""
    dev = _gpu()
    M, N, K = 1024, 768, 768
    dy = _randn((M, N), 7, dev)
    x = _randn((M, K), 8, dev)
    first = ops.gemm_wgrad(dy, x)
    _check_against_torch(dy, x, first, "repeat")
    for _ in range(19):
        assert torch.equal(ops.gemm_wgrad(dy, x), first)


@pytest.mark.gpu
def test_grouped_equals_single():
    dev = _gpu()
    M, N, K = 512, 768, 256
    dy0 = _randn((M, N), 9, dev)
    dy1 = _randn((M, N), 10, dev)
    x = _randn((M, K), 11, dev)
    o0, o1 = ops.gemm_wgrad_grouped(dy0, dy1, x)
    assert torch.equal(o0, ops.gemm_wgrad(dy0, x))
    assert torch.equal(o1, ops.gemm_wgrad(dy1, x))


@pytest.mark.gpu
def test_refuses_unqualified():
    dev = _gpu()
    x = _randn((256, 256), 12, dev)
    with pytest.raises(ValueError):
        ops.gemm_wgrad(_randn((256, 320), 13, dev), x)       # N % 256
    with pytest.raises(ValueError):
        ops.gemm_wgrad(_randn((192, 256), 13, dev), x[:192])  # M % 128
    with pytest.raises(ValueError):
        ops.gemm_wgrad(x.float(), x)                          # dtype


def _linear_pair(x, w, b, fn):
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    bb = None if b is None else b.detach().clone().requires_grad_(True)
    y = fn(x, w, bb)
    g = torch.Generator(device=x.device)
    g.manual_seed(99)
    dy = torch.randn(y.shape, generator=g, device=x.device,
                     dtype=torch.float32).to(y.dtype)
    y.backward(dy)
    return y, x.grad, w.grad, None if bb is None else bb.grad


def _assert_same_as_f_linear(x, w, b=None):
    got = _linear_pair(x, w, b, ops.linear)
    ref = _linear_pair(x, w, b, F.linear)
    for a, r in zip(got, ref):
        assert (a is None) == (r is None)
        if a is not None:
            assert torch.equal(a, r)


@pytest.mark.gpu
def test_dispatch_falls_back_to_torch(monkeypatch):
    dev = _gpu()
    monkeypatch.setattr(ops, "_WGRAD_FORCE", True)
    x = _randn((2, 128, 256), 20, dev)
    # misaligned N
    _assert_same_as_f_linear(x, _randn((320, 256), 21, dev))
    # fp32 weight (and input)
    _assert_same_as_f_linear(x.float(), _randn((256, 256), 22, dev).float())
    # bias
    _assert_same_as_f_linear(x, _randn((256, 256), 23, dev),
                             _randn((256,), 24, dev))
    # no_grad
    w = _randn((256, 256), 25, dev)
    with torch.no_grad():
        assert torch.equal(ops.linear(x, w), F.linear(x, w))
    # the switch restores the torch path bitwise
    monkeypatch.setenv("RAY_AMD_NO_WGRAD_GEMM", "1")
    _assert_same_as_f_linear(x, w)


@pytest.mark.gpu
def test_linear_uses_kernel_when_listed(monkeypatch):
    dev = _gpu()
    monkeypatch.setattr(ops, "_WGRAD_FORCE", True)
    x = _randn((2, 128, 256), 30, dev)
    w = _randn((512, 256), 31, dev)
    y, dx, dw, _ = _linear_pair(x, w, None, ops.linear)
    yr, dxr, dwr, _ = _linear_pair(x, w, None, F.linear)
    assert torch.equal(y, yr) and torch.equal(dx, dxr)
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    dy = torch.randn(y.shape, generator=g, device=dev,
                     dtype=torch.float32).to(y.dtype).reshape(-1, 512)
    assert torch.equal(dw, ops.gemm_wgrad(dy, x.reshape(-1, 256)))
    _check_against_torch(dy, x.reshape(-1, 256), dw, "linear")
    # weight only / input only
    xin = x.detach().clone().requires_grad_(True)
    ops.linear(xin, w.detach()).sum().backward()
    assert xin.grad is not None


def _tiny_grads(dev, dtype, checkpoint, tokens, targets, state=None):
    from ray_amd.models.llama import CONFIGS, LlamaModel

    torch.manual_seed(0)
    model = LlamaModel(CONFIGS["llama-tiny"], dtype=dtype,
                       gradient_checkpointing=checkpoint)
    if state is not None:
        model.load_state_dict(state)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    model.train()
    loss = model(tokens.to(dev), targets.to(dev))
    loss.backward()
    return loss.detach(), {n: p.grad.detach().float().cpu()
                           for n, p in model.named_parameters()}, sd


_E2E = {}


def _e2e_reference(dev):
    """Switched-off bf16 gradients and the fp32 (CPU) gradients, computed
    once and shared by the two end-to-end cases."""
    if not _E2E:
        g = torch.Generator()
        g.manual_seed(5)
        tokens = torch.randint(0, 512, (2, 128), generator=g)
        targets = torch.randint(0, 512, (2, 128), generator=g)
        os.environ["RAY_AMD_NO_WGRAD_GEMM"] = "1"
        try:
            loss_off, g_off, sd = _tiny_grads(dev, torch.bfloat16, False,
                                              tokens, targets)
        finally:
            del os.environ["RAY_AMD_NO_WGRAD_GEMM"]
        _, g32, _ = _tiny_grads(torch.device("cpu"), torch.float32, False,
                                tokens, targets, sd)
        _E2E.update(tokens=tokens, targets=targets, loss_off=loss_off,
                    g_off=g_off, g32=g32, sd=sd)
    return _E2E


@pytest.mark.gpu
@pytest.mark.parametrize("checkpoint", [False, True])
def test_llama_tiny_end_to_end(monkeypatch, checkpoint):
    dev = _gpu()
    monkeypatch.delenv("RAY_AMD_NO_WGRAD_GEMM", raising=False)
    ref = _e2e_reference(dev)
    monkeypatch.setattr(ops, "_WGRAD_FORCE", True)
    loss, grads, _ = _tiny_grads(dev, torch.bfloat16, checkpoint,
                                 ref["tokens"], ref["targets"], ref["sd"])
    assert torch.equal(loss, ref["loss_off"]), "forward must be unchanged"
    for name, g32 in ref["g32"].items():
        e_on = _errs(grads[name], g32)
        e_off = _errs(ref["g_off"][name], g32)
        assert e_on[0] <= 1.1 * e_off[0], (name, e_on, e_off)
        assert e_on[1] <= 1.1 * e_off[1], (name, e_on, e_off)


def test_cpu_linear_equals_nn_linear():
    torch.manual_seed(0)
    for dtype in (torch.float32, torch.bfloat16):
        a = ops.Linear(64, 48, bias=False, dtype=dtype)
        b = torch.nn.Linear(64, 48, bias=False, dtype=dtype)
        b.load_state_dict(a.state_dict())
        assert isinstance(a, torch.nn.Linear)
        assert list(a.state_dict()) == list(b.state_dict())
        x = torch.randn(3, 5, 64).to(dtype)
        xa = x.clone().requires_grad_(True)
        xb = x.clone().requires_grad_(True)
        ya, yb = a(xa), b(xb)
        assert torch.equal(ya, yb)
        dy = torch.randn(3, 5, 48).to(dtype)
        ya.backward(dy)
        yb.backward(dy)
        assert torch.equal(xa.grad, xb.grad)
        assert torch.equal(a.weight.grad, b.weight.grad)


def test_cpu_swiglu_mlp_in_equals_two_linears():
    torch.manual_seed(1)
    x = torch.randn(2, 7, 32, requires_grad=True)
    wg = torch.randn(48, 32, requires_grad=True)
    wu = torch.randn(48, 32, requires_grad=True)
    g, u = ops.swiglu_mlp_in(x, wg, wu)
    assert torch.equal(g, F.linear(x, wg)) and torch.equal(u, F.linear(x, wu))
