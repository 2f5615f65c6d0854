"""ops.add_rmsnorm (residual add + RMSNorm as one op) and the one-pass
RMSNorm backward (csrc/hip/rmsnorm.hip), and the model paths built on them.

What must be bit-equal, and why it can be: s = bf16(x + r) is torch's bf16
add; the norm is computed from the rounded s with the per-thread summation
order of rmsnorm_fwd_bf16; dx uses the expression and the summation order of
rmsnorm_bwd_dx_bf16 (`_K.rmsnorm_bwd_two_pass`, the kernels every earlier
revision ran); with a gradient of s the kernel stores
bf16(float(bf16(dx)) + float(g_s)), the double rounding of torch's add.

dw is the one thing whose bits move: the one-pass kernel sums the same fp32
terms dy*x*inv in another order (per-block partials over rows b, b+grid, ...,
then a fixed-order sum over blocks) than the two-pass kernel (row ranges,
then atomics). Bounds, against an fp64 reference from the same bf16 inputs,
at every shape (N = 1, 3, 257, 2049 x H = 8, 256, 2056, 4096):
  * relative L2 and max-abs error each at most 2x what
    `rmsnorm_bwd_two_pass` shows on the same inputs. The errors of the two
    orders differ by rounding noise, not systematically. With up to four
    rows the one-pass kernel runs one block, whose per-column fma chain adds
    the rows in the order of the two-pass kernel's single row split, so the
    two are then equal.
  * the worst-case bound of an n-term fp32 sum as well,
    |dw - ref| <= n 2^-24 sum|terms| + 2^-20 sum|terms| (the second part is
    the fp32 inv that both kernels are handed).
Measured pairs (MI355X) are in PERFORMANCE.md.
"""
import pytest
import torch

from ray_amd import ops
from ray_amd.models.llama import LlamaConfig, LlamaModel

EPS = 1e-5


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if not ops.HAVE_HIP_OPS:
        raise RuntimeError("HIP extension not built")
    return torch.device("cuda")


def _randn(shape, seed, dev, scale=1.0, dtype=torch.bfloat16):
    g = torch.Generator()
    g.manual_seed(seed)
    t = torch.randn(shape, generator=g, dtype=torch.float32) * scale
    return t.to(dtype).to(dev)


def _grid():
    return int(ops._K.rmsnorm_bwd_grid)


# rows N = 1, 3, 257, 2 * grid + 1: fewer than blocks, a ragged last sweep,
# more than one sweep
_INPUTS = {}


def _inputs(N, H, dev):
    """Seeded x, r, w, g_h, g_s for one shape; made once and never written."""
    key = (N, H)
    if key not in _INPUTS:
        seed = 1000 * N + H
        _INPUTS[key] = (
            _randn((N, H), seed, dev), _randn((N, H), seed + 1, dev),
            _randn((H,), seed + 2, dev, dtype=torch.float32).add_(1.0)
            .bfloat16(),
            _randn((N, H), seed + 3, dev), _randn((N, H), seed + 4, dev))
    return _INPUTS[key]


def _composed(x, r, w, g_h, g_s):
    """x + r, then ops.rmsnorm: (s, h, dx, dr, dw)."""
    xl = x.clone().requires_grad_(True)
    rl = r.clone().requires_grad_(True)
    wl = w.clone().requires_grad_(True)
    s = xl + rl
    h = ops.rmsnorm(s, wl, EPS)
    if g_s is None:
        h.backward(g_h)
    else:
        torch.autograd.backward([h, s], [g_h, g_s])
    return s.detach(), h.detach(), xl.grad, rl.grad, wl.grad


def _fused(x, r, w, g_h, g_s):
    xl = x.clone().requires_grad_(True)
    rl = r.clone().requires_grad_(True)
    wl = w.clone().requires_grad_(True)
    s, h = ops.add_rmsnorm(xl, rl, wl, EPS)
    if g_s is None:
        h.backward(g_h)
    else:
        torch.autograd.backward([h, s], [g_h, g_s])
    return s.detach(), h.detach(), xl.grad, rl.grad, wl.grad


@pytest.mark.gpu
@pytest.mark.parametrize("H", [8, 256, 2056, 4096])
@pytest.mark.parametrize("N", [1, 3, 257, 2049])
def test_add_rmsnorm_equals_add_then_rmsnorm(N, H):
    dev = _gpu()
    assert 2049 == 2 * _grid() + 1, "rows must cover more than two sweeps"
    x, r, w, g_h, g_s = _inputs(N, H, dev)
    for gs in (None, g_s):
        want = _composed(x, r, w, g_h, gs)
        got = _fused(x, r, w, g_h, gs)
        for name, a, b in zip(("s", "h", "dx", "dr", "dw"), got, want):
            assert torch.equal(a, b), (name, N, H, gs is not None)
    # the norm's own dx keeps the bits of the two-pass kernels
    s = (x + r).contiguous()
    _, inv = ops._K.rmsnorm_fwd(s, w, EPS)
    dx2, _ = ops._K.rmsnorm_bwd_two_pass(g_h, s, w, inv)
    dx1, _ = ops._K.rmsnorm_bwd(g_h, s, w, inv)
    assert torch.equal(dx1, dx2), ("dx vs two-pass", N, H)
    dxr, _ = ops._K.rmsnorm_bwd_res(g_h, s, w, inv, g_s)
    assert torch.equal(dxr, dx2 + g_s), ("dx + g_s vs torch add", N, H)


def _dw_errors(dw, ref):
    d = dw.double() - ref
    return (d.norm() / ref.norm()).item(), d.abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("H", [8, 256, 2056, 4096])
@pytest.mark.parametrize("N", [1, 3, 257, 2049])
def test_dw_deterministic_and_as_accurate_as_two_pass(N, H):
    dev = _gpu()
    x, r, w, g_h, _ = _inputs(N, H, dev)
    s = (x + r).contiguous()
    _, inv = ops._K.rmsnorm_fwd(s, w, EPS)
    _, dw_a = ops._K.rmsnorm_bwd(g_h, s, w, inv)
    _, dw_b = ops._K.rmsnorm_bwd(g_h, s, w, inv)
    assert dw_a.dtype == torch.float32 and dw_a.shape == (H,)
    assert torch.equal(dw_a, dw_b), "dw differs between two calls"
    _, dw_old = ops._K.rmsnorm_bwd_two_pass(g_h, s, w, inv)
    sd = s.double()
    inv64 = torch.rsqrt(sd.pow(2).mean(-1, keepdim=True) + EPS)
    terms = g_h.double() * sd * inv64
    ref = terms.sum(0)
    bound = (N * 2.0 ** -24 + 2.0 ** -20) * terms.abs().sum(0)
    assert ((dw_a.double() - ref).abs() <= bound).all(), (N, H)
    new_l2, new_max = _dw_errors(dw_a, ref)
    old_l2, old_max = _dw_errors(dw_old, ref)
    print(f"dw N={N} H={H}: rel L2 {new_l2:.3e} / {old_l2:.3e}, "
          f"max abs {new_max:.3e} / {old_max:.3e} (one-pass / two-pass)")
    assert new_l2 <= 2 * old_l2, (N, H, new_l2, old_l2)
    assert new_max <= 2 * old_max, (N, H, new_max, old_max)


@pytest.mark.gpu
def test_wide_h_takes_the_two_pass_kernels():
    """H > 8192 is beyond the one-pass template: add kernel + rmsnorm_fwd
    forward, two-pass backward + add kernel. Same contract."""
    dev = _gpu()
    N, H = 3, 8200
    x, r, w, g_h, g_s = _inputs(N, H, dev)
    for gs in (None, g_s):
        want = _composed(x, r, w, g_h, gs)
        got = _fused(x, r, w, g_h, gs)
        for name, a, b in zip(("s", "h", "dx", "dr"), got, want):
            assert torch.equal(a, b), (name, gs is not None)
        # dw: a single row split, so the two-pass kernel is deterministic
        assert torch.equal(got[4], want[4])
    s = (x + r).contiguous()
    _, inv = ops._K.rmsnorm_fwd(s, w, EPS)
    before = g_s.clone()
    dxr, _ = ops._K.rmsnorm_bwd_res(g_h, s, w, inv, g_s)
    dx2, _ = ops._K.rmsnorm_bwd_two_pass(g_h, s, w, inv)
    assert torch.equal(dxr, dx2 + g_s) and torch.equal(g_s, before)


@pytest.mark.gpu
def test_add_rmsnorm_3d_and_noncontiguous():
    dev = _gpu()
    x, r, w, g_h, g_s = _inputs(257, 256, dev)
    x3, r3 = x[:256].view(2, 128, 256), r[:256].view(2, 128, 256)
    s, h = ops.add_rmsnorm(x3, r3, w, EPS)
    assert s.shape == h.shape == x3.shape
    assert torch.equal(s, x3 + r3)
    assert torch.equal(h, ops.rmsnorm(x3 + r3, w, EPS))
    xt = x[:256].t()                       # a non-contiguous operand
    s, h = ops.add_rmsnorm(xt, r[:256], w, EPS)
    assert torch.equal(s, xt + r[:256])
    assert torch.equal(h, ops.rmsnorm(xt + r[:256], w, EPS))
    with pytest.raises(RuntimeError, match="bf16"):
        ops._K.add_rmsnorm_fwd(x.float(), r, w, EPS)
    with pytest.raises(RuntimeError):
        ops._K.add_rmsnorm_fwd(x, r[:3], w, EPS)


def test_add_rmsnorm_cpu_is_add_then_rmsnorm():
    x = _randn((5, 64), 1, "cpu", dtype=torch.float32).requires_grad_(True)
    r = _randn((5, 64), 2, "cpu", dtype=torch.float32).requires_grad_(True)
    w = _randn((64,), 3, "cpu", dtype=torch.float32).requires_grad_(True)
    s, h = ops.add_rmsnorm(x, r, w, EPS)
    assert torch.equal(s, x + r)
    assert torch.equal(h, ops.rmsnorm(x + r, w, EPS))
    (h.sum() + 2 * s.sum()).backward()
    got = [t.grad.clone() for t in (x, r, w)]
    for t in (x, r, w):
        t.grad = None
    s2 = x + r
    (ops.rmsnorm(s2, w, EPS).sum() + 2 * s2.sum()).backward()
    for a, t in zip(got, (x, r, w)):
        assert torch.equal(a, t.grad)


# --------------------------------------------------------------------------
# the model: fused paths against today's composition
# --------------------------------------------------------------------------

_CFG = LlamaConfig(vocab_size=512, hidden_size=512, intermediate_size=1024,
                   num_layers=2, num_heads=4, num_kv_heads=2, max_seq_len=256)


def _model_grads(monkeypatch, dev, dtype, fused, checkpoint=False, T=256):
    monkeypatch.setattr(ops, "_FUSED_QKV_ATTN", fused)
    monkeypatch.setattr(ops, "_FUSED_ADD_NORM", fused)
    torch.manual_seed(7)
    model = LlamaModel(_CFG, dtype=dtype, gradient_checkpointing=checkpoint)
    model = model.to(dev)
    g = torch.Generator()
    g.manual_seed(8)
    tokens = torch.randint(0, _CFG.vocab_size, (2, T), generator=g).to(dev)
    targets = torch.randint(0, _CFG.vocab_size, (2, T), generator=g).to(dev)
    loss = model(tokens, targets)
    loss.backward()
    return loss.detach(), {n: p.grad for n, p in model.named_parameters()}


_MODEL_REF = {}


def _model_reference(monkeypatch, dev):
    if "ref" not in _MODEL_REF:
        _MODEL_REF["ref"] = _model_grads(monkeypatch, dev, torch.bfloat16,
                                         False)
    return _MODEL_REF["ref"]


@pytest.mark.gpu
@pytest.mark.parametrize("checkpoint", [False, True])
def test_model_fused_paths_equal_composition(monkeypatch, checkpoint):
    dev = _gpu()
    loss0, grads0 = _model_reference(monkeypatch, dev)
    loss1, grads1 = _model_grads(monkeypatch, dev, torch.bfloat16, True,
                                 checkpoint)
    assert torch.equal(loss0, loss1)
    assert grads0.keys() == grads1.keys()
    for n in grads0:
        assert grads1[n] is not None, n
        assert torch.equal(grads0[n], grads1[n]), n


def test_model_fp32_cpu_new_path_equals_old(monkeypatch):
    loss0, grads0 = _model_grads(monkeypatch, "cpu", torch.float32, False,
                                 T=32)
    loss1, grads1 = _model_grads(monkeypatch, "cpu", torch.float32, True,
                                 T=32)
    assert torch.equal(loss0, loss1)
    for n in grads0:
        assert torch.equal(grads0[n], grads1[n]), n
