"""Attention backward with the key-on-lane dK/dV kernel (fa_bwd_dkv_v6)
and the 64-row split-staged dQ kernel (fa_bwd_dq_v5): numerics against the
fp32 autograd reference and against the recorded errors of the kernels they
replaced, exact zeros under a one-hot upstream gradient, run-to-run
repeatability and NaN guard bands around the inputs. The 128-row path
(T % 256 != 0) is checked forward and backward at more than one block."""
import functools

import pytest
import torch

from ray_amd import ops

D = 128
REL_BOUND = 0.03  # the project's ||ours - ref|| / ||ref|| bound

# (B, Hq, Hkv, T, bthd view, causal)
SHAPES = [
    # three key blocks (a wrong block-order mapping cannot cancel itself),
    # rep 4, batch stride
    (2, 8, 2, 768, True, True),
    # one all-diagonal block: every wave takes the masked path and the skip
    (1, 4, 4, 256, False, True),
    # mask off; an odd number of q tiles per buffer swap
    (1, 8, 2, 512, True, False),
    # rep 4 onto a single kv head; many tiles through the double buffer
    (2, 4, 1, 1024, False, True),
]

# ||grad - ref|| / ||ref|| (dq, dk, dv) of the kernels this path replaced,
# dq v4 + dkv v5, on the inputs of _case(shape). Recorded on an MI355X at
# commit 087f136, the last one that has those kernels (this test selected
# them there through environment switches), from the `old` column of
#   pytest tests/test_fa_bwd_v6.py -s -k no_worse_than_previous
# _case seeds the device generator, so the figures are reproducible.
OLD_REL_ERR = {
    SHAPES[0]: (2.7591e-03, 2.7294e-03, 2.5003e-03),
    SHAPES[1]: (2.7669e-03, 2.7945e-03, 2.4909e-03),
    SHAPES[2]: (2.6273e-03, 2.5648e-03, 2.6102e-03),
    SHAPES[3]: (2.7346e-03, 2.6785e-03, 2.5625e-03),
}

# The 128-row path (T % 256 != 0) at three key and three query blocks:
# diagonal and off-diagonal tiles, GQA rep 4 and a batch stride; run from
# contiguous BHTD tensors and from BTHD views, which are copied at this T.
# The last shape is the smallest at which the dK/dV kernel's staging and
# causal skip can go wrong: one key block, and per head a q-tile sequence of
# two tiles, so the flattened loop crosses a head boundary at every second
# tile.
SHAPES_128 = [
    (2, 8, 2, 384, False, True),
    (2, 8, 2, 384, True, True),
    (1, 4, 4, 384, False, False),
    (1, 4, 2, 128, False, True),
]


def _rand(B, H, T, bthd, gen):
    if bthd:
        t = torch.randn(B, T, H, D, device="cuda", dtype=torch.bfloat16,
                        generator=gen)
        return t.transpose(1, 2)
    return torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16,
                       generator=gen)


def _ref_grads(q, k, v, g, causal):
    q2 = q.detach().clone().requires_grad_()
    k2 = k.detach().clone().requires_grad_()
    v2 = v.detach().clone().requires_grad_()
    ref, _ = ops.flash_attention_ref(q2, k2, v2, causal=causal)
    ref.backward(g.float())
    return q2.grad.float(), k2.grad.float(), v2.grad.float()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs and fp32 reference gradients of one shape, computed once and
    shared (read-only) by the tests below."""
    B, Hq, Hkv, T, bthd, causal = shape
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234 + T + Hq)
    q = _rand(B, Hq, T, bthd, gen)
    k = _rand(B, Hkv, T, bthd, gen)
    v = _rand(B, Hkv, T, bthd, gen)
    g = _rand(B, Hq, T, bthd, gen)
    return q, k, v, g, _ref_grads(q, k, v, g, causal)


def _ours(q, k, v, g, causal):
    q1 = q.detach().requires_grad_()
    k1 = k.detach().requires_grad_()
    v1 = v.detach().requires_grad_()
    out = ops.flash_attention(q1, k1, v1, causal=causal)
    out.backward(g)
    return q1.grad, k1.grad, v1.grad


def _rel(ours, ref):
    return float((ours.float() - ref).norm() / (ref.norm() + 1e-6))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES,
                         ids=lambda s: "B%dHq%dHkv%dT%d" % s[:4])
def test_fa_bwd_v6_matches_fp32_reference(shape):
    q, k, v, g, refs = _case(shape)
    grads = _ours(q, k, v, g, shape[5])
    for name, ours, ref in zip(("dq", "dk", "dv"), grads, refs):
        assert torch.isfinite(ours).all(), (name, shape)
        rel = _rel(ours, ref)
        print(f"{shape} {name} rel {rel:.3e}")
        assert rel < REL_BOUND, (name, shape, rel)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%dHq%dHkv%dT%d" % s[:4])
def test_fa_bwd_v6_no_worse_than_previous_kernels(shape):
    """Old (dkv v5 + dq v4) and new kernels both round P and dS to bf16
    once and accumulate in f32; only the order of the f32 sums differs, so
    the new relative error may exceed the old (OLD_REL_ERR) by at most
    20 %."""
    q, k, v, g, refs = _case(shape)
    new = _ours(q, k, v, g, shape[5])
    for name, e_old, n, ref in zip(("dq", "dk", "dv"), OLD_REL_ERR[shape],
                                   new, refs):
        e_new = _rel(n, ref)
        print(f"{shape} {name} old {e_old:.4e} new {e_new:.4e}")
        assert e_new <= 1.2 * e_old, (name, shape, e_old, e_new)


@pytest.mark.gpu
@pytest.mark.parametrize(
    "shape", SHAPES_128,
    ids=lambda s: "B%dHq%dHkv%dT%d-%s-%s" % (
        s[:4] + ("bthd" if s[4] else "bhtd", "causal" if s[5] else "full")))
def test_fa_128_row_path_matches_fp32_reference(shape):
    """Forward (output and LSE, the forward tolerances of test_hip_ops.py)
    and the three gradients of the 128-row kernels."""
    q, k, v, g, refs = _case(shape)
    out, lse = ops.flash_attention(q, k, v, causal=shape[5], return_lse=True)
    ref_out, ref_lse = ops.flash_attention_ref(q, k, v, causal=shape[5])
    torch.testing.assert_close(out.float(), ref_out.float(), atol=4e-2,
                               rtol=4e-2)
    torch.testing.assert_close(lse, ref_lse, atol=2e-2, rtol=2e-2)
    grads = _ours(q, k, v, g, shape[5])
    for name, ours, ref in zip(("dq", "dk", "dv"), grads, refs):
        assert torch.isfinite(ours).all(), (name, shape)
        rel = _rel(ours, ref)
        print(f"{shape} {name} rel {rel:.3e}")
        assert rel < REL_BOUND, (name, shape, rel)


@pytest.mark.gpu
def test_fa_bwd_v6_one_hot_upstream_gradient():
    """dO is one query row q* (second key block) of one head: dK and dV
    are exactly zero for every later key of that kv head and for every
    other (batch, kv head). A transposed mask or wrong head / batch
    indexing, which a norm can hide, puts non-zeros there."""
    B, Hq, Hkv, T, bthd, causal = SHAPES[0]
    q, k, v, _, _ = _case(SHAPES[0])
    b_s, hq_s, q_s = 1, 5, 256 + 77
    hkv_s = hq_s // (Hq // Hkv)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    g = torch.zeros(B, T, Hq, D, device="cuda",
                    dtype=torch.bfloat16).transpose(1, 2)
    g[b_s, hq_s, q_s] = torch.randn(D, device="cuda", dtype=torch.bfloat16,
                                    generator=gen)
    _, dk, dv = _ours(q, k, v, g, causal)
    _, rdk, rdv = _ref_grads(q, k, v, g, causal)
    for name, ours, ref in (("dk", dk, rdk), ("dv", dv, rdv)):
        for b in range(B):
            for h in range(Hkv):
                if (b, h) == (b_s, hkv_s):
                    assert (ours[b, h, q_s + 1:] == 0).all(), name
                else:
                    assert (ours[b, h] == 0).all(), (name, b, h)
        assert _rel(ours, ref) < REL_BOUND, name


@pytest.mark.gpu
def test_fa_bwd_v6_repeatable():
    """20 backward passes over the same inputs are bit-identical: a read
    that races the split staging shows up as a run that differs."""
    B, Hq, Hkv, T = 2, 8, 2, 1024
    gen = torch.Generator(device="cuda")
    gen.manual_seed(99)
    q = _rand(B, Hq, T, True, gen).requires_grad_()
    k = _rand(B, Hkv, T, True, gen).requires_grad_()
    v = _rand(B, Hkv, T, True, gen).requires_grad_()
    g = _rand(B, Hq, T, True, gen)
    out = ops.flash_attention(q, k, v, causal=True)
    first = torch.autograd.grad(out, (q, k, v), g, retain_graph=True)
    for run in range(1, 20):
        again = torch.autograd.grad(out, (q, k, v), g, retain_graph=True)
        for name, a, b in zip(("dq", "dk", "dv"), first, again):
            assert torch.equal(a, b), (name, run)


def _guarded(t, offset=64, tail=4096):
    """A contiguous copy of t at a storage offset inside a NaN buffer."""
    buf = torch.full((offset + t.numel() + tail,), float("nan"),
                     device=t.device, dtype=t.dtype)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.storage_offset() == offset
    return view


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]],
                         ids=lambda s: "B%dHq%dHkv%dT%d" % s[:4])
def test_fa_bwd_v6_guard_bands(shape):
    """q, k, v and dO surrounded by NaN: a read outside the tensors
    poisons the gradients."""
    q, k, v, g, refs = _case(shape)
    grads = _ours(_guarded(q), _guarded(k), _guarded(v), _guarded(g),
                  shape[5])
    for name, ours, ref in zip(("dq", "dk", "dv"), grads, refs):
        assert torch.isfinite(ours).all(), (name, shape)
        assert _rel(ours, ref) < REL_BOUND, (name, shape)
