"""The dQ kernel's query-block order: block (x, y) of the (T/256, B*Hq) grid
takes query block (x + y) % gridDim.x, heaviest first inside a grid row and
rotated from row to row. The shapes are the smallest at which that mapping
can go wrong: a block count that does not divide the number of grid rows
(the rotation wraps), as many rows as blocks, one block, eight blocks, the
mask off. dq is held to the fp32 autograd reference, to exact zeros under a
one-row upstream gradient, to "every row written once" over a NaN-filled
packed gradient buffer, to run-to-run equality and to NaN guard bands.

Every case runs ops.flash_attention(...).backward. The autograd function has
no argument for a packed gradient buffer, so the cases that need one call the
binding once more on the saved forward results, with the buffer, the way
ops._QkvRopeAttn.backward does."""
import functools

import pytest
import torch

from ray_amd import ops

D = 128
REL_BOUND = 0.03  # the project's ||ours - ref|| / ||ref|| bound

# (B, Hq, Hkv, T, layout, causal); layout "bhtd" is contiguous [B,H,T,D],
# "view" a transpose of [B,T,H,D] storage, "packed" the column sections of
# one [B,T,(Hq+2Hkv)*D] buffer inside wider NaN-filled rows.
S_WRAP = (1, 4, 2, 768, "view", True)      # 3 blocks, 4 grid rows
S_FIVE = (1, 5, 5, 1280, "bhtd", True)     # n_tiles 4, 8, 12, 16, 20
S_DIAG = (1, 4, 4, 256, "bhtd", True)      # one all-diagonal block
S_FULL = (1, 8, 2, 512, "view", False)     # no wave skips
S_EIGHT = (2, 4, 1, 2048, "packed", True)  # gridDim.x = 8
SHAPES = [S_WRAP, S_FIVE, S_DIAG, S_FULL, S_EIGHT]
S_ZEROS = (2, 8, 2, 768, "view", True)
S_REPEAT = (2, 8, 2, 1024, "view", True)

PAD = 128   # extra NaN columns on either side of a packed row
GUARD = 4096


def _ids(s):
    return "B%dHq%dHkv%dT%d-%s-%s" % (s[:5] + ("causal" if s[5] else "full",))


def _rand(B, H, T, layout, gen):
    if layout == "bhtd":
        return torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16,
                           generator=gen)
    return torch.randn(B, T, H, D, device="cuda", dtype=torch.bfloat16,
                       generator=gen).transpose(1, 2)


def _nan_packed(B, T, W):
    """A [B,T,W] view at column PAD of NaN-filled rows of W + 2 PAD elements,
    GUARD elements of NaN before and after. Returns (allocation, view)."""
    rs = W + 2 * PAD
    big = torch.full((GUARD + B * T * rs + GUARD,), float("nan"),
                     device="cuda", dtype=torch.bfloat16)
    body = big[GUARD:GUARD + B * T * rs].view(B, T, rs)
    return big, body[:, :, PAD:PAD + W]


def _outside_is_nan(big, view):
    mark = torch.zeros_like(big, dtype=torch.bool)
    mark.as_strided(view.shape, view.stride(),
                    view.storage_offset()).fill_(True)
    return bool(torch.isnan(big[~mark]).all())


def _ref_dq(q, k, v, g, causal):
    q2 = q.detach().clone().requires_grad_()
    ref, _ = ops.flash_attention_ref(q2, k.detach(), v.detach(),
                                     causal=causal)
    ref.backward(g.float())
    return q2.grad.float()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs and the fp32 reference dq of one shape, computed once and
    shared (read-only) by the tests below."""
    B, Hq, Hkv, T, layout, causal = shape
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4321 + T + Hq)
    q = _rand(B, Hq, T, layout, gen)
    k = _rand(B, Hkv, T, layout, gen)
    v = _rand(B, Hkv, T, layout, gen)
    g = _rand(B, Hq, T, layout, gen)
    if layout == "packed":
        _, qkv = _nan_packed(B, T, (Hq + 2 * Hkv) * D)
        qs, ks, vs = ops._qkv_sections(qkv, Hq, Hkv)
        qs.copy_(q), ks.copy_(k), vs.copy_(v)
        q, k, v = qs, ks, vs
        assert ops._attn_operands(q, k, v)[3]  # read as they are, no copy
    return q, k, v, g, _ref_dq(q, k, v, g, causal)


def _ours_dq(q, k, v, g, causal):
    q1 = q.detach().requires_grad_()
    out = ops.flash_attention(q1, k.detach(), v.detach(), causal=causal)
    out.backward(g)
    return q1.grad


def _packed_dq(q, k, v, g, causal):
    """The backward once more on a NaN-filled packed gradient buffer.
    Returns (allocation, buffer, dq section as [B,Hq,T,D])."""
    B, Hq, T, _ = q.shape
    Hkv = k.shape[1]
    out, lse = ops._K.flash_attn_fwd(q, k, v, causal, 0, True)
    big, buf = _nan_packed(B, T, (Hq + 2 * Hkv) * D)
    dq, _, _ = ops._K.flash_attn_bwd(q, k, v, out, g, lse, causal, buf)
    assert dq.data_ptr() == buf.data_ptr() and dq.shape == q.shape
    return big, buf, dq


def _rel(ours, ref):
    return float((ours.float() - ref).norm() / (ref.norm() + 1e-6))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_dq_matches_fp32_reference(shape):
    q, k, v, g, ref = _case(shape)
    dq = _ours_dq(q, k, v, g, shape[5])
    assert torch.isfinite(dq).all(), shape
    rel = _rel(dq, ref)
    print(f"{shape} dq rel {rel:.3e}")
    assert rel < REL_BOUND, (shape, rel)
    if shape[4] == "packed":
        # the same gradient written into column sections of wider rows
        big, buf, dq_p = _packed_dq(q, k, v, g, shape[5])
        assert torch.isfinite(buf).all()
        assert torch.equal(dq_p, dq)
        assert _outside_is_nan(big, buf)


@pytest.mark.gpu
@pytest.mark.parametrize("q_s", [256 + 77, 512 + 201],
                         ids=["second_block", "last_block"])
def test_dq_exact_zeros_under_one_row_gradient(q_s):
    """dO is one query row q* of one (batch, head): dP and delta are 0 in
    every other row, so dQ is exactly 0 there, in every other head and in
    the other batch. A wrong query-block or head index, which a norm can
    hide, puts non-zeros there."""
    B, Hq, Hkv, T, _, causal = S_ZEROS
    q, k, v, _, _ = _case(S_ZEROS)
    b_s, hq_s = 1, 5
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    g = torch.zeros(B, T, Hq, D, device="cuda",
                    dtype=torch.bfloat16).transpose(1, 2)
    g[b_s, hq_s, q_s] = torch.randn(D, device="cuda", dtype=torch.bfloat16,
                                    generator=gen)
    dq = _ours_dq(q, k, v, g, causal)
    ref = _ref_dq(q, k, v, g, causal)
    assert torch.isfinite(dq).all()
    rest = dq.clone()
    rest[b_s, hq_s, q_s] = 0
    assert (rest == 0).all(), torch.nonzero(rest)[:8].tolist()
    assert (dq[b_s, hq_s, q_s] != 0).any()
    rel = _rel(dq[b_s, hq_s, q_s], ref[b_s, hq_s, q_s])
    print(f"q* {q_s} row rel {rel:.3e}")
    assert rel < REL_BOUND, rel
    assert _rel(dq, ref) < REL_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [S_WRAP, S_FIVE], ids=_ids)
def test_dq_every_row_written_once(shape):
    """The dq section of a NaN-filled packed gradient buffer is finite
    everywhere after the backward and equals the gradient of the unpacked
    call: a block mapped twice or never leaves NaN or stale rows."""
    B, Hq, Hkv, T, _, causal = shape
    q, k, v, g, _ = _case(shape)
    # the packed gradient needs the operands in the BTHD-view layout
    qv, kv, vv, gv = (t.transpose(1, 2).contiguous().transpose(1, 2)
                      for t in (q, k, v, g))
    big, buf, dq_p = _packed_dq(qv, kv, vv, gv, causal)
    assert torch.isfinite(dq_p).all()
    assert torch.isfinite(buf).all()
    assert _outside_is_nan(big, buf)
    assert torch.equal(dq_p, _ours_dq(q, k, v, g, causal))


@pytest.mark.gpu
def test_dq_repeatable():
    """20 backward passes over the same inputs give the same dq bits: a
    read that races the staging shows up as a run that differs."""
    q, k, v, g, _ = _case(S_REPEAT)
    q1 = q.detach().requires_grad_()
    out = ops.flash_attention(q1, k, v, causal=True)
    first, = torch.autograd.grad(out, (q1,), g, retain_graph=True)
    for run in range(1, 20):
        again, = torch.autograd.grad(out, (q1,), g, retain_graph=True)
        assert torch.equal(first, again), run


def _guarded(t, offset=64, tail=4096):
    """A contiguous copy of t at a storage offset inside a NaN buffer."""
    buf = torch.full((offset + t.numel() + tail,), float("nan"),
                     device=t.device, dtype=t.dtype)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.storage_offset() == offset
    return view


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [S_DIAG, S_FIVE], ids=_ids)
def test_dq_guard_bands(shape):
    """q, k, v and dO surrounded by NaN: a read outside the tensors
    poisons dq."""
    q, k, v, g, ref = _case(shape)
    dq = _ours_dq(_guarded(q), _guarded(k), _guarded(v), _guarded(g),
                  shape[5])
    assert torch.isfinite(dq).all(), shape
    assert _rel(dq, ref) < REL_BOUND, shape
