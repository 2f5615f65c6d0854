"""Attention straight on the packed QKV projection output:
`rope_qk_inplace`, the 256-row flash kernels reading and writing column
sections of one [B,T,(Hq+2Hkv)*D] buffer, and ops.qkv_rope_attention.

Everything here is compared bit for bit (torch.equal) with today's
composition: split, ops.rope (a gather into fresh tensors), v.contiguous(),
the flash kernels on [B,T,H,D] storage, the inverse rope and a cat. The
kernels do the same arithmetic on the same values at other addresses, so
nothing but equality is acceptable. Packed buffers live inside a NaN guard
band, and every column a kernel must not write holds NaN before the call.
"""
import pytest
import torch

from ray_amd import ops

D = 128
GUARD = 4096          # elements of NaN before and after a packed buffer

# (B, Hq, Hkv, T): one block with diagonal tiles only; batch stride, GQA 4
# and an off-diagonal tile; MHA with an odd number of blocks
SHAPES = [(1, 4, 2, 256), (2, 8, 2, 512), (1, 4, 4, 768)]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if not ops.HAVE_HIP_OPS:
        raise RuntimeError("HIP extension not built")
    return torch.device("cuda")


def _randn(shape, seed, dev, dtype=torch.bfloat16):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(dtype).to(dev)


def _tables(T, d, dev):
    c, s = ops.rope_tables(T, d)
    return c.to(dev), s.to(dev)


def _packed(vals, pad=0, off=0, lead=0):
    """`vals` [B,T,W] copied into a NaN-filled allocation: GUARD + lead
    elements of NaN, then rows of W + pad elements with the data at column
    `off`, then GUARD elements of NaN. Returns (allocation, view)."""
    B, T, W = vals.shape
    rs = W + pad
    big = torch.full((GUARD + lead + B * T * rs + GUARD,), float("nan"),
                     dtype=vals.dtype, device=vals.device)
    body = big[GUARD + lead: GUARD + lead + B * T * rs].view(B, T, rs)
    view = body[:, :, off: off + W]
    view.copy_(vals)
    return big, view


def _outside_is_nan(big, view):
    """Every element of the allocation outside `view` is still NaN."""
    mark = torch.zeros_like(big, dtype=torch.bool)
    mark_view = mark.as_strided(view.shape, view.stride(),
                                view.storage_offset())
    mark_view.fill_(True)
    return bool(torch.isnan(big[~mark]).all())


def _sections(qkv, Hq, Hkv, d=D):
    B, T, _ = qkv.shape
    q, k, v = qkv.split([Hq * d, Hkv * d, Hkv * d], dim=-1)
    return (q.view(B, T, Hq, d), k.view(B, T, Hkv, d), v.view(B, T, Hkv, d))


_REF = {}


def _reference(shape, dev):
    """Today's composition on the seeded inputs of one shape, computed once:
    rotated q/k, out, lse and the packed gradient."""
    if shape in _REF:
        return _REF[shape]
    B, Hq, Hkv, T = shape
    W = (Hq + 2 * Hkv) * D
    vals = _randn((B, T, W), 31 * T + Hq, dev)
    d_out = _randn((B, T, Hq, D), 31 * T + Hq + 1, dev)
    cosT, sinT = _tables(T, D, dev)
    q, k, v = _sections(vals, Hq, Hkv)
    qr, kr = ops.rope(q, cosT, sinT), ops.rope(k, cosT, sinT)
    vc = v.contiguous()
    out, lse = ops._K.flash_attn_fwd(
        qr.transpose(1, 2), kr.transpose(1, 2), vc.transpose(1, 2), True, 0,
        True)
    dq, dk, dv = ops._K.flash_attn_bwd(
        qr.transpose(1, 2), kr.transpose(1, 2), vc.transpose(1, 2), out,
        d_out.transpose(1, 2), lse, True)
    dq, dk, dv = (t.transpose(1, 2).contiguous() for t in (dq, dk, dv))
    dq_u = ops._K.rope_apply(dq, cosT, sinT, Hq, T, -1)
    dk_u = ops._K.rope_apply(dk, cosT, sinT, Hkv, T, -1)
    rot = torch.cat([t.reshape(B, T, -1) for t in (dq, dk, dv)], dim=-1)
    grad = torch.cat([t.reshape(B, T, -1) for t in (dq_u, dk_u, dv)], dim=-1)
    _REF[shape] = dict(vals=vals, d_out=d_out, cosT=cosT, sinT=sinT, qr=qr,
                       kr=kr, out=out, lse=lse, grad_rot=rot, grad=grad)
    return _REF[shape]


def _run_packed(shape, dev, pad, off):
    B, Hq, Hkv, T = shape
    ref = _reference(shape, dev)
    cosT, sinT = ref["cosT"], ref["sinT"]
    big, qkv = _packed(ref["vals"], pad, off)
    ops._K.rope_qk_inplace(qkv, cosT, sinT, Hq, Hkv, 1)
    q, k, v = _sections(qkv, Hq, Hkv)
    assert torch.equal(q, ref["qr"]) and torch.equal(k, ref["kr"])
    assert torch.equal(v, _sections(ref["vals"], Hq, Hkv)[2])
    assert _outside_is_nan(big, qkv)
    qt, kt, vt = (t.transpose(1, 2) for t in (q, k, v))
    assert ops._is_bthd_view(qt, True) and ops._is_bthd_view(vt, True)
    out, lse = ops._K.flash_attn_fwd(qt, kt, vt, True, 0, True)
    assert torch.equal(out, ref["out"]) and torch.equal(lse, ref["lse"])
    # ops.flash_attention reads the same views without a copy
    assert ops._attn_operands(qt, kt, vt)[3]
    assert torch.equal(ops.flash_attention(qt, kt, vt), ref["out"])
    gbig, g = _packed(torch.full_like(ref["vals"], float("nan")), pad, off)
    dq, dk, dv = ops._K.flash_attn_bwd(
        qt, kt, vt, out, ref["d_out"].transpose(1, 2), lse, True, g)
    assert not torch.isnan(g).any()
    assert torch.equal(g, ref["grad_rot"])
    assert dq.data_ptr() == g.data_ptr() and dq.shape == qt.shape
    assert torch.equal(dv, _sections(g, Hq, Hkv)[2].transpose(1, 2))
    ops._K.rope_qk_inplace(g, cosT, sinT, Hq, Hkv, -1)
    assert torch.equal(g, ref["grad"])
    assert _outside_is_nan(gbig, g) and _outside_is_nan(big, qkv)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_packed_kernels_equal_composition(shape):
    _run_packed(shape, _gpu(), pad=0, off=0)


@pytest.mark.gpu
def test_packed_kernels_wider_row_stride():
    """The packed buffer as a column slice of a wider tensor."""
    _run_packed(SHAPES[1], _gpu(), pad=24, off=8)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_op_equals_composition(monkeypatch, shape):
    dev = _gpu()
    B, Hq, Hkv, T = shape
    ref = _reference(shape, dev)
    d_out = ref["d_out"].reshape(B, T, Hq * D)
    res = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "_FUSED_QKV_ATTN", fused)
        leaf = ref["vals"].clone().requires_grad_(True)
        qkv = leaf * 1                      # what a projection hands over
        assert ops._qkv_packed_ok(qkv, Hq, Hkv)
        out = ops.qkv_rope_attention(qkv, ref["cosT"], ref["sinT"], Hq, Hkv)
        assert out.shape == (B, T, Hq * D)
        # the fused path rotates its input in place, the other leaves it
        assert torch.equal(qkv.detach(), ref["vals"]) == (not fused)
        out.backward(d_out)
        res.append((out.detach(), leaf.grad))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][0],
                       ref["out"].transpose(1, 2).reshape(B, T, Hq * D))
    assert torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][1], ref["grad"])


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("T", [1, 5, 256])
def test_rope_qk_inplace(T, d):
    dev = _gpu()
    B, Hq, Hkv = 2, 4, 2
    W = (Hq + 2 * Hkv) * d
    vals = _randn((B, T, W), 17 * T + d, dev)
    cosT, sinT = _tables(T, d, dev)
    q0, k0, v0 = _sections(vals, Hq, Hkv, d)
    qr, kr = ops.rope(q0, cosT, sinT), ops.rope(k0, cosT, sinT)
    # what rope_fwd_bf16 itself loses on a round trip of the same data
    q_back = ops._K.rope_apply(qr, cosT, sinT, Hq, T, -1)
    k_back = ops._K.rope_apply(kr, cosT, sinT, Hkv, T, -1)
    bound = max((q_back.float() - q0.float()).abs().max().item(),
                (k_back.float() - k0.float()).abs().max().item())
    for pad, off in ((0, 0), (16, 8)):
        big, qkv = _packed(vals, pad, off)
        ops._K.rope_qk_inplace(qkv, cosT, sinT, Hq, Hkv, 1)
        q, k, v = _sections(qkv, Hq, Hkv, d)
        assert torch.equal(q, qr) and torch.equal(k, kr)
        assert torch.equal(v, v0)
        assert _outside_is_nan(big, qkv)
        ops._K.rope_qk_inplace(qkv, cosT, sinT, Hq, Hkv, -1)
        q, k, v = _sections(qkv, Hq, Hkv, d)
        assert torch.equal(v, v0) and _outside_is_nan(big, qkv)
        err = max((q.float() - q0.float()).abs().max().item(),
                  (k.float() - k0.float()).abs().max().item())
        print(f"rope round trip T={T} D={d}: in place {err:.3e}, "
              f"rope_fwd {bound:.3e}")
        assert err <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("T", [5, 256])
def test_rope_vector_and_scalar_kernels_agree(T, d, strided):
    """ops.rope takes the 16-byte kernel for aligned inputs and the one-pair
    kernel (the arithmetic every earlier revision ran) otherwise: same bits,
    for contiguous inputs and for slices of a wider row (in_rs > H*D), in
    both directions."""
    dev = _gpu()
    B, H = 2, 3
    rs = H * d + (2 * d if strided else 0)
    cosT, sinT = _tables(T, d, dev)
    vals = _randn((B, T, rs), 7 * T + d, dev)
    flat = torch.empty(vals.numel() + 1, dtype=vals.dtype, device=dev)
    shifted = flat[1:].view(B, T, rs)            # 2-byte aligned only
    shifted.copy_(vals)
    x = vals[..., :H * d].view(B, T, H, d)
    xs = shifted[..., :H * d].view(B, T, H, d)
    assert x.data_ptr() % 16 == 0 and xs.data_ptr() % 16 != 0
    assert x.is_contiguous() != strided
    for sign in (1, -1):
        vec = ops._K.rope_apply(x, cosT, sinT, H, T, sign)
        sca = ops._K.rope_apply(xs, cosT, sinT, H, T, sign)
        assert torch.equal(vec, sca), (T, d, strided, sign)
    assert torch.equal(ops.rope(xs, cosT, sinT), ops.rope(x, cosT, sinT))


@pytest.mark.gpu
def test_layouts_that_do_not_qualify():
    dev = _gpu()
    shape = SHAPES[0]
    B, Hq, Hkv, T = shape
    ref = _reference(shape, dev)
    cosT, sinT = ref["cosT"], ref["sinT"]
    rot = torch.cat([ref["qr"].reshape(B, T, -1), ref["kr"].reshape(B, T, -1),
                     _sections(ref["vals"], Hq, Hkv)[2].reshape(B, T, -1)],
                    dim=-1)
    # a section start that is not 16-byte aligned; a row stride % 8 != 0
    for pad, off, lead in ((8, 0, 1), (4, 0, 0)):
        big, qkv = _packed(rot, pad, off, lead)
        with pytest.raises(RuntimeError):
            ops._K.rope_qk_inplace(qkv, cosT, sinT, Hq, Hkv, 1)
        qt, kt, vt = (t.transpose(1, 2) for t in _sections(qkv, Hq, Hkv))
        assert not ops._is_bthd_view(qt, True)
        assert not ops._qkv_packed_ok(qkv, Hq, Hkv)
        with pytest.raises(RuntimeError):
            ops._K.flash_attn_fwd(qt, kt, vt, True, 0, True)
        # routed to contiguous copies, not misread
        assert torch.equal(ops.flash_attention(qt, kt, vt), ref["out"])
        assert torch.equal(qkv, rot) and _outside_is_nan(big, qkv)
    # a packed gradient buffer that does not qualify is refused
    _, qkv = _packed(rot)
    qt, kt, vt = (t.transpose(1, 2) for t in _sections(qkv, Hq, Hkv))
    _, g = _packed(rot, 4, 0)
    with pytest.raises(RuntimeError):
        ops._K.flash_attn_bwd(qt, kt, vt, ref["out"],
                              ref["d_out"].transpose(1, 2), ref["lse"], True,
                              g)
    # T = 384: only the 128-row kernels run it, and they read contiguous
    # tensors, so the op takes the composed path and the binding refuses
    # the views
    T2 = 384
    vals = _randn((1, T2, (Hq + 2 * Hkv) * D), 99, dev)
    cos2, sin2 = _tables(T2, D, dev)
    assert not ops._qkv_packed_ok(vals, Hq, Hkv)
    got = ops.qkv_rope_attention(vals.clone(), cos2, sin2, Hq, Hkv)
    q, k, v = _sections(vals, Hq, Hkv)
    want = ops.flash_attention(
        ops.rope(q, cos2, sin2).transpose(1, 2),
        ops.rope(k, cos2, sin2).transpose(1, 2),
        v.contiguous().transpose(1, 2))
    assert torch.equal(got, want.transpose(1, 2).reshape(1, T2, Hq * D))
    with pytest.raises(RuntimeError):
        ops._K.flash_attn_fwd(*(t.transpose(1, 2) for t in (q, k, v)), True,
                              0, True)


def test_cpu_op_equals_composition():
    B, T, Hq, Hkv, d = 2, 8, 4, 2, 16
    vals = _randn((B, T, (Hq + 2 * Hkv) * d), 3, "cpu", torch.float32)
    g_out = _randn((B, T, Hq * d), 4, "cpu", torch.float32)
    cosT, sinT = ops.rope_tables(T, d)
    a = vals.clone().requires_grad_(True)
    out = ops.qkv_rope_attention(a * 1, cosT, sinT, Hq, Hkv)
    out.backward(g_out)
    b = vals.clone().requires_grad_(True)
    q, k, v = _sections(b * 1, Hq, Hkv, d)
    want = ops.flash_attention(
        ops.rope(q, cosT, sinT).transpose(1, 2),
        ops.rope(k, cosT, sinT).transpose(1, 2),
        v.contiguous().transpose(1, 2))
    want = want.transpose(1, 2).reshape(B, T, Hq * d)
    want.backward(g_out)
    assert torch.equal(out, want)
    assert torch.equal(a.grad, b.grad)
