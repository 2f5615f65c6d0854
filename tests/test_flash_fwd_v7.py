"""Forward attention on the 256-row path (flash_attn_fwd_v7: two-phase
ping-pong schedule, a test-free loop over unmasked tiles, the masked body
for the causal diagonal and a ragged tail) against the fp32 reference:
pipeline depth and parity, the diagonal on every storage layout, q_offset,
the defer-max rescale after the first tile, NaN guard bands and run-to-run
repeatability."""
import functools

import pytest
import torch

from ray_amd import ops

D = 128
OUT_TOL = 4e-2   # the project's forward tolerance, atol = rtol
LSE_TOL = 2e-2


def _randn(*shape):
    return torch.randn(*shape, device="cuda", dtype=torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _case(B, Hq, Hkv, T, Tk, causal):
    """Contiguous BHTD inputs and their fp32 reference, computed once and
    shared read-only."""
    torch.manual_seed(4321 + 7 * T + Tk + Hq)
    q = _randn(B, Hq, T, D)
    k = _randn(B, Hkv, Tk, D)
    v = _randn(B, Hkv, Tk, D)
    ref, ref_lse = ops.flash_attention_ref(q, k, v, causal=causal)
    return q, k, v, ref.float(), ref_lse


def _check(out, lse, ref, ref_lse, what):
    assert torch.isfinite(out).all(), what
    assert torch.isfinite(lse).all(), what
    rel = float((out.float() - ref).norm() / ref.norm())
    rel_lse = float((lse - ref_lse).norm() / ref_lse.norm())
    print(f"{what}: out rel L2 {rel:.3e}, lse rel L2 {rel_lse:.3e}")
    assert torch.allclose(out.float(), ref, atol=OUT_TOL, rtol=OUT_TOL), what
    assert torch.allclose(lse, ref_lse, atol=LSE_TOL, rtol=LSE_TOL), what


def _fwd(q, k, v, causal, q_offset=0):
    return ops.flash_attention(q, k, v, causal=causal, q_offset=q_offset,
                               return_lse=True)


def _bthd(t):
    """The same values as a transpose view of [B,T,H,D] storage."""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def _packed(q, k, v, pad=0):
    """q, k, v as the column sections of one packed [B,T,(Hq+2Hkv)*D]
    buffer; with pad, that buffer is a column slice of a wider tensor."""
    B, Hq, T, _ = q.shape
    Hkv = k.shape[1]
    W = (Hq + 2 * Hkv) * D
    wide = torch.full((B, T, W + 2 * pad), float("nan"), device=q.device,
                      dtype=q.dtype)
    qkv = wide[..., pad:pad + W] if pad else wide
    qs, ks, vs = ops._qkv_sections(qkv, Hq, Hkv)
    qs.copy_(q)
    ks.copy_(k)
    vs.copy_(v)
    return qs, ks, vs


@pytest.mark.gpu
@pytest.mark.parametrize("Tk", [40, 64, 128, 192, 300, 320, 1024])
def test_pipeline_depth_and_parity(Tk):
    """1, 1, 2, 3, 5, 5 and 16 tiles: a ragged tail in the first and in the
    second sub-tile, odd and even counts, and a loop of full tiles only."""
    q, k, v, ref, ref_lse = _case(1, 4, 2, 256, Tk, False)
    out, lse = _fwd(q, k, v, False)
    _check(out, lse, ref, ref_lse, f"Tk{Tk}")


DIAG = [(1, 4, 2, 256), (2, 8, 2, 512), (1, 4, 4, 768)]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["bhtd", "bthd", "packed"])
@pytest.mark.parametrize("shape", DIAG, ids=lambda s: "B%dHq%dHkv%dT%d" % s)
def test_causal_diagonal(shape, layout):
    """T 768 has blocks with 0, 4 and 8 unmasked tiles in front of the
    diagonal; in each diagonal tile some waves compute and some skip."""
    B, Hq, Hkv, T = shape
    q, k, v, ref, ref_lse = _case(B, Hq, Hkv, T, T, True)
    if layout == "bthd":
        q, k, v = _bthd(q), _bthd(k), _bthd(v)
        assert ops._is_bthd_view(q) and not q.is_contiguous()
    elif layout == "packed":
        q, k, v = _packed(q, k, v)
        assert ops._is_bthd_view(q, True) and q.stride(2) > Hq * D
    out, lse = _fwd(q, k, v, True)
    _check(out, lse, ref, ref_lse, f"{shape} {layout}")


@pytest.mark.gpu
def test_causal_packed_slice_of_wider_tensor():
    B, Hq, Hkv, T = DIAG[1]
    q, k, v, ref, ref_lse = _case(B, Hq, Hkv, T, T, True)
    qs, ks, vs = _packed(q, k, v, pad=128)
    assert qs.stride(2) == (Hq + 2 * Hkv) * D + 256
    out, lse = _fwd(qs, ks, vs, True)
    _check(out, lse, ref, ref_lse, "packed slice")


@pytest.mark.gpu
@pytest.mark.parametrize("Tk", [320, 576])
def test_q_offset(Tk):
    """q_offset = Tk - T: the diagonal sits inside the first tile's
    successor (Tk 320) and after two unmasked tiles (Tk 576)."""
    T = 256
    q, k, v, ref, ref_lse = _case(1, 4, 2, T, Tk, True)
    out, lse = _fwd(q, k, v, True, q_offset=Tk - T)
    _check(out, lse, ref, ref_lse, f"q_offset Tk{Tk}")


@functools.lru_cache(maxsize=None)
def _rescale_inputs():
    # drawn on the CPU: the same inputs on every machine
    torch.manual_seed(7)
    B, Hq, Hkv, T = 1, 4, 2, 512
    q = torch.randn(B, Hq, T, D).to(torch.bfloat16)
    k = torch.randn(B, Hkv, T, D).to(torch.bfloat16)
    v = torch.randn(B, Hkv, T, D).to(torch.bfloat16)
    for j in (70, 200, 235, 300, 497):
        k[:, :, j] *= 6
    return q.cuda(), k.cuda(), v.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True])
def test_defer_max_rescale(causal):
    """Five keys scaled by 6 move the row maximum by more than the defer-max
    threshold (8) in the middle of the key range, for some rows of a wave
    and not for others. The kernel's deferred maximum is never above the
    true one, so it takes the rescale branch at least where the true running
    maximum jumps. The fp32 reference gives 247 such rows in 63 mixed groups
    without the mask and 144 rows in 45 groups with it."""
    q, k, v = _rescale_inputs()
    B, Hq, T, _ = q.shape
    kf = k.float().repeat_interleave(Hq // k.shape[1], dim=1)
    s = torch.matmul(q.float(), kf.transpose(-1, -2)) / D ** 0.5
    if causal:
        mask = torch.ones(T, T, dtype=torch.bool, device=q.device).tril_()
        s = s.masked_fill(~mask, float("-inf"))
    sub_max = s.view(B, Hq, T, T // 32, 32).amax(-1)       # per 32-key sub-tile
    run = sub_max.cummax(-1).values
    prev = run[..., :-1]
    jump = (torch.isfinite(prev) & (sub_max[..., 1:] - prev > 8)).any(-1)
    rows = jump.reshape(-1)                                 # 2048 query rows
    groups = rows.view(-1, 32)                              # one wave's rows
    mixed = int((groups.any(1) & ~groups.all(1)).sum())
    print(f"causal {causal}: {int(rows.sum())} rows jump, "
          f"{mixed} of {groups.shape[0]} groups mixed")
    assert rows.numel() == 2048 and int(rows.sum()) >= 100
    assert mixed * 2 >= groups.shape[0]

    ref, ref_lse = ops.flash_attention_ref(q, k, v, causal=causal)
    out, lse = _fwd(q, k, v, causal)
    _check(out, lse, ref.float(), ref_lse, f"rescale causal {causal}")


def _guarded(t, offset=64, tail=4096):
    """A contiguous copy of t at a storage offset inside a NaN buffer."""
    buf = torch.full((offset + t.numel() + tail,), float("nan"),
                     device=t.device, dtype=t.dtype)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.storage_offset() == offset
    return view


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(1, 4, 2, 256, 300, False),
                                  (2, 8, 2, 512, 512, True)],
                         ids=["T256Tk300", "T512causal"])
def test_guard_bands(case):
    """q, k and v surrounded by NaN: a row read at or past Tk, or a column
    past the head, poisons the output."""
    q, k, v, ref, ref_lse = _case(*case)
    out, lse = _fwd(_guarded(q), _guarded(k), _guarded(v), case[5])
    _check(out, lse, ref, ref_lse, f"guarded {case}")


@pytest.mark.gpu
def test_repeatable():
    q, k, v, _, _ = _case(2, 8, 2, 512, 512, True)
    out1, lse1 = _fwd(q, k, v, True)
    out2, lse2 = _fwd(q, k, v, True)
    assert torch.equal(out1, out2) and torch.equal(lse1, lse2)
