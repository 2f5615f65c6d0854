"""Paged-KV prefill attention: the fp32 reference on CPU, the HIP
kernel (csrc/hip/paged_attn_prefill.hip) against it on GPU."""
import functools

import pytest
import torch

from ray_amd import ops

PAGE = 16


def _cache_and_table(g, specs, Hkv, D, num_pages, dtype, fill):
    """K/V caches filled with `fill`, a block table that is a random
    permutation of pages 1..num_pages-1 with unused entries 0, and
    random values in exactly the first ctx + q_len rows of each
    sequence. specs is [(ctx, q_len)]."""
    B = len(specs)
    max_pages = max(1, max(-(-(c + n) // PAGE) for c, n in specs))
    kc = torch.full((num_pages, Hkv, PAGE, D), fill, dtype=dtype)
    vc = torch.full((num_pages, Hkv, PAGE, D), fill, dtype=dtype)
    perm = (torch.randperm(num_pages - 1, generator=g) + 1).tolist()
    bt = torch.zeros(B, max_pages, dtype=torch.int32)
    for b, (c, n) in enumerate(specs):
        L = c + n
        for i in range(-(-L // PAGE)):
            pg = perm.pop()
            bt[b, i] = pg
            rows = min(PAGE, L - i * PAGE)
            kc[pg, :, :rows] = torch.randn(Hkv, rows, D, generator=g).to(dtype)
            vc[pg, :, :rows] = torch.randn(Hkv, rows, D, generator=g).to(dtype)
    return kc, vc, bt


def _gather(cache, bt_row, L):
    """Dense [1, Hkv, L, D] view of one sequence's cache rows."""
    Hkv, D = cache.shape[1], cache.shape[3]
    pages = bt_row[: -(-L // PAGE)].long()
    return cache[pages].permute(1, 0, 2, 3).reshape(1, Hkv, -1, D)[:, :, :L]


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------


@pytest.mark.parametrize("ctx,Tq", [(0, 5), (17, 1), (60, 70)])
def test_prefill_ref_matches_dense_on_shuffled_table(ctx, Tq):
    """The paged reference over a shuffled, non-monotonic block table
    equals dense causal attention (Tk - T offset) over the gathered
    K/V."""
    g = torch.Generator().manual_seed(ctx + Tq)
    Hq, Hkv, D = 4, 2, 64
    kc, vc, bt = _cache_and_table(g, [(ctx, Tq)], Hkv, D, 24, torch.float32,
                                  0.0)
    row = bt[0, : -(-(ctx + Tq) // PAGE)].tolist()
    if len(row) > 2:
        assert row != sorted(row)  # the table really is shuffled
    q = torch.randn(1, Tq, Hq, D, generator=g)
    out = ops.paged_attention_prefill_ref(
        q, kc, vc, bt, torch.tensor([ctx], dtype=torch.int32),
        torch.tensor([Tq], dtype=torch.int32))
    assert out.shape == q.shape
    L = ctx + Tq
    dense, _ = ops.flash_attention_ref(q.transpose(1, 2), _gather(kc, bt[0], L),
                                       _gather(vc, bt[0], L), causal=True)
    assert torch.allclose(out, dense.transpose(1, 2), atol=1e-5, rtol=0)


def test_prefill_ref_single_row_equals_decode_ref():
    g = torch.Generator().manual_seed(3)
    Hq, Hkv, D = 4, 2, 64
    specs = [(0, 1), (15, 1), (16, 1), (40, 1)]
    kc, vc, bt = _cache_and_table(g, specs, Hkv, D, 16, torch.float32, 0.0)
    q = torch.randn(len(specs), 1, Hq, D, generator=g)
    ctx = torch.tensor([c for c, _ in specs], dtype=torch.int32)
    out = ops.paged_attention_prefill_ref(q, kc, vc, bt, ctx,
                                          torch.ones_like(ctx))
    dec = ops.paged_attention_ref(q[:, 0], kc, vc, bt, ctx + 1)
    assert torch.allclose(out[:, 0], dec, atol=1e-5, rtol=0)


def test_prefill_ref_pads_with_zeros():
    g = torch.Generator().manual_seed(4)
    kc, vc, bt = _cache_and_table(g, [(3, 2), (9, 0)], 2, 64, 8,
                                  torch.float32, float("nan"))
    q = torch.randn(2, 4, 4, 64, generator=g)
    out = ops.paged_attention_prefill_ref(
        q, kc, vc, bt, torch.tensor([3, 9], dtype=torch.int32),
        torch.tensor([2, 0], dtype=torch.int32))
    assert torch.isfinite(out).all()
    assert (out[0, :2] != 0).any() and (out[0, 2:] == 0).all()
    assert (out[1] == 0).all()


def test_prefill_dispatch_uses_ref_on_cpu():
    g = torch.Generator().manual_seed(5)
    kc, vc, bt = _cache_and_table(g, [(10, 9)], 2, 64, 6, torch.float32, 0.0)
    q = torch.randn(1, 9, 4, 64, generator=g)
    ctx = torch.tensor([10], dtype=torch.int32)
    ql = torch.tensor([9], dtype=torch.int32)
    assert torch.equal(ops.paged_attention_prefill(q, kc, vc, bt, ctx, ql),
                       ops.paged_attention_prefill_ref(q, kc, vc, bt, ctx, ql))


# --------------------------------------------------------------------------
# GPU: kernel vs paged_attention_prefill_ref on the same bf16 inputs.
# Every case lives in a NaN-filled cache: the null page, unallocated
# pages and the tail slots of each last page are NaN in K and V.
# --------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _gpu_case(D, Hq, Hkv, specs, Tq, seed):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(seed)
    need = sum(-(-(c + n) // PAGE) for c, n in specs)
    kc, vc, bt = _cache_and_table(g, list(specs), Hkv, D, need + 3,
                                  torch.bfloat16, float("nan"))
    q = torch.randn(len(specs), Tq, Hq, D, generator=g).bfloat16()
    ctx = torch.tensor([c for c, _ in specs], dtype=torch.int32)
    ql = torch.tensor([n for _, n in specs], dtype=torch.int32)
    ref = ops.paged_attention_prefill_ref(q, kc, vc, bt, ctx, ql)  # CPU fp32
    return tuple(t.to(dev) for t in (q, kc, vc, bt, ctx, ql)) + (ref,)


def _check(out, ref, atol=4e-2, rtol=4e-2):
    out = out.float().cpu()
    ref = ref.float()
    assert torch.isfinite(out).all()
    err = float((out - ref).abs().max())
    print(f"max abs err {err:.3e}")
    assert torch.allclose(out, ref, atol=atol, rtol=rtol), err


@pytest.mark.gpu
@pytest.mark.parametrize("ctx,Tq", [(0, 1), (0, 5), (1, 16), (15, 17),
                                    (16, 64), (17, 65), (63, 2), (60, 70)])
@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (8, 1), (4, 4)])
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_kernel_shape_grid(D, Hq, Hkv, ctx, Tq):
    q, kc, vc, bt, cl, ql, ref = _gpu_case(D, Hq, Hkv, ((ctx, Tq),), Tq,
                                           D + Hq + Hkv + ctx + Tq)
    out = ops.paged_attention_prefill(q, kc, vc, bt, cl, ql)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    _check(out, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("ctx,Tq", [(0, 129), (100, 130), (5, 260)])
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_kernel_crosses_query_tiles(D, ctx, Tq):
    """The kernel's query tile is 128 rows: chunks that end just past
    one and two tiles, with the diagonal inside a KV tile."""
    q, kc, vc, bt, cl, ql, ref = _gpu_case(D, 4, 2, ((ctx, Tq),), Tq,
                                           D + ctx + Tq)
    _check(ops.paged_attention_prefill(q, kc, vc, bt, cl, ql), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("B,Tq", [(63, 3), (64, 3), (22, 260)])
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_kernel_wide_tile_dispatch(D, B, Tq):
    """From 512 blocks of 128 query rows on (ceil(Tq/128) * Hq * B) the
    binding launches 256-row tiles: one case on each side of that
    threshold, and one whose chunks cross a 256-row tile, with mixed
    contexts and some short and empty rows."""
    Hq, Hkv = 8, 2
    assert (-(-Tq // 128) * Hq * B >= 512) == (B != 63)
    specs = tuple(((13 * b) % 90, Tq if b % 5 else (7 * b) % (Tq + 1))
                  for b in range(B))
    q, kc, vc, bt, cl, ql, ref = _gpu_case(D, Hq, Hkv, specs, Tq, B + D)
    out = ops.paged_attention_prefill(q, kc, vc, bt, cl, ql)
    _check(out, ref)
    for b, (_, n) in enumerate(specs):
        assert (out[b, n:] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_kernel_batch_with_padding(D):
    """B = 3 with different contexts, one short row and one empty row;
    padded rows are exactly zero."""
    Tq = 40
    specs = ((33, 40), (70, 23), (12, 0))
    q, kc, vc, bt, cl, ql, ref = _gpu_case(D, 8, 2, specs, Tq, 11 + D)
    out = ops.paged_attention_prefill(q, kc, vc, bt, cl, ql)
    _check(out, ref)
    assert (out[1, 23:] == 0).all()
    assert (out[2] == 0).all()
    assert (out[1, :23] != 0).any()


@pytest.mark.gpu
def test_prefill_kernel_poisoned_cache():
    """Whole cache NaN, only the valid rows written, shuffled table with
    unused entries 0: rows past ctx + q_len never reach the output."""
    q, kc, vc, bt, cl, ql, ref = _gpu_case(128, 4, 2, ((21, 30), (0, 3)), 30,
                                           99)
    assert torch.isnan(kc[0].float()).all()  # the null page is poison
    assert int((bt == 0).sum()) > 0           # and the table points at it
    L = 51
    last = int(bt[0, (L - 1) // PAGE])
    assert torch.isnan(kc[last, :, L % PAGE:].float()).all()  # tail slots
    out = ops.paged_attention_prefill(q, kc, vc, bt, cl, ql)
    assert torch.isfinite(out.float()).all()
    _check(out, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("D,Hq,Hkv", [(64, 4, 2), (128, 8, 1)])
def test_prefill_kernel_single_row_matches_decode_kernel(D, Hq, Hkv):
    specs = ((0, 1), (15, 1), (16, 1), (100, 1))
    q, kc, vc, bt, cl, ql, ref = _gpu_case(D, Hq, Hkv, specs, 1, 5 + D)
    out = ops.paged_attention_prefill(q, kc, vc, bt, cl, ql)
    _check(out, ref)
    dec = ops.paged_attention_decode(q[:, 0].contiguous(), kc, vc, bt,
                                     cl + 1, num_splits=1)
    d = float((out[:, 0].float() - dec.float()).abs().max())
    print(f"prefill vs decode kernel: max abs diff {d:.3e}")
    assert torch.allclose(out[:, 0].float(), dec.float(), atol=2e-2, rtol=0)


@pytest.mark.gpu
def test_prefill_binding_rejects_bad_inputs():
    q, kc, vc, bt, cl, ql, _ = _gpu_case(64, 4, 2, ((3, 8),), 8, 1)
    dev = q.device
    ops.paged_attention_prefill(q, kc, vc, bt, cl, ql)  # the good call
    with pytest.raises(RuntimeError):  # dtype
        ops.paged_attention_prefill(q.float(), kc, vc, bt, cl, ql)
    with pytest.raises(RuntimeError):  # non-contiguous q
        qt = q.transpose(1, 2).contiguous().transpose(1, 2)
        assert qt.shape == q.shape and not qt.is_contiguous()
        ops.paged_attention_prefill(qt, kc, vc, bt, cl, ql)
    with pytest.raises(RuntimeError):  # D = 96
        q96 = torch.zeros(1, 8, 4, 96, dtype=torch.bfloat16, device=dev)
        c96 = torch.zeros(4, 2, PAGE, 96, dtype=torch.bfloat16, device=dev)
        ops.paged_attention_prefill(q96, c96, c96.clone(), bt, cl, ql)
    with pytest.raises(RuntimeError):  # Hq/Hkv = 3
        q6 = torch.zeros(1, 8, 6, 64, dtype=torch.bfloat16, device=dev)
        ops.paged_attention_prefill(q6, kc, vc, bt, cl, ql)
    with pytest.raises(RuntimeError):  # int64 table
        ops.paged_attention_prefill(q, kc, vc, bt.long(), cl, ql)
    with pytest.raises(RuntimeError):  # int64 lengths
        ops.paged_attention_prefill(q, kc, vc, bt, cl.long(), ql)
    with pytest.raises(RuntimeError):  # Tq = 0
        ops.paged_attention_prefill(q[:, :0], kc, vc, bt, cl, ql)
