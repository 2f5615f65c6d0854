"""Split-KV multi-token verify attention (csrc/hip/paged_attn_verify.hip)
and rope_append_paged_multi against ops.paged_attention_prefill_ref and
rope_append_paged_multi_ref."""
import functools

import pytest
import torch

from ray_amd import ops

PAGE = 16
FP8 = torch.float8_e4m3fn


@functools.lru_cache(maxsize=None)
def _case(D, Hq, Hkv, specs, Tq, dtype=torch.bfloat16, fill=0.0, seed=0):
    """CPU inputs and reference for sequences specs = ((ctx, q_len), ...):
    caches filled with `fill` (the null page, pages in no table and rows at
    or beyond ctx + q_len keep it), a shuffled block table, random values in
    the first ctx + q_len rows of each sequence. fp8 caches use scales 0.5
    and 2."""
    g = torch.Generator().manual_seed(seed)
    B = len(specs)
    max_pages = max(1, max(-(-(c + n) // PAGE) for c, n in specs))
    num_pages = sum(-(-(c + n) // PAGE) for c, n in specs) + 3
    kc = torch.full((num_pages, Hkv, PAGE, D), fill).to(dtype)
    vc = kc.clone()
    perm = (torch.randperm(num_pages - 1, generator=g) + 1).tolist()
    bt = torch.zeros(B, max_pages, dtype=torch.int32)
    for b, (c, n) in enumerate(specs):
        for i in range(-(-(c + n) // PAGE)):
            bt[b, i] = pg = perm.pop()
            rows = min(PAGE, c + n - i * PAGE)
            kc[pg, :, :rows] = torch.randn(Hkv, rows, D, generator=g).to(dtype)
            vc[pg, :, :rows] = torch.randn(Hkv, rows, D, generator=g).to(dtype)
    q = torch.randn(B, Tq, Hq, D, generator=g).bfloat16()
    ctx = torch.tensor([c for c, _ in specs], dtype=torch.int32)
    ql = torch.tensor([n for _, n in specs], dtype=torch.int32)
    scales = (0.5, 2.0) if dtype == FP8 else (1.0, 1.0)
    ref = ops.paged_attention_prefill_ref(q, kc, vc, bt, ctx, ql, *scales)
    return (q, kc, vc, bt, ctx, ql), scales, ref.float()


def _run(args, scales, S):
    dev = torch.device("cuda", 0)
    out = ops.paged_attention_verify(*(a.to(dev) for a in args), num_splits=S,
                                     k_scale=scales[0], v_scale=scales[1])
    return out.float().cpu()


def _check(out, ref):
    # the bound of tests/test_paged_prefill.py::_check: same reference,
    # same arithmetic
    assert torch.isfinite(out).all()
    assert torch.allclose(out, ref, atol=4e-2, rtol=4e-2), \
        float((out - ref).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("ctx,q_len", [(0, 1), (0, 8), (15, 2), (16, 1),
                                       (17, 8), (63, 2), (64, 3), (300, 4)])
@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (8, 2), (4, 4), (8, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_verify_matches_prefill_ref(D, Hq, Hkv, ctx, q_len, S):
    if q_len * (Hq // Hkv) > ops.VERIFY_MAX_ROWS:
        pytest.skip("q_len * REP > 32 is out of the kernel's range")
    args, scales, ref = _case(D, Hq, Hkv, ((ctx, q_len),), q_len)
    _check(_run(args, scales, S), ref)


BATCH = ((40, 3), (9, 0), (0, 8), (130, 1), (65, 5))


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("dtype", [torch.bfloat16, FP8])
def test_verify_batch_padding_rows_are_zero(dtype, S):
    """Five sequences, Tq 8 at REP 4, in a pool poisoned with NaN
    everywhere a sequence has no row: rows i >= q_len and the q_len 0
    sequence are exactly zero, the rest is finite and within the bound."""
    args, scales, ref = _case(128, 8, 2, BATCH, 8, dtype, float("nan"))
    out = _run(args, scales, S)
    _check(out, ref)
    for b, (_, n) in enumerate(BATCH):
        assert (out[b, n:] == 0).all()
        assert n == 0 or (out[b, :n] != 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("ctx,q_len", [(17, 8), (63, 2), (300, 4)])
def test_verify_poisoned_pool(ctx, q_len, S):
    args, scales, ref = _case(64, 4, 2, ((ctx, q_len),), 8,
                              fill=float("nan"))
    _check(_run(args, scales, S), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("rep", [2, 4])
@pytest.mark.parametrize("ctx", [13, 64])
@pytest.mark.parametrize("i0", [0, 3, 6])
def test_verify_key_inclusion_exact(i0, ctx, rep, S):
    """q = 0 makes every row's softmax uniform over the keys it sees; V is
    zero except V[ctx + i0 + 1, 0] = 1. Row i sees that key iff i > i0."""
    Tq, Hkv, D = 8, 2, 64
    (q, kc, vc, bt, c, ql), _, _ = _case(D, Hkv * rep, Hkv, ((ctx, Tq),), Tq)
    vc = torch.zeros_like(vc)
    p = ctx + i0 + 1
    vc[bt[0, p // PAGE].long(), :, p % PAGE, 0] = 1.0
    out = _run((torch.zeros_like(q), kc, vc, bt, c, ql), (1.0, 1.0), S)[0]
    assert (out[: i0 + 1, :, 0] == 0).all()
    for i in range(i0 + 1, Tq):
        want = 1.0 / (ctx + i + 1)
        ulp = 2.0 ** (torch.tensor(want).log2().floor().item() - 7)
        assert ((out[i, :, 0] - want).abs() <= ulp).all(), (i, out[i, :, 0])


@pytest.mark.gpu
def test_verify_captured_replay_follows_device_state():
    dev = torch.device("cuda", 0)
    specs = ((70, 2), (3, 8), (200, 5))
    a, _, _ = _case(128, 8, 2, specs, 8, seed=1)
    b, _, _ = _case(128, 8, 2, specs[::-1], 8, seed=2)
    S = 3
    # b's pool is the same size: both have the same page count
    q, kc, vc, bt, ctx, ql = (t.to(dev).clone() for t in a)
    ws = torch.empty(3 * 8 * 8 * S * (128 + 2), device=dev)
    call = functools.partial(ops.paged_attention_verify, q, kc, vc, bt, ctx,
                             ql, num_splits=S, workspace=ws)
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for src in (b, a):
        for dst, t in zip((q, kc, vc, bt, ctx, ql), src):
            dst.copy_(t)
        for _ in range(2):
            graph.replay()
            assert torch.equal(out, call())


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, FP8])
def test_rope_append_paged_multi_matches_ref(dtype, D):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(D)
    B, Tq, Hq, Hkv = 4, 4, 4, 2
    scales = (0.5, 2.0) if dtype == FP8 else (1.0, 1.0)
    fused = torch.randn(B, Tq, (Hq + 2 * Hkv) * D, generator=g).bfloat16()
    pos0 = torch.tensor([0, 14, -1, 37], dtype=torch.int32)
    q_lens = torch.tensor([4, 4, 4, 2], dtype=torch.int32)
    bt = (torch.randperm(B * 3, generator=g).int() + 1).view(B, 3)
    cache = torch.randn(B * 3 + 1, Hkv, PAGE, D, generator=g)
    cosT, sinT = ops.rope_tables(64, D)

    def run(device, fn):
        f = fused.to(device)
        q, k, v = (t.view(B, Tq, -1, D) for t in f.split(
            [Hq * D, Hkv * D, Hkv * D], dim=-1))
        kc, vc = cache.to(dtype).to(device), (-cache).to(dtype).to(device)
        qr = fn(q, k, v, cosT.to(device), sinT.to(device), pos0.to(device),
                q_lens.to(device), bt.to(device), kc, vc, *scales)
        return qr.float().cpu(), kc.cpu(), vc.cpu()

    got = run(dev, ops.rope_append_paged_multi)
    want = run("cpu", ops.rope_append_paged_multi_ref)
    # q and bf16 pages: the tolerance of tests/test_hip_ops.py for rope
    assert torch.allclose(got[0], want[0], atol=2e-2, rtol=2e-2)
    assert (got[0][2] == 0).all() and (got[0][3, 2:] == 0).all()
    written = torch.zeros(B * 3 + 1, PAGE, dtype=torch.bool)
    for b in range(B):
        for i in range(int(q_lens[b]) if pos0[b] >= 0 else 0):
            p = int(pos0[b]) + i
            written[bt[b, p // PAGE].long(), p % PAGE] = True
    for got_c, want_c, old in ((got[1], want[1], cache), (got[2], want[2],
                                                          -cache)):
        if dtype == FP8:
            assert torch.equal(got_c.view(torch.uint8),
                               want_c.view(torch.uint8))
        else:
            assert torch.allclose(got_c.float(), want_c.float(), atol=2e-2,
                                  rtol=2e-2)
        keep = ~written[:, None, :, None].expand_as(got_c)
        assert torch.equal(got_c.float()[keep], old.to(dtype).float()[keep])


def test_verify_on_cpu_is_the_prefill_ref():
    (q, kc, vc, bt, ctx, ql), _, ref = _case(64, 4, 2, ((10, 3), (0, 2)), 3)
    out = ops.paged_attention_verify(q, kc, vc, bt, ctx, ql)
    assert torch.equal(out.float(), ref)


@pytest.mark.gpu
def test_verify_binding_errors():
    dev = torch.device("cuda", 0)

    def call(Tq, Hq, D, **kw):
        q = torch.zeros(1, Tq, Hq, D, device=dev, dtype=torch.bfloat16)
        kc = torch.zeros(4, 2, PAGE, D, device=dev, dtype=torch.bfloat16)
        z = torch.zeros(1, dtype=torch.int32, device=dev)
        return ops.paged_attention_verify(
            q, kc, kc.clone(), torch.ones(1, 2, dtype=torch.int32,
                                          device=dev), z, z + 1, **kw)

    call(8, 8, 64, num_splits=2)
    with pytest.raises(RuntimeError, match="Tq \\* \\(Hq/Hkv\\)"):
        call(9, 8, 64, num_splits=1)
    with pytest.raises(RuntimeError, match="head_dim must be 64 or 128"):
        call(2, 4, 96, num_splits=1)
    with pytest.raises(RuntimeError, match="workspace"):
        call(8, 8, 64, num_splits=2,
             workspace=torch.empty(8 * 8 * 2 * 66 - 1, device=dev))
