"""FP8 (OCP e4m3fn) paged KV cache: the quantisation rule, the
references, the pool and the engine on CPU; the fp8 instantiations of
the decode, prefill and append kernels against the references on GPU.

GPU cases live in caches whose every byte outside the valid rows (the
null page, unallocated pages, tail slots of last pages) is 0x7F, the
e4m3fn NaN."""
import functools

import pytest
import torch

from ray_amd import ops
from ray_amd.llm import ContinuousBatchingEngine, LLMConfig
from ray_amd.llm.paged import PagedDecoder, PagedKVPool
from ray_amd.models.llama import CONFIGS, LlamaModel

PAGE = 16
FP8 = torch.float8_e4m3fn
NAN_BYTE = 0x7F
SCALES = [(1.0, 1.0), (0.5, 2.0)]


def _bytes(t):
    return t.view(torch.uint8)


def _fp8_full(shape, byte, device="cpu"):
    return torch.full(shape, byte, dtype=torch.uint8, device=device).view(FP8)


# --------------------------------------------------------------------------
# CPU: the quantisation rule
# --------------------------------------------------------------------------


def _q(vals, scale=1.0, dtype=torch.float32):
    return ops.quantize_kv_fp8(torch.tensor(vals, dtype=dtype), scale)


def test_quantize_saturates_instead_of_nan():
    out = _q([1000.0, -1000.0, 448.0, 460.0, -460.0, 464.0, 1e30])
    assert out.dtype == FP8
    assert out.float().tolist() == [448.0, -448.0, 448.0, 448.0, -448.0,
                                    448.0, 448.0]
    # the bare conversion does not saturate, which is why the rule clamps
    assert torch.isnan(torch.tensor([1000.0]).to(FP8).float()).all()


def test_quantize_rounds_to_nearest_even():
    # e4m3fn: 3 mantissa bits; spacing 2 in [16, 32), 2^-9 below 2^-6
    out = _q([17.0, 19.0, 16.9, 17.1, 2.0 ** -10, 3 * 2.0 ** -10,
              2.0 ** -9, 0.3])
    assert out.float().tolist() == [16.0, 20.0, 16.0, 18.0, 0.0, 2.0 ** -8,
                                    2.0 ** -9, 0.3125]
    assert _bytes(_q([0.0, -0.0])).tolist() == [0x00, 0x80]


def test_quantize_scales():
    # stored = x / scale; dequantised = stored * scale
    # 200 is halfway between 192 and 208 (spacing 16); 192 is the even one
    assert _q([1.0, 100.0, 101.0, 300.0], 0.5).float().tolist() == [
        2.0, 192.0, 208.0, 448.0]
    # 1/3 is not exact in fp32: 3 * fp32(1/3) rounds to 1 in fp32
    assert _q([3.0, 51.0, 1500.0, -6.0], 3.0).float().tolist() == [
        1.0, 16.0, 448.0, -2.0]


def test_quantize_bf16_and_fp32_inputs_agree():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(4096, generator=g) * 40).bfloat16()
    for s in (1.0, 0.5, 3.0):
        a, b = ops.quantize_kv_fp8(x, s), ops.quantize_kv_fp8(x.float(), s)
        assert torch.equal(_bytes(a), _bytes(b))
        assert torch.isfinite(a.float()).all()


@pytest.mark.parametrize("bad", [0.0, -1.0, float("inf"), float("nan")])
def test_quantize_rejects_bad_scale(bad):
    with pytest.raises(ValueError):
        ops.quantize_kv_fp8(torch.zeros(4), bad)


# --------------------------------------------------------------------------
# CPU: references on fp8 caches
# --------------------------------------------------------------------------


def _fp8_cache_and_table(g, specs, Hkv, D, num_pages, k_scale, v_scale,
                         device="cpu"):
    """fp8 K/V caches of NaN bytes, a block table that is a random
    permutation of pages 1..num_pages-1 with unused entries 0, and
    quantised random values in exactly the first L rows of each
    sequence. specs is [L]."""
    B = len(specs)
    max_pages = max(1, max(-(-L // PAGE) for L in specs))
    kc = _fp8_full((num_pages, Hkv, PAGE, D), NAN_BYTE)
    vc = _fp8_full((num_pages, Hkv, PAGE, D), NAN_BYTE)
    perm = (torch.randperm(num_pages - 1, generator=g) + 1).tolist()
    bt = torch.zeros(B, max_pages, dtype=torch.int32)
    for b, L in enumerate(specs):
        for i in range(-(-L // PAGE)):
            pg = perm.pop()
            bt[b, i] = pg
            rows = min(PAGE, L - i * PAGE)
            kc[pg, :, :rows] = ops.quantize_kv_fp8(
                torch.randn(Hkv, rows, D, generator=g), k_scale)
            vc[pg, :, :rows] = ops.quantize_kv_fp8(
                torch.randn(Hkv, rows, D, generator=g), v_scale)
    return kc, vc, bt


def _dequant(cache, scale):
    """The fp32 cache an fp8 cache stands for; NaN bytes become zeros so
    the fp32 run and the fp8 run differ in nothing but the format."""
    return torch.nan_to_num(cache.float() * scale, nan=0.0)


@pytest.mark.parametrize("k_scale,v_scale", SCALES)
def test_decode_ref_on_fp8_cache_equals_ref_on_dequantised_cache(k_scale,
                                                                 v_scale):
    g = torch.Generator().manual_seed(0)
    lens = [37, 16, 5, 0]
    kc, vc, bt = _fp8_cache_and_table(g, lens, 2, 64, 24, k_scale, v_scale)
    row = bt[0, :3].tolist()
    assert row != sorted(row)  # the table really is shuffled
    q = torch.randn(len(lens), 4, 64, generator=g)
    sl = torch.tensor(lens, dtype=torch.int32)
    out = ops.paged_attention_ref(q, kc, vc, bt, sl, k_scale, v_scale)
    want = ops.paged_attention_ref(q, _dequant(kc, k_scale),
                                   _dequant(vc, v_scale), bt, sl)
    assert torch.isfinite(out).all() and (out[3] == 0).all()
    assert torch.allclose(out, want, atol=1e-5, rtol=0)
    # and the dispatching op takes the same path on CPU
    assert torch.equal(out, ops.paged_attention_decode(
        q, kc, vc, bt, sl, k_scale=k_scale, v_scale=v_scale))


@pytest.mark.parametrize("k_scale,v_scale", SCALES)
def test_prefill_ref_on_fp8_cache_equals_ref_on_dequantised_cache(k_scale,
                                                                  v_scale):
    g = torch.Generator().manual_seed(1)
    specs = [(17, 20), (60, 3), (0, 5)]
    kc, vc, bt = _fp8_cache_and_table(g, [c + n for c, n in specs], 2, 64,
                                      24, k_scale, v_scale)
    q = torch.randn(len(specs), 20, 4, 64, generator=g)
    ctx = torch.tensor([c for c, _ in specs], dtype=torch.int32)
    ql = torch.tensor([n for _, n in specs], dtype=torch.int32)
    out = ops.paged_attention_prefill_ref(q, kc, vc, bt, ctx, ql, k_scale,
                                          v_scale)
    want = ops.paged_attention_prefill_ref(q, _dequant(kc, k_scale),
                                           _dequant(vc, v_scale), bt, ctx, ql)
    assert torch.isfinite(out).all()
    assert torch.allclose(out, want, atol=1e-5, rtol=0)
    assert torch.equal(out, ops.paged_attention_prefill(
        q, kc, vc, bt, ctx, ql, k_scale, v_scale))


SENTINEL = 0x5A  # an ordinary finite e4m3fn byte (= 52.0)


@pytest.mark.parametrize("k_scale,v_scale", SCALES)
def test_rope_append_ref_fp8_cache(k_scale, v_scale):
    g = torch.Generator().manual_seed(2)
    B, Hq, Hkv, D = 3, 4, 2, 64
    cosT, sinT = ops.rope_tables(64, D)
    q = torch.randn(B, Hq, D, generator=g).bfloat16()
    k = (torch.randn(B, Hkv, D, generator=g) * 3).bfloat16()
    v = (torch.randn(B, Hkv, D, generator=g) * 3).bfloat16()
    bt = torch.tensor([[1, 2], [3, 4], [5, 6]], dtype=torch.int32)
    pos = torch.tensor([0, 17, -1], dtype=torch.int32)
    kc, vc = (_fp8_full((8, Hkv, PAGE, D), SENTINEL) for _ in range(2))
    kb = torch.zeros(8, Hkv, PAGE, D, dtype=torch.bfloat16)
    vb = torch.zeros_like(kb)
    q8 = ops.rope_append_paged(q, k, v, cosT, sinT, pos, bt, kc, vc,
                               k_scale, v_scale)
    qb = ops.rope_append_paged(q, k, v, cosT, sinT, pos, bt, kb, vb)
    assert torch.equal(q8, qb) and (q8[2] == 0).all()
    written = torch.zeros(8, PAGE, dtype=torch.bool)
    for pg, sl in [(1, 0), (4, 1)]:
        written[pg, sl] = True
        # the bytes are the rule applied to what the bf16 cache holds
        assert torch.equal(
            _bytes(kc[pg, :, sl]),
            _bytes(ops.quantize_kv_fp8(kb[pg, :, sl], k_scale)))
        assert torch.equal(
            _bytes(vc[pg, :, sl]),
            _bytes(ops.quantize_kv_fp8(vb[pg, :, sl], v_scale)))
    for cache in (kc, vc):  # pos -1 wrote nothing, nor did anything else
        assert (_bytes(cache).permute(0, 2, 1, 3)[~written] == SENTINEL).all()


def _append_case(g, T, Hkv, D, dtype=torch.bfloat16):
    k = (torch.randn(T, Hkv, D, generator=g) * 3).to(dtype)
    v = (torch.randn(T, Hkv, D, generator=g) * 3).to(dtype)
    return k, v


def _append_expected(k, v, pos0, row, num_pages, k_scale, v_scale):
    """Expected fp8 cache bytes after kv_append_paged into sentinel
    caches, written out independently of the op's reference."""
    T, Hkv, D = k.shape
    kq, vq = ops.quantize_kv_fp8(k, k_scale), ops.quantize_kv_fp8(v, v_scale)
    kc, vc = (_fp8_full((num_pages, Hkv, PAGE, D), SENTINEL)
              for _ in range(2))
    for t in range(T):
        p = pos0 + t
        if p // PAGE < len(row) and 0 <= row[p // PAGE] < num_pages:
            kc[row[p // PAGE], :, p % PAGE] = kq[t]
            vc[row[p // PAGE], :, p % PAGE] = vq[t]
    return kc, vc


@pytest.mark.parametrize("T,pos0", [(1, 0), (16, 5), (37, 16)])
def test_kv_append_ref_fp8_cache(T, pos0):
    g = torch.Generator().manual_seed(T + pos0)
    Hkv, D, P = 2, 64, 9
    k, v = _append_case(g, T, Hkv, D)
    row = [7, 3, 8, 1]
    kc, vc = (_fp8_full((P, Hkv, PAGE, D), SENTINEL) for _ in range(2))
    ops.kv_append_paged(k, v, pos0, torch.tensor(row, dtype=torch.int32),
                        kc, vc, 0.5, 2.0)
    ke, ve = _append_expected(k, v, pos0, row, P, 0.5, 2.0)
    assert torch.equal(_bytes(kc), _bytes(ke))
    assert torch.equal(_bytes(vc), _bytes(ve))
    assert int((_bytes(kc) != SENTINEL).any(-1).sum()) <= T * Hkv


def test_kv_append_ref_skips_rows_outside_table_and_pool():
    g = torch.Generator().manual_seed(5)
    k, v = _append_case(g, 40, 2, 64)
    row = [2, 9, 1]  # page id 9 is outside a pool of 4; rows 48.. have no entry
    kc, vc = (_fp8_full((4, 2, PAGE, 64), SENTINEL) for _ in range(2))
    ops.kv_append_paged_ref(k, v, 10, torch.tensor(row, dtype=torch.int32),
                            kc, vc)
    ke, ve = _append_expected(k, v, 10, row, 4, 1.0, 1.0)
    assert torch.equal(_bytes(kc), _bytes(ke))
    assert torch.equal(_bytes(vc), _bytes(ve))
    assert (_bytes(kc[2, :, :10]) == SENTINEL).all()
    assert (_bytes(kc[2, :, 10:]) != SENTINEL).any()
    assert (_bytes(kc[1]) != SENTINEL).any()   # rows 32..47
    assert (_bytes(kc[[0, 3]]) == SENTINEL).all()


def test_kv_append_ref_bf16_cache_stores_values():
    g = torch.Generator().manual_seed(6)
    k, v = _append_case(g, 5, 2, 64)
    kc = torch.zeros(4, 2, PAGE, 64, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    ops.kv_append_paged(k, v, 14, torch.tensor([3, 1], dtype=torch.int32),
                        kc, vc)
    assert torch.equal(kc[3, :, 14:], k[:2].transpose(0, 1))
    assert torch.equal(vc[1, :, :3], v[2:].transpose(0, 1))


# --------------------------------------------------------------------------
# CPU: pool, decoder, engine
# --------------------------------------------------------------------------


def test_pool_fp8_is_half_the_bytes():
    dev = torch.device("cpu")
    a = PagedKVPool(3, 8, 2, 64, dev, torch.bfloat16)
    b = PagedKVPool(3, 8, 2, 64, dev, FP8, k_scale=0.5, v_scale=2.0)
    assert a.kv_bytes == 2 * 3 * 8 * 2 * PAGE * 64 * 2
    assert b.kv_bytes * 2 == a.kv_bytes
    assert b.is_fp8 and not a.is_fp8
    assert b.k[0].dtype == FP8 and (b.k_scale, b.v_scale) == (0.5, 2.0)


def test_pool_rejects_other_fp8_flavours_and_bad_scales():
    dev = torch.device("cpu")
    for dt in (torch.float8_e4m3fnuz, torch.float8_e5m2):
        with pytest.raises(ValueError):
            PagedKVPool(1, 4, 1, 64, dev, dt)
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            PagedKVPool(1, 4, 1, 64, dev, FP8, k_scale=bad)
        with pytest.raises(ValueError):
            PagedKVPool(1, 4, 1, 64, dev, FP8, v_scale=bad)
    with pytest.raises(ValueError):  # a scale means nothing to a bf16 pool
        PagedKVPool(1, 4, 1, 64, dev, torch.bfloat16, k_scale=0.5)


def _tiny(dev, dtype):
    cfg = CONFIGS["llama-tiny"]
    torch.manual_seed(0)
    m = LlamaModel(cfg, dtype=dtype).to(dev).eval()
    m.cosT = m.cosT.to(dev)
    m.sinT = m.sinT.to(dev)
    return m


def _rel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-6))


_CPU = {}


def _cpu_model_and_whole_prompt_logits():
    """llama-tiny in fp32 and the fp8-pool whole-prompt prefill logits of
    a 37-token prompt, computed once."""
    if not _CPU:
        m = _tiny(torch.device("cpu"), torch.float32)
        prompt = torch.arange(3, 40) * 7 % 512
        with torch.no_grad():
            pd = PagedDecoder(m, 1, 96, torch.device("cpu"), kv_dtype=FP8)
            _CPU.update(m=m, prompt=prompt,
                        logits=pd.prefill_slot(0, prompt).clone())
    return _CPU["m"], _CPU["prompt"], _CPU["logits"]


def test_fp8_whole_prompt_prefill_goes_through_the_pages_cpu():
    """With an fp8 pool and no flag set, prefill is one chunk through
    the paged path: the pages hold quantised rows and the logits differ
    from the bf16-pool ones by the quantisation, not by nothing."""
    m, prompt, got = _cpu_model_and_whole_prompt_logits()
    dev = torch.device("cpu")
    with torch.no_grad():
        plain = PagedDecoder(m, 1, 96, dev).prefill_slot(0, prompt)
        pd = PagedDecoder(m, 1, 96, dev, kv_dtype=FP8)
        again = pd.prefill_slot(0, prompt)
    assert torch.equal(again, got)
    assert pd.pool.k[0].dtype == FP8
    assert pd.prefill_tokens_computed == 37
    r = _rel(got, plain)
    print(f"fp8 vs unquantised whole-prompt logits: rel L2 {r:.3e}")
    assert r > 0
    pages = pd._slot_pages[0][:3]
    assert torch.isfinite(pd.pool.k[0][pages[:2]].float()).all()


@pytest.mark.parametrize("chunk", [1, 7, 16, 40])
def test_fp8_chunked_prefill_matches_whole_prompt_cpu(chunk):
    """Chunking changes the fp32 summation order of the attention that
    produces the next layer's K; one K element landing on another fp8
    code would break this bound, and for this prompt none does."""
    m, prompt, want = _cpu_model_and_whole_prompt_logits()
    pd = PagedDecoder(m, 1, 96, torch.device("cpu"), prefill_chunk=chunk,
                      kv_dtype=FP8)
    with torch.no_grad():
        got = pd.prefill_slot(0, prompt)
    r = _rel(got, want)
    print(f"chunk {chunk}: rel L2 {r:.3e}")
    assert r < 1e-4
    assert int(pd.seq_lens[0]) == 37
    pd.release_slot(0)
    assert pd.pool.num_free == pd.pool.num_usable


def test_fp8_prefix_hit_prefill_matches_cold_cpu():
    m, prompt, want = _cpu_model_and_whole_prompt_logits()
    pd = PagedDecoder(m, 2, 96, torch.device("cpu"), prefix_caching=True,
                      kv_dtype=FP8)
    with torch.no_grad():
        cold = pd.prefill_slot(0, prompt)
        shared = pd._slot_pages[0][:2]
        before = [(_bytes(pd.pool.k[li][shared]).clone(),
                   _bytes(pd.pool.v[li][shared]).clone())
                  for li in range(len(pd.pool.k))]
        warm = pd.prefill_slot(1, prompt)
    assert pd.prefix_hit_tokens == 32 and pd.prefill_tokens_computed == 37 + 5
    assert pd._slot_pages[1][:2] == shared
    for li, (k0, v0) in enumerate(before):
        assert torch.equal(_bytes(pd.pool.k[li][shared]), k0)
        assert torch.equal(_bytes(pd.pool.v[li][shared]), v0)
    for name, got in (("cold", cold), ("warm", warm)):
        r = _rel(got, want)
        print(f"{name}: rel L2 {r:.3e}")
        assert r < 1e-4


def _engine_prompts():
    prefix = [(11 * i + 5) % 512 for i in range(40)]
    return [prefix + [300, 301, 302], prefix + [310 + i for i in range(9)],
            list(range(100, 104))]


def test_engine_fp8_runs_deterministic_and_returns_pages_cpu():
    def run():
        eng = ContinuousBatchingEngine(LLMConfig(
            model_id="llama-tiny", max_seq_len=96, max_batch_size=2,
            use_hip_graph=False, kv_cache="paged", kv_cache_dtype="fp8",
            kv_k_scale=0.5, kv_v_scale=2.0))
        pool = eng.decoder.pool
        assert pool.k[0].dtype == FP8
        assert (pool.k_scale, pool.v_scale) == (0.5, 2.0)
        assert eng.stats["kv_cache_bytes"] == pool.kv_bytes
        ids = [eng.submit(p, max_new_tokens=n)
               for p, n in zip(_engine_prompts(), [6, 5, 9])]
        out = eng.run_until_complete()
        assert eng.stats["kv_pages_free"] == eng.stats["kv_pages_total"] == 12
        return [out[i] for i in ids], eng.stats["kv_cache_bytes"]

    (a, nbytes), (b, _) = run(), run()
    assert a == b and [len(r) for r in a] == [6, 5, 9]
    ref = ContinuousBatchingEngine(LLMConfig(
        model_id="llama-tiny", max_seq_len=96, max_batch_size=2,
        use_hip_graph=False, kv_cache="paged", kv_cache_dtype="bf16"))
    assert ref.decoder.pool.k[0].dtype == torch.bfloat16
    assert ref.stats["kv_cache_bytes"] == 2 * nbytes
    alias = ContinuousBatchingEngine(LLMConfig(
        model_id="llama-tiny", max_seq_len=96, use_hip_graph=False,
        kv_cache="paged", kv_cache_dtype="fp8_e4m3"))
    assert alias.decoder.pool.is_fp8


def test_engine_fp8_shared_page_bits_unchanged_by_second_request_cpu():
    prompts = _engine_prompts()
    eng = ContinuousBatchingEngine(LLMConfig(
        model_id="llama-tiny", max_seq_len=96, max_batch_size=2,
        use_hip_graph=False, kv_cache="paged", enable_prefix_caching=True,
        kv_cache_dtype="fp8"))
    eng.submit(prompts[0], max_new_tokens=8)
    eng.step()
    pool = eng.decoder.pool
    shared = list(eng.decoder._slot_pages[0][:2])
    before = [(_bytes(k[shared]).clone(), _bytes(v[shared]).clone())
              for k, v in zip(pool.k, pool.v)]
    eng.submit(prompts[1], max_new_tokens=8)
    eng.step()
    assert eng.decoder._slot_pages[1][:2] == shared
    assert eng.stats["prefix_hit_tokens"] == 32
    eng.run_until_complete()
    for (k0, v0), k, v in zip(before, pool.k, pool.v):
        assert torch.equal(_bytes(k[shared]), k0)
        assert torch.equal(_bytes(v[shared]), v0)
    assert eng.stats["kv_pages_free"] == eng.stats["kv_pages_total"]


def test_engine_fp8_validation():
    def cfg(**kw):
        return LLMConfig(model_id="llama-tiny", max_seq_len=64,
                         use_hip_graph=False, **kw)

    with pytest.raises(ValueError):
        ContinuousBatchingEngine(cfg(kv_cache="paged", kv_cache_dtype="int8"))
    with pytest.raises(ValueError):
        ContinuousBatchingEngine(cfg(kv_cache="paged",
                                     kv_cache_dtype="fp8_e5m2"))
    with pytest.raises(ValueError):  # fp8 needs the paged cache
        ContinuousBatchingEngine(cfg(kv_cache_dtype="fp8"))
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            ContinuousBatchingEngine(cfg(kv_cache="paged",
                                         kv_cache_dtype="fp8",
                                         kv_k_scale=bad))
    with pytest.raises(ValueError):
        ContinuousBatchingEngine(cfg(kv_cache="paged", kv_cache_dtype="fp8",
                                     kv_v_scale=float("nan")))


# --------------------------------------------------------------------------
# GPU: decode kernel vs paged_attention_ref on the same fp8 bytes
# --------------------------------------------------------------------------


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _decode_case(D, Hq, Hkv, lens, num_pages, k_scale, v_scale, seed):
    g = torch.Generator().manual_seed(seed)
    kc, vc, bt = _fp8_cache_and_table(g, list(lens), Hkv, D, num_pages,
                                      k_scale, v_scale)
    q = torch.randn(len(lens), Hq, D, generator=g).bfloat16()
    sl = torch.tensor(lens, dtype=torch.int32)
    ref = ops.paged_attention_ref(q, kc, vc, bt, sl, k_scale, v_scale)  # CPU
    assert (_bytes(kc[0]) == NAN_BYTE).all()  # the null page is poison
    return tuple(t.to(_dev()) for t in (q, kc, vc, bt, sl)) + (ref,)


def _check(out, ref, atol=4e-2, rtol=4e-2):
    out = out.float().cpu()
    ref = ref.float()
    assert torch.isfinite(out).all()
    err = float((out - ref).abs().max())
    print(f"max abs err {err:.3e}")
    assert torch.allclose(out, ref, atol=atol, rtol=rtol), err


@pytest.mark.gpu
@pytest.mark.parametrize("k_scale,v_scale", SCALES)
@pytest.mark.parametrize("num_splits", [1, 4])
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (4, 2), (8, 2), (8, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_fp8_decode_kernel_short(D, Hq, Hkv, num_splits, k_scale, v_scale):
    q, kc, vc, bt, sl, ref = _decode_case(D, Hq, Hkv, (1, 15, 16, 17, 0), 64,
                                          k_scale, v_scale, D + Hq + Hkv)
    out = ops.paged_attention_decode(q, kc, vc, bt, sl,
                                     num_splits=num_splits, k_scale=k_scale,
                                     v_scale=v_scale)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    _check(out, ref)
    assert (out[4] == 0).all()  # seq_len 0 row is exactly zero


@pytest.mark.gpu
@pytest.mark.parametrize("k_scale,v_scale", SCALES)
@pytest.mark.parametrize("D,Hq,Hkv", [(64, 8, 2), (128, 8, 1), (128, 4, 4),
                                      (64, 4, 2)])
def test_fp8_decode_kernel_long_and_split_consistency(D, Hq, Hkv, k_scale,
                                                      v_scale):
    q, kc, vc, bt, sl, ref = _decode_case(D, Hq, Hkv, (1000, 33), 72,
                                          k_scale, v_scale, 7 + D)
    outs = {}
    for s in (1, 3, 8):
        outs[s] = ops.paged_attention_decode(q, kc, vc, bt, sl, num_splits=s,
                                             k_scale=k_scale,
                                             v_scale=v_scale)
        _check(outs[s], ref)
    for s in (3, 8):
        d = float((outs[s].float() - outs[1].float()).abs().max())
        print(f"splits {s} vs 1: max abs diff {d:.3e}")
        assert torch.allclose(outs[s].float(), outs[1].float(), atol=2e-2,
                              rtol=0), (s, d)


# --------------------------------------------------------------------------
# GPU: every finite byte code through both attention kernels
# --------------------------------------------------------------------------

ALL_CODES_SCALE = 2.0 ** -6


@functools.lru_cache(maxsize=None)
def _all_codes_case(D):
    """One 48-row sequence whose K and V bytes cycle through the 254
    finite e4m3fn codes (subnormals, +-448 and -0 included), at
    different phases for K and V. Both scales are 2^-6, which maps the
    code range +-448 to +-7: the dequantised values then have the unit
    scale that the project's 4e-2 tolerance is written for, and the
    power of two keeps them exact."""
    Hq, Hkv, L, P = 4, 2, 48, 6
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F],
                         dtype=torch.uint8)
    assert codes.numel() == 254
    n = Hkv * L * D
    idx = torch.arange(n)
    # [L, Hkv, D] so consecutive codes run along a row
    kb = codes[idx % 254].view(L, Hkv, D)
    vb = codes[(idx * 5 + 101) % 254].view(L, Hkv, D)  # 5 is coprime to 254
    assert set(kb.flatten().tolist()) == set(codes.tolist())
    assert set(vb.flatten().tolist()) == set(codes.tolist())
    kc = _fp8_full((P, Hkv, PAGE, D), NAN_BYTE)
    vc = _fp8_full((P, Hkv, PAGE, D), NAN_BYTE)
    pages = [4, 1, 3]
    for i, pg in enumerate(pages):
        rows = slice(i * PAGE, (i + 1) * PAGE)
        _bytes(kc)[pg] = kb[rows].transpose(0, 1)
        _bytes(vc)[pg] = vb[rows].transpose(0, 1)
    bt = torch.tensor([pages], dtype=torch.int32)
    g = torch.Generator().manual_seed(D)
    q = torch.randn(1, L, Hq, D, generator=g).bfloat16()
    return q, kc, vc, bt


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 128])
def test_fp8_all_codes_through_decode_and_prefill_kernels(D):
    q, kc, vc, bt = _all_codes_case(D)
    s = ALL_CODES_SCALE
    L = q.shape[1]
    dev = _dev()
    kd, vd, btd = kc.to(dev), vc.to(dev), bt.to(dev)
    # decode: the last query row over all 48 rows, and over 47
    for n in (L, L - 1):
        sl = torch.tensor([n], dtype=torch.int32)
        qd = q[:, n - 1].contiguous()
        ref = ops.paged_attention_ref(qd, kc, vc, bt, sl, s, s)
        for splits in (1, 2):
            out = ops.paged_attention_decode(qd.to(dev), kd, vd, btd,
                                             sl.to(dev), num_splits=splits,
                                             k_scale=s, v_scale=s)
            _check(out, ref)
    # prefill: all 48 rows as one causal chunk
    ctx = torch.tensor([0], dtype=torch.int32)
    ql = torch.tensor([L], dtype=torch.int32)
    ref = ops.paged_attention_prefill_ref(q, kc, vc, bt, ctx, ql, s, s)
    out = ops.paged_attention_prefill(q.to(dev), kd, vd, btd, ctx.to(dev),
                                      ql.to(dev), s, s)
    _check(out, ref)


# --------------------------------------------------------------------------
# GPU: prefill kernel
# --------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _prefill_case(D, Hq, Hkv, specs, Tq, k_scale, v_scale, seed):
    g = torch.Generator().manual_seed(seed)
    need = sum(-(-(c + n) // PAGE) for c, n in specs)
    kc, vc, bt = _fp8_cache_and_table(g, [c + n for c, n in specs], Hkv, D,
                                      need + 3, k_scale, v_scale)
    q = torch.randn(len(specs), Tq, Hq, D, generator=g).bfloat16()
    ctx = torch.tensor([c for c, _ in specs], dtype=torch.int32)
    ql = torch.tensor([n for _, n in specs], dtype=torch.int32)
    ref = ops.paged_attention_prefill_ref(q, kc, vc, bt, ctx, ql, k_scale,
                                          v_scale)  # CPU, fp32 math
    return tuple(t.to(_dev()) for t in (q, kc, vc, bt, ctx, ql)) + (ref,)


@pytest.mark.gpu
@pytest.mark.parametrize("k_scale,v_scale", SCALES)
@pytest.mark.parametrize("ctx,Tq", [(0, 1), (15, 17), (60, 70), (100, 130),
                                    (5, 260)])
@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (8, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_fp8_prefill_kernel_shape_grid(D, Hq, Hkv, ctx, Tq, k_scale, v_scale):
    q, kc, vc, bt, cl, ql, ref = _prefill_case(
        D, Hq, Hkv, ((ctx, Tq),), Tq, k_scale, v_scale,
        D + Hq + Hkv + ctx + Tq)
    out = ops.paged_attention_prefill(q, kc, vc, bt, cl, ql, k_scale, v_scale)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    _check(out, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 128])
def test_fp8_prefill_kernel_wide_tile_dispatch(D):
    """B 22, Tq 260, Hq 8 is 528 blocks of 128 query rows: past the 512
    at which the binding launches 8-wave, 256-row tiles. Mixed contexts
    and some short and empty rows."""
    B, Tq, Hq, Hkv = 22, 260, 8, 2
    assert -(-Tq // 128) * Hq * B >= 512
    specs = tuple(((13 * b) % 90, Tq if b % 5 else (7 * b) % (Tq + 1))
                  for b in range(B))
    q, kc, vc, bt, cl, ql, ref = _prefill_case(D, Hq, Hkv, specs, Tq, 0.5,
                                               2.0, B + D)
    out = ops.paged_attention_prefill(q, kc, vc, bt, cl, ql, 0.5, 2.0)
    _check(out, ref)
    for b, (_, n) in enumerate(specs):
        assert (out[b, n:] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 128])
def test_fp8_prefill_kernel_batch_with_padding(D):
    Tq = 40
    specs = ((33, 40), (70, 23), (12, 0))
    q, kc, vc, bt, cl, ql, ref = _prefill_case(D, 8, 2, specs, Tq, 0.5, 2.0,
                                               11 + D)
    out = ops.paged_attention_prefill(q, kc, vc, bt, cl, ql, 0.5, 2.0)
    _check(out, ref)
    assert (out[1, 23:] == 0).all()
    assert (out[2] == 0).all()
    assert (out[1, :23] != 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("k_scale,v_scale", SCALES)
@pytest.mark.parametrize("D,Hq,Hkv", [(64, 4, 2), (128, 8, 1)])
def test_fp8_prefill_single_row_matches_decode_kernel(D, Hq, Hkv, k_scale,
                                                      v_scale):
    specs = ((0, 1), (15, 1), (16, 1), (100, 1))
    q, kc, vc, bt, cl, ql, ref = _prefill_case(D, Hq, Hkv, specs, 1, k_scale,
                                               v_scale, 5 + D)
    out = ops.paged_attention_prefill(q, kc, vc, bt, cl, ql, k_scale, v_scale)
    _check(out, ref)
    dec = ops.paged_attention_decode(q[:, 0].contiguous(), kc, vc, bt,
                                     cl + 1, num_splits=1, k_scale=k_scale,
                                     v_scale=v_scale)
    d = float((out[:, 0].float() - dec.float()).abs().max())
    print(f"prefill vs decode kernel: max abs diff {d:.3e}")
    assert torch.allclose(out[:, 0].float(), dec.float(), atol=2e-2, rtol=0)


# --------------------------------------------------------------------------
# GPU: append kernels, bit-exact
# --------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 0.5, 3.0])
@pytest.mark.parametrize("D", [64, 128])
def test_fp8_rope_append_kernel_bits(D, scale):
    """The fp8 kernel stores exactly quantize_kv_fp8 (computed on the
    CPU) of what the bf16 kernel stores from the same inputs."""
    dev = _dev()
    g = torch.Generator().manual_seed(D)
    B, Hq, Hkv, P = 4, 8, 2, 16
    # row 1 is scaled up so that part of it lands in the clamp at every
    # scale (|x| > 448 * scale); the other rows cover the ordinary range
    fused = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g) * 4
    fused[1] *= 150
    fused = fused.bfloat16().to(dev)
    qf, kf, vf = fused.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    q, k, v = (qf.view(B, Hq, D), kf.view(B, Hkv, D), vf.view(B, Hkv, D))
    assert not k.is_contiguous()
    cosT, sinT = ops.rope_tables(64, D, device=dev)
    pos_l = [0, 17, 31, -1]
    pos = torch.tensor(pos_l, dtype=torch.int32, device=dev)
    bt = torch.tensor([[3, 9], [5, 2], [7, 11], [13, 14]],
                      dtype=torch.int32, device=dev)
    kb = torch.zeros(P, Hkv, PAGE, D, dtype=torch.bfloat16, device=dev)
    vb = torch.zeros_like(kb)
    kc = _fp8_full((P, Hkv, PAGE, D), SENTINEL, dev)
    vc = _fp8_full((P, Hkv, PAGE, D), SENTINEL, dev)
    q_bf = ops.rope_append_paged(q, k, v, cosT, sinT, pos, bt, kb, vb)
    q_f8 = ops.rope_append_paged(q, k, v, cosT, sinT, pos, bt, kc, vc,
                                 scale, scale)
    torch.cuda.synchronize()
    assert torch.equal(q_f8.view(torch.int16), q_bf.view(torch.int16))
    kb, vb, kc, vc, btc = (t.cpu() for t in (kb, vb, kc, vc, bt))
    written = torch.zeros(P, PAGE, dtype=torch.bool)
    saturated = 0
    for b, p in enumerate(pos_l):
        if p < 0:
            continue
        pg, slt = int(btc[b, p // PAGE]), p % PAGE
        written[pg, slt] = True
        for name, c8, cb in (("k", kc, kb), ("v", vc, vb)):
            want = _bytes(ops.quantize_kv_fp8(cb[pg, :, slt], scale))
            got = _bytes(c8[pg, :, slt])
            bad = int((got != want).sum())
            print(f"{name} row {b}: {bad} of {want.numel()} bytes differ")
            assert bad == 0
            saturated += int(((want & 0x7F) == 0x7E).sum())
    assert saturated > 0  # the clamp was exercised
    for cache in (kc, vc):
        assert (_bytes(cache).permute(0, 2, 1, 3)[~written] == SENTINEL).all()
    assert int(written.sum()) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("pos0", [0, 5, 16])
@pytest.mark.parametrize("T", [1, 16, 37])
def test_fp8_kv_append_kernel_bits(T, pos0):
    dev = _dev()
    g = torch.Generator().manual_seed(100 * T + pos0)
    Hkv, D, P = 2, 128, 9
    k, v = _append_case(g, T, Hkv, D)
    k[0] *= 100  # into the clamp
    row = [7, 3, 8, 1]
    kc = _fp8_full((P, Hkv, PAGE, D), SENTINEL, dev)
    vc = _fp8_full((P, Hkv, PAGE, D), SENTINEL, dev)
    ops.kv_append_paged(k.to(dev), v.to(dev), pos0,
                        torch.tensor(row, dtype=torch.int32, device=dev),
                        kc, vc, 0.5, 3.0)
    ke, ve = _append_expected(k, v, pos0, row, P, 0.5, 3.0)
    assert torch.equal(_bytes(kc).cpu(), _bytes(ke))
    assert torch.equal(_bytes(vc).cpu(), _bytes(ve))


@pytest.mark.gpu
def test_kv_append_kernel_table_and_pool_guards_and_bf16():
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    k, v = _append_case(g, 40, 2, 64)
    row = [2, 9, 1]  # page id 9 is outside the pool; rows 48.. have no entry
    btr = torch.tensor(row, dtype=torch.int32, device=dev)
    kc = _fp8_full((4, 2, PAGE, 64), SENTINEL, dev)
    vc = _fp8_full((4, 2, PAGE, 64), SENTINEL, dev)
    ops.kv_append_paged(k.to(dev), v.to(dev), 10, btr, kc, vc)
    ke, ve = _append_expected(k, v, 10, row, 4, 1.0, 1.0)
    assert torch.equal(_bytes(kc).cpu(), _bytes(ke))
    assert torch.equal(_bytes(vc).cpu(), _bytes(ve))
    # bf16 caches: a plain copy, as the reference does it
    kb = torch.zeros(4, 2, PAGE, 64, dtype=torch.bfloat16, device=dev)
    vb = torch.zeros_like(kb)
    ops.kv_append_paged(k.to(dev), v.to(dev), 10, btr, kb, vb)
    kr = torch.zeros(4, 2, PAGE, 64, dtype=torch.bfloat16)
    vr = torch.zeros_like(kr)
    ops.kv_append_paged_ref(k, v, 10, torch.tensor(row, dtype=torch.int32),
                            kr, vr)
    assert torch.equal(kb.cpu(), kr) and torch.equal(vb.cpu(), vr)


@pytest.mark.gpu
def test_fp8_bindings_reject_bad_inputs():
    q, kc, vc, bt, sl, _ = _decode_case(64, 4, 2, (1, 15, 16, 17, 0), 64,
                                        1.0, 1.0, 70)
    dev = q.device
    dec = functools.partial(ops.paged_attention_decode, q, num_splits=1)
    dec(kc, vc, bt, sl)  # the good call
    kb = torch.zeros(kc.shape, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError):  # mixed k/v dtypes
        dec(kc, kb, bt, sl)
    with pytest.raises(RuntimeError):
        dec(kb, vc, bt, sl)
    for dt in (torch.float8_e4m3fnuz, torch.float8_e5m2):
        other = torch.zeros(kc.shape, dtype=torch.uint8, device=dev).view(dt)
        with pytest.raises(RuntimeError):
            dec(other, other.clone(), bt, sl)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError):
            dec(kc, vc, bt, sl, k_scale=bad)
        with pytest.raises(RuntimeError):
            dec(kc, vc, bt, sl, v_scale=bad)
    with pytest.raises(RuntimeError):  # scales mean nothing to bf16 caches
        dec(kb, kb.clone(), bt, sl, k_scale=0.5)
    with pytest.raises(RuntimeError):
        dec(kb, kb.clone(), bt, sl, v_scale=2.0)
    # the same checks guard the other entry points
    q4 = q[:1].view(1, 1, 4, 64)
    one = torch.ones(1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError):
        ops.paged_attention_prefill(q4, kc, kb, bt[:1], one, one)
    with pytest.raises(RuntimeError):
        ops.paged_attention_prefill(q4, kc, vc, bt[:1], one, one, 0.0, 1.0)
    kv = torch.zeros(3, 2, 64, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError):
        ops.kv_append_paged(kv, kv, 0, bt[0], kc, vc, 1.0, -1.0)
    with pytest.raises(RuntimeError):
        ops.kv_append_paged(kv, kv, 0, bt[0], kb, kb.clone(), 0.5, 1.0)
    with pytest.raises(RuntimeError):  # misaligned fp8 cache
        flat = torch.zeros(kc.numel() + 8, dtype=torch.uint8, device=dev)
        off = flat[4 : 4 + kc.numel()].view(FP8).view(kc.shape)
        dec(off, off.clone(), bt, sl)


# --------------------------------------------------------------------------
# GPU: decoder and engine
# --------------------------------------------------------------------------


class _QuantisedKVCache:
    """Dense per-sequence cache whose rows go through the fp8 storage
    rule: update() stores dequantise(quantize_kv_fp8(k)) and returns the
    stored rows, so the dense reference attends to the values the fp8
    pages hold."""

    def __init__(self, max_T, n_kv, hd, device, dtype, k_scale, v_scale):
        self.k = torch.zeros(1, n_kv, max_T, hd, device=device, dtype=dtype)
        self.v = torch.zeros_like(self.k)
        self.k_scale, self.v_scale = k_scale, v_scale
        self.len = 0

    def _round_trip(self, x, scale):
        return (ops.quantize_kv_fp8(x, scale).float() * scale).to(x.dtype)

    def update(self, k, v, pos0):
        T = k.size(2)
        self.k[:, :, pos0 : pos0 + T] = self._round_trip(k, self.k_scale)
        self.v[:, :, pos0 : pos0 + T] = self._round_trip(v, self.v_scale)
        self.len = pos0 + T
        return self.k[:, :, : self.len], self.v[:, :, : self.len]


@pytest.mark.gpu
def test_fp8_paged_decoder_gpu_logits():
    """Teacher-forced fp8 PagedDecoder logits, eager and replayed from a
    captured graph and after a slot is recycled, against the dense
    per-sequence path over the same quantised K/V. Also printed, not
    asserted: rel against the unquantised bf16 reference, which is the
    accuracy cost of fp8 (on the MI355X: 0.0076 against the quantised
    reference, 0.031 against the unquantised one)."""
    from ray_amd.models.llama import KVCache

    dev = _dev()
    cfg = CONFIGS["llama-tiny"]
    m = _tiny(dev, torch.bfloat16)
    hd = cfg.hidden_size // cfg.num_heads
    ks, vs = 1.0, 1.0

    prompts = [list(range(5, 15)), list(range(50, 58)),
               list(range(200, 221))]
    forced = [list(range(300, 308)), list(range(400, 408)),
              list(range(330, 338))]

    def reference(p, f, quantised):
        caches = [
            _QuantisedKVCache(96, cfg.num_kv_heads, hd, dev, torch.bfloat16,
                              ks, vs) if quantised else
            KVCache(1, 96, cfg.num_kv_heads, hd, dev, torch.bfloat16)
            for _ in range(cfg.num_layers)]
        m(torch.tensor([p], device=dev), kv_caches=caches, pos0=0)
        out, pos = [], len(p)
        for t in f:
            lg = m(torch.tensor([[t]], device=dev), kv_caches=caches,
                   pos0=pos)[:, -1]
            out.append(lg[0].float())
            pos += 1
        return out

    def run(pd, slot_prompts, slot_forced):
        for slot in range(2):
            pd.prefill_slot(slot, torch.tensor(slot_prompts[slot],
                                               device=dev),
                            reserve_tokens=len(slot_prompts[slot]) + 9)
        pos = torch.tensor([len(p) for p in slot_prompts], device=dev)
        steps = []
        for step in range(8):
            for slot in range(2):
                pd.set_slot_len(slot, int(pos[slot]) + 1)
            toks = torch.tensor([f[step] for f in slot_forced], device=dev)
            steps.append(pd.decode(toks, pos).float().clone())
            pos += 1
        return steps

    def new_decoder():
        pd = PagedDecoder(m, 2, 96, dev, num_pages=9, kv_dtype=FP8,
                          k_scale=ks, v_scale=vs)
        for t in pd.pool.k + pd.pool.v:  # unallocated memory is poison
            _bytes(t).fill_(NAN_BYTE)
        return pd

    with torch.no_grad():
        refs = [reference(p, f, True) for p, f in zip(prompts, forced)]
        plain = [reference(p, f, False) for p, f in zip(prompts, forced)]

        eager = new_decoder()
        lg_e = run(eager, prompts[:2], forced[:2])
        graphed = new_decoder()
        graphed.capture()
        assert graphed.graph is not None
        lg_g = run(graphed, prompts[:2], forced[:2])
        worst = worst_plain = 0.0
        for step in range(8):
            for slot in range(2):
                assert torch.isfinite(lg_e[step][slot]).all()
                assert torch.isfinite(lg_g[step][slot]).all()
                worst = max(worst, _rel(lg_e[step][slot], refs[slot][step]),
                            _rel(lg_g[step][slot], refs[slot][step]))
                worst_plain = max(worst_plain,
                                  _rel(lg_g[step][slot], plain[slot][step]))
        print(f"fp8 pool vs quantised dense reference: max rel {worst:.4f}")
        print(f"fp8 pool vs unquantised bf16 reference: max rel "
              f"{worst_plain:.4f}")
        for step in range(8):
            for slot in range(2):
                ref = refs[slot][step]
                assert _rel(lg_e[step][slot], ref) < 0.05, (slot, step)
                assert _rel(lg_g[step][slot], ref) < 0.05, (slot, step)
                assert _rel(lg_g[step][slot], lg_e[step][slot]) < 0.05

        # recycle slot 0: the 21-token prompt gets stale pages back
        stale = list(graphed._slot_pages[0])
        graphed.release_slot(0)
        assert graphed.pool.num_free == 6
        lg_r = run(graphed, [prompts[2], prompts[1]], [forced[2], forced[1]])
        assert set(graphed._slot_pages[0]) & set(stale)
        for step in range(8):
            assert _rel(lg_r[step][0], refs[2][step]) < 0.05, step
            assert _rel(lg_r[step][1], refs[1][step]) < 0.05, step
        graphed.release_slot(0)
        graphed.release_slot(1)
        assert graphed.pool.num_free == graphed.pool.num_usable


@pytest.mark.gpu
def test_fp8_engine_gpu_captured_prefix_caching():
    prompts = _engine_prompts()

    def run():
        eng = ContinuousBatchingEngine(LLMConfig(
            model_id="llama-tiny", max_seq_len=96, max_batch_size=2,
            kv_cache="paged", kv_cache_dtype="fp8",
            enable_prefix_caching=True))
        assert eng.decoder.graph is not None
        assert eng.decoder.pool.k[0].dtype == FP8
        ids = [eng.submit(p, max_new_tokens=n)
               for p, n in zip(prompts, [8, 14, 6])]
        out = eng.run_until_complete()
        assert eng.stats["kv_pages_free"] == eng.stats["kv_pages_total"] == 12
        assert eng.stats["prefix_hit_tokens"] == 32
        return [out[i] for i in ids]

    a, b = run(), run()
    assert [len(r) for r in a] == [8, 14, 6]
    assert all(0 <= t < 512 for r in a for t in r)
    assert a == b
