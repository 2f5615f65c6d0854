"""Prefix caching and chunked prefill over the paged KV cache: the
pool's reference counts, prefix index and eviction, PagedDecoder's
chunked / prefix-hit prefill against whole-prompt prefill, and the
engine flags. CPU in fp32; the decoder again on GPU in bf16."""
import pytest
import torch

from ray_amd.llm import ContinuousBatchingEngine, LLMConfig
from ray_amd.llm.paged import PagedDecoder, PagedKVPool
from ray_amd.models.llama import CONFIGS, KVCache, LlamaModel

PAGE = 16


def _pool(num_pages):
    return PagedKVPool(1, num_pages, 1, 64, torch.device("cpu"),
                       torch.float32)


# --------------------------------------------------------------------------
# pool
# --------------------------------------------------------------------------


def test_pool_share_and_free_count():
    pool = _pool(6)
    a = pool.alloc(2)
    pool.share(a)
    pool.share(a[:1])
    pool.free(a)            # counts 2, 1
    assert pool.num_free == 3
    pool.free(a)            # counts 1, 0
    assert pool.num_free == 4
    pool.free(a[:1])
    assert pool.num_free == 5
    with pytest.raises(ValueError):  # already at count 0
        pool.free(a[:1])
    with pytest.raises(ValueError):
        pool.share(a)
    with pytest.raises(ValueError):
        pool.share([0])
    b = pool.alloc(1)
    with pytest.raises(ValueError):  # listed twice
        pool.free(b + b)
    assert pool.num_free == 4


def test_pool_order_unchanged_without_prefixes():
    """Nothing registered: low page numbers first, freed pages reused
    last-freed-first, exactly the plain free list."""
    pool = _pool(8)
    assert pool.alloc(3) == [1, 2, 3]
    b = pool.alloc(2)
    assert b == [4, 5]
    pool.free([2, 3])
    assert pool.alloc(3) == [3, 2, 6]
    assert pool.num_cached == 0
    assert pool.match_prefix(list(range(64)), 4) == []


def test_pool_match_prefix_longest_chain_and_cap():
    pool = _pool(10)
    toks = list(range(100, 100 + 3 * PAGE + 5))   # 3 full pages + 5
    pages = pool.alloc(4)
    pool.register_prefix(toks, pages[:3])
    assert pool.num_cached == 3
    # whole chain, the cap, and a reference per returned page
    assert pool.match_prefix(toks, 8) == pages[:3]
    assert pool.match_prefix(toks, 2) == pages[:2]
    assert pool.match_prefix(toks[: 2 * PAGE], 8) == pages[:2]
    assert pool.match_prefix(toks[: 2 * PAGE - 1], 8) == pages[:1]
    # a prompt that differs inside the second page matches one page
    other = list(toks)
    other[PAGE + 3] += 1
    assert pool.match_prefix(other, 8) == pages[:1]
    # the same 16 tokens under another parent do not match
    assert pool.match_prefix(toks[PAGE:], 8) == []
    # counts: page0 1+5, page1 1+3, page2 1+1
    for p, extra in zip(pages[:3], (5, 3, 1)):
        for _ in range(extra):
            pool.free([p])
    assert pool.num_free == 10 - 1 - 4
    # registering the same tokens from other pages keeps the first pages
    dup = pool.alloc(3)
    pool.register_prefix(toks, dup)
    assert pool.num_cached == 3
    pool.free(dup)
    assert pool.match_prefix(toks, 8) == pages[:3]


def test_pool_eviction_lru_tail_first_and_only_when_free_list_empty():
    pool = _pool(7)                      # 6 usable
    toks = list(range(3 * PAGE))
    chain = pool.alloc(3)
    pool.register_prefix(toks, chain)
    pool.free(chain[::-1])               # deepest first, as release_slot
    assert pool.num_cached == 3
    assert pool.num_free == 6            # evictable pages count as free
    # three plain free pages go first; the chain survives
    a = pool.alloc(3)
    assert not set(a) & set(chain)
    assert pool.num_cached == 3
    # the free list is empty: the deepest cached page is evicted
    b = pool.alloc(1)
    assert b == [chain[2]] and pool.num_cached == 2
    got = pool.match_prefix(toks, 8)
    assert got == chain[:2]              # its index entry is gone
    pool.free(got[::-1])
    c = pool.alloc(2)
    assert c == [chain[1], chain[0]] and pool.num_cached == 0
    assert pool.alloc(1) is None
    assert pool.match_prefix(toks, 8) == []
    pool.free(a + b + c)
    assert pool.num_free == 6


def test_pool_matched_page_leaves_the_lru():
    pool = _pool(4)                      # 3 usable
    toks = list(range(PAGE))
    p = pool.alloc(1)
    pool.register_prefix(toks, p)
    pool.free(p)
    assert pool.num_free == 3
    assert pool.match_prefix(toks, 1) == p   # back in use
    assert pool.num_free == 2
    rest = pool.alloc(2)
    assert p[0] not in rest and pool.alloc(1) is None
    assert pool.num_cached == 1


# --------------------------------------------------------------------------
# decoder, CPU fp32
# --------------------------------------------------------------------------


def _tiny(dev, dtype):
    cfg = CONFIGS["llama-tiny"]
    torch.manual_seed(0)
    m = LlamaModel(cfg, dtype=dtype).to(dev).eval()
    m.cosT = m.cosT.to(dev)
    m.sinT = m.sinT.to(dev)
    return m


_CPU = {}


def _cpu_model_and_whole_prompt_logits():
    """llama-tiny in fp32 and the whole-prompt prefill logits of the
    37-token prompt, computed once."""
    if not _CPU:
        m = _tiny(torch.device("cpu"), torch.float32)
        prompt = torch.arange(3, 40) * 7 % 512
        with torch.no_grad():
            pd = PagedDecoder(m, 1, 96, torch.device("cpu"))
            _CPU.update(m=m, prompt=prompt,
                        logits=pd.prefill_slot(0, prompt).clone())
    return _CPU["m"], _CPU["prompt"], _CPU["logits"]


def _rel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-6))


@pytest.mark.parametrize("chunk", [1, 7, 16, 40])
def test_chunked_prefill_matches_whole_prompt_cpu(chunk):
    m, prompt, want = _cpu_model_and_whole_prompt_logits()
    assert prompt.numel() == 37
    pd = PagedDecoder(m, 1, 96, torch.device("cpu"), prefill_chunk=chunk)
    with torch.no_grad():
        got = pd.prefill_slot(0, prompt)
    r = _rel(got, want)
    print(f"chunk {chunk}: rel L2 {r:.3e}")
    assert r < 1e-4
    assert int(pd.seq_lens[0]) == 37
    assert pd.prefill_tokens_computed == 37 and pd.prefix_hit_tokens == 0
    assert pd.pool.num_cached == 0
    pd.release_slot(0)
    assert pd.pool.num_free == pd.pool.num_usable


def test_prefix_hit_prefill_matches_cold_cpu():
    m, prompt, want = _cpu_model_and_whole_prompt_logits()
    pd = PagedDecoder(m, 2, 96, torch.device("cpu"), prefix_caching=True)
    with torch.no_grad():
        cold = pd.prefill_slot(0, prompt)
        assert pd.prefix_hit_tokens == 0
        shared = pd._slot_pages[0][:2]
        before = [(pd.pool.k[li][shared].clone(), pd.pool.v[li][shared].clone())
                  for li in range(len(pd.pool.k))]
        warm = pd.prefill_slot(1, prompt)
    assert pd.prefix_hit_tokens == 32 and pd.prefill_tokens_computed == 37 + 5
    assert pd._slot_pages[1][:2] == shared        # the pages are shared
    assert pd._slot_pages[1][2] != pd._slot_pages[0][2]
    for li, (k0, v0) in enumerate(before):        # and were only read
        assert torch.equal(pd.pool.k[li][shared], k0)
        assert torch.equal(pd.pool.v[li][shared], v0)
    for name, got in (("cold", cold), ("warm", warm)):
        r = _rel(got, want)
        print(f"{name}: rel L2 {r:.3e}")
        assert r < 1e-4
    # releasing one owner keeps the pages for the other
    pd.release_slot(0)
    assert pd.pool.num_free == pd.pool.num_usable - 6
    pd.release_slot(1)
    assert pd.pool.num_free == pd.pool.num_usable
    assert pd.pool.num_cached == 2


def test_prefix_hit_with_chunks_and_failed_alloc_cpu():
    m, prompt, want = _cpu_model_and_whole_prompt_logits()
    dev = torch.device("cpu")
    pd = PagedDecoder(m, 2, 96, dev, num_pages=8, prefix_caching=True,
                      prefill_chunk=3)               # 7 usable pages
    with torch.no_grad():
        pd.prefill_slot(0, prompt, reserve_tokens=48)   # 3 pages
        warm = pd.prefill_slot(1, prompt, reserve_tokens=48)  # 2 shared + 1
        assert _rel(warm, want) < 1e-4
        pd.release_slot(1)
        assert pd.pool.num_free == 4
        # 6 pages for 96 tokens: 2 shared + the 4 that are free
        pd.prefill_slot(1, prompt, reserve_tokens=96)
        assert pd.pool.num_free == 0
        pd.release_slot(1)
        # a request that cannot fit drops the references it took
        big = PagedDecoder(m, 2, 96, dev, num_pages=5, prefix_caching=True)
        big.prefill_slot(0, prompt, reserve_tokens=48)  # 3 of 4 pages
        with pytest.raises(RuntimeError):
            big.prefill_slot(1, prompt, reserve_tokens=64)  # 2 shared + 2
        assert big.pool.num_free == 1
        big.release_slot(0)
        assert big.pool.num_free == 4


# --------------------------------------------------------------------------
# engine, CPU
# --------------------------------------------------------------------------


def _engine_prompts():
    prefix = [(11 * i + 5) % 512 for i in range(40)]
    return [
        prefix + [300, 301, 302],
        prefix + [310 + i for i in range(9)],
        prefix + [17],
        prefix + [300, 301, 302],      # identical to the first
        prefix[:32],                   # exactly two pages, both cached
    ]


def test_engine_prefix_caching_same_outputs_and_stats_cpu():
    prompts = _engine_prompts()
    budgets = [6, 5, 7, 6, 4]
    results = {}
    for on in (False, True):
        eng = ContinuousBatchingEngine(LLMConfig(
            model_id="llama-tiny", max_seq_len=96, max_batch_size=2,
            use_hip_graph=False, kv_cache="paged",
            enable_prefix_caching=on))
        ids = [eng.submit(p, max_new_tokens=n)
               for p, n in zip(prompts, budgets)]
        out = eng.run_until_complete()
        results[on] = [out[i] for i in ids]
        st = eng.stats
        assert st["kv_pages_free"] == st["kv_pages_total"] == 12
        total = sum(len(p) for p in prompts)
        if on:
            # two slots: requests 0 and 1 prefill cold one after the
            # other, so 1 already hits 0's two pages; 2 and 3 hit two
            # pages; the 32-token prompt may reuse (32-1)//16 = 1 page
            assert st["prefix_hit_tokens"] == 32 + 32 + 32 + 16
            assert st["kv_pages_cached"] >= 2
        else:
            assert st["prefix_hit_tokens"] == 0
            assert st["kv_pages_cached"] == 0
        assert (st["prefill_tokens_computed"]
                == total - st["prefix_hit_tokens"])
    assert results[True] == results[False]
    assert results[True][0] == results[True][3]
    assert [len(r) for r in results[True]] == budgets


def test_engine_shared_page_bits_unchanged_by_second_request_cpu():
    prompts = _engine_prompts()
    eng = ContinuousBatchingEngine(LLMConfig(
        model_id="llama-tiny", max_seq_len=96, max_batch_size=2,
        use_hip_graph=False, kv_cache="paged", enable_prefix_caching=True))
    eng.submit(prompts[0], max_new_tokens=8)
    eng.step()
    pool = eng.decoder.pool
    shared = list(eng.decoder._slot_pages[0][:2])
    before = [(k[shared].clone(), v[shared].clone())
              for k, v in zip(pool.k, pool.v)]
    eng.submit(prompts[1], max_new_tokens=8)
    eng.step()
    assert eng.decoder._slot_pages[1][:2] == shared
    assert eng.stats["prefix_hit_tokens"] == 32
    eng.run_until_complete()
    for (k0, v0), k, v in zip(before, pool.k, pool.v):
        assert torch.equal(k[shared], k0) and torch.equal(v[shared], v0)
    assert eng.stats["kv_pages_free"] == eng.stats["kv_pages_total"]


def test_engine_chunked_prefill_same_outputs_cpu():
    prompts = _engine_prompts()[:2]
    results = {}
    for chunk in (None, 16):
        eng = ContinuousBatchingEngine(LLMConfig(
            model_id="llama-tiny", max_seq_len=96, max_batch_size=2,
            use_hip_graph=False, kv_cache="paged",
            prefill_chunk_tokens=chunk))
        ids = [eng.submit(p, max_new_tokens=5) for p in prompts]
        out = eng.run_until_complete()
        results[chunk] = [out[i] for i in ids]
        assert eng.stats["kv_pages_cached"] == 0
    assert results[16] == results[None]


def test_engine_flags_need_paged_cache():
    with pytest.raises(ValueError):
        ContinuousBatchingEngine(LLMConfig(
            model_id="llama-tiny", enable_prefix_caching=True))
    with pytest.raises(ValueError):
        ContinuousBatchingEngine(LLMConfig(
            model_id="llama-tiny", kv_cache="contiguous",
            prefill_chunk_tokens=16))


# --------------------------------------------------------------------------
# decoder, GPU bf16: the HIP prefill kernel inside the model
# --------------------------------------------------------------------------


@pytest.mark.gpu
def test_paged_decoder_gpu_chunked_and_prefix_hit_logits():
    """Teacher-forced decode logits after a chunked prefill and after a
    prefix-hit prefill match the per-sequence KVCache path (relative L2
    < 0.05, the bound of test_paged_decoder_gpu_logits), eagerly and
    replayed from a captured graph."""
    dev = torch.device("cuda:0")
    m = _tiny(dev, torch.bfloat16)
    cfg = m.cfg
    hd = cfg.hidden_size // cfg.num_heads
    prompt = list(range(200, 221))           # 21 tokens
    sibling = prompt[:16] + list(range(90, 97))   # same first page
    forced = list(range(300, 306))

    def reference(p):
        caches = [KVCache(1, 96, cfg.num_kv_heads, hd, dev, torch.bfloat16)
                  for _ in range(cfg.num_layers)]
        first = m(torch.tensor([p], device=dev), kv_caches=caches,
                  pos0=0)[0, -1].float()
        out, pos = [first], len(p)
        for t in forced:
            out.append(m(torch.tensor([[t]], device=dev), kv_caches=caches,
                         pos0=pos)[0, -1].float())
            pos += 1
        return out

    def run(pd, slot, p):
        """Prefill logits, then the forced steps' logits of one slot.
        The other slot keeps its pages but sits out (length 0), so the
        decode step appends nothing to it."""
        pd.set_slot_len(1 - slot, 0)
        out = [pd.prefill_slot(slot, torch.tensor(p, device=dev),
                               reserve_tokens=len(p) + 8).float().clone()]
        pos = torch.zeros(pd.B, dtype=torch.long, device=dev)
        pos[slot] = len(p)
        for t in forced:
            pd.set_slot_len(slot, int(pos[slot]) + 1)
            toks = torch.full((pd.B,), t, device=dev)
            out.append(pd.decode(toks, pos)[slot].float().clone())
            pos[slot] += 1
        return out

    def check(got, want, what):
        for step, (a, b) in enumerate(zip(got, want)):
            r = _rel(a, b)
            print(f"{what} step {step}: rel L2 {r:.3e}")
            assert r < 0.05, (what, step, r)

    with torch.no_grad():
        ref_p, ref_s = reference(prompt), reference(sibling)

        chunked = PagedDecoder(m, 2, 96, dev, prefill_chunk=16)
        check(run(chunked, 0, prompt), ref_p, "chunked")

        cached = PagedDecoder(m, 2, 96, dev, prefix_caching=True)
        check(run(cached, 0, prompt), ref_p, "cold")
        assert cached.prefix_hit_tokens == 0
        check(run(cached, 1, sibling), ref_s, "prefix hit")
        assert cached.prefix_hit_tokens == 16
        assert cached._slot_pages[1][0] == cached._slot_pages[0][0]

        graphed = PagedDecoder(m, 2, 96, dev, prefix_caching=True,
                               prefill_chunk=16)
        graphed.capture()
        assert graphed.graph is not None
        check(run(graphed, 0, prompt), ref_p, "graph cold")
        check(run(graphed, 1, sibling), ref_s, "graph prefix hit")
        assert graphed.prefix_hit_tokens == 16
        for slot in (0, 1):
            graphed.release_slot(slot)
        assert graphed.pool.num_free == graphed.pool.num_usable
