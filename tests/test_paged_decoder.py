"""Paged KV cache through the decoder and the continuous-batching
engine. CPU: engine equivalence and pool-limited admission; GPU:
PagedDecoder logits (eager and graph replay) against the per-sequence
KVCache path."""
import pytest
import torch

from ray_amd.llm import ContinuousBatchingEngine, LLMConfig


def test_paged_engine_matches_contiguous_cpu():
    prompts = [
        list(range(5, 17)),          # 12 tokens
        list(range(100, 104)),       # 4 tokens
        list(range(40, 61)),         # 21 tokens
    ]
    budgets = [8, 14, 6]
    results = {}
    for kind in ("contiguous", "paged"):
        eng = ContinuousBatchingEngine(LLMConfig(
            model_id="llama-tiny", max_seq_len=96, max_batch_size=2,
            use_hip_graph=False, kv_cache=kind))  # same seed, same weights
        ids = [eng.submit(p, max_new_tokens=n)
               for p, n in zip(prompts, budgets)]
        out = eng.run_until_complete()
        results[kind] = [out[i] for i in ids]
        if kind == "paged":
            assert eng.stats["kv_pages_total"] == 2 * 6
            assert eng.stats["kv_pages_free"] == eng.stats["kv_pages_total"]
            assert eng.stats["requests"] == 3
        else:
            assert "kv_pages_total" not in eng.stats
    assert results["paged"] == results["contiguous"]
    assert [len(r) for r in results["paged"]] == budgets


def test_paged_engine_small_pool_trades_length_for_concurrency_cpu():
    """13 pages (12 usable) cannot hold 4 full-length sequences of 96
    tokens (6 pages each; a contiguous cache of the same bytes holds
    13*16 // 96 = 2 slots), yet four short requests run at once."""
    eng = ContinuousBatchingEngine(LLMConfig(
        model_id="llama-tiny", max_seq_len=96, max_batch_size=4,
        use_hip_graph=False, kv_cache="paged", kv_num_pages=13))
    assert (13 * 16) // 96 == 2
    assert eng.stats["kv_pages_total"] == 12
    ids = [eng.submit(list(range(10 + i, 15 + i)), max_new_tokens=6)
           for i in range(6)]
    results, peak = {}, 0
    while eng.has_work():
        for f in eng.step():
            results[f["id"]] = f["token_ids"]
        peak = max(peak, sum(s is not None for s in eng._slots))
        assert eng.stats["kv_pages_free"] == 12 - sum(
            s is not None for s in eng._slots)  # one page per short request
    assert set(results) == set(ids)
    assert all(len(results[i]) == 6 for i in ids)
    assert peak == 4
    assert eng.stats["kv_pages_free"] == 12


def test_paged_engine_admission_waits_for_pages_in_order_cpu():
    """A request whose pages are not free stays queued and the ones
    behind it do not overtake it."""
    eng = ContinuousBatchingEngine(LLMConfig(
        model_id="llama-tiny", max_seq_len=96, max_batch_size=3,
        use_hip_graph=False, kv_cache="paged", kv_num_pages=8))  # 7 usable
    a = eng.submit(list(range(60)), max_new_tokens=4)   # 64 tok: 4 pages
    b = eng.submit(list(range(60)), max_new_tokens=4)   # 4 pages: must wait
    c = eng.submit(list(range(5)), max_new_tokens=4)    # 1 page, behind b
    eng.step()
    active = [s["id"] for s in eng._slots if s is not None]
    assert active == [a]
    assert [r["id"] for r in eng._queue] == [b, c]
    out = eng.run_until_complete()
    assert set(out) == {a, b, c}
    assert eng.stats["kv_pages_free"] == 7


def test_paged_engine_rejects_request_that_can_never_fit_cpu():
    eng = ContinuousBatchingEngine(LLMConfig(
        model_id="llama-tiny", max_seq_len=512, max_batch_size=2,
        use_hip_graph=False, kv_cache="paged", kv_num_pages=13))
    eng.submit(list(range(100)), max_new_tokens=92)      # 192 tok: 12 pages
    with pytest.raises(ValueError):
        eng.submit(list(range(100)), max_new_tokens=93)  # 193 tok: 13 pages
    with pytest.raises(ValueError):
        ContinuousBatchingEngine(LLMConfig(model_id="llama-tiny",
                                           kv_cache="bogus"))


@pytest.mark.gpu
def test_paged_engine_gpu_captured_runs_and_frees_pages():
    """The engine's paged path on the GPU: captured decoder, queueing
    through 2 slots, deterministic greedy output, pages all returned."""
    def run():
        eng = ContinuousBatchingEngine(LLMConfig(
            model_id="llama-tiny", max_seq_len=96, max_batch_size=2,
            kv_cache="paged"))
        assert eng.decoder.graph is not None
        ids = [eng.submit(list(range(5 + i, 12 + 3 * i)), max_new_tokens=n)
               for i, n in enumerate([8, 14, 6])]
        out = eng.run_until_complete()
        assert eng.stats["kv_pages_free"] == eng.stats["kv_pages_total"] == 12
        return [out[i] for i in ids]

    a, b = run(), run()
    assert [len(r) for r in a] == [8, 14, 6]
    assert all(0 <= t < 512 for r in a for t in r)
    assert a == b


@pytest.mark.gpu
def test_paged_decoder_gpu_logits():
    """Teacher-forced PagedDecoder logits, eager and replayed from a
    captured graph, match the per-sequence KVCache path; so do they
    after a slot is released and reused for another prompt (stale data
    in the recycled pages)."""
    from ray_amd.llm.paged import PagedDecoder
    from ray_amd.models.llama import CONFIGS, KVCache, LlamaModel

    dev = torch.device("cuda:0")
    cfg = CONFIGS["llama-tiny"]
    torch.manual_seed(0)
    m = LlamaModel(cfg, dtype=torch.bfloat16).to(dev).eval()
    m.cosT = m.cosT.to(dev)
    m.sinT = m.sinT.to(dev)
    hd = cfg.hidden_size // cfg.num_heads

    prompts = [list(range(5, 15)), list(range(50, 58)),
               list(range(200, 221))]
    forced = [list(range(300, 308)), list(range(400, 408)),
              list(range(330, 338))]

    def reference(p, f):
        caches = [KVCache(1, 96, cfg.num_kv_heads, hd, dev, torch.bfloat16)
                  for _ in range(cfg.num_layers)]
        m(torch.tensor([p], device=dev), kv_caches=caches, pos0=0)
        out, pos = [], len(p)
        for t in f:
            lg = m(torch.tensor([[t]], device=dev), kv_caches=caches,
                   pos0=pos)[:, -1]
            out.append(lg[0].float())
            pos += 1
        return out

    def rel(a, b):
        return float((a - b).norm() / (b.norm() + 1e-6))

    def run(pd, slot_prompts, slot_forced, prefill):
        """8 forced steps; returns logits[step][slot]."""
        for slot in prefill:
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

    with torch.no_grad():
        refs = [reference(p, f) for p, f in zip(prompts, forced)]

        eager = PagedDecoder(m, 2, 96, dev, num_pages=9)
        lg_e = run(eager, prompts[:2], forced[:2], prefill=[0, 1])
        graphed = PagedDecoder(m, 2, 96, dev, num_pages=9)
        graphed.capture()
        assert graphed.graph is not None
        lg_g = run(graphed, prompts[:2], forced[:2], prefill=[0, 1])
        for step in range(8):
            for slot in range(2):
                ref = refs[slot][step]
                assert rel(lg_e[step][slot], ref) < 0.05, (slot, step)
                assert rel(lg_g[step][slot], ref) < 0.05, (slot, step)
                assert rel(lg_g[step][slot], lg_e[step][slot]) < 0.05

        # recycle slot 0: its 2 pages return to a pool of 8 usable pages
        # with 4 free, and the 21-token prompt (30 reserved -> 2 pages)
        # gets the stale ones back
        stale = list(graphed._slot_pages[0])
        graphed.release_slot(0)
        assert graphed.pool.num_free == 6
        lg_r = run(graphed, [prompts[2], prompts[1]],
                   [forced[2], forced[1]], prefill=[0, 1])
        assert set(graphed._slot_pages[0]) & set(stale)
        for step in range(8):
            assert rel(lg_r[step][0], refs[2][step]) < 0.05, step
            assert rel(lg_r[step][1], refs[1][step]) < 0.05, step
        graphed.release_slot(0)
        graphed.release_slot(1)
        assert graphed.pool.num_free == graphed.pool.num_usable
