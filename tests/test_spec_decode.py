"""Speculative decoding: exact acceptance in the engine on CPU, the
PagedDecoder verify step and the engine end to end on the GPU."""
import pytest
import torch

from ray_amd import ops
from ray_amd.llm.engine import ContinuousBatchingEngine, LLMConfig, LLMEngine

# repeated n-grams, so that prompt lookup has something to find
PROMPTS = [[5, 6, 7, 8] * 5, list(range(40, 52)) * 2 + [40, 41],
           [9, 3, 9, 3, 9, 3, 200, 9, 3]]
NEW = [12, 9, 15]


def _engine(cpu=True, **kw):
    """cpu: an fp32 engine on the CPU wherever the test runs, where equal
    tokens can be asked for (an engine picks its device when it is built)."""
    kw = {"model_id": "llama-tiny", "max_seq_len": 128, "max_batch_size": 2,
          "kv_cache": "paged", **kw}
    with pytest.MonkeyPatch.context() as mp:
        if cpu:
            mp.setattr(torch.cuda, "is_available", lambda: False)
        return ContinuousBatchingEngine(LLMConfig(**kw))


def _run(eng, extra=()):
    rids = [eng.submit(p, n) for p, n in zip(PROMPTS, NEW)]
    rids += [eng.submit(*a, **k) for a, k in extra]
    done = eng.run_until_complete()
    assert eng.stats["kv_pages_free"] == eng.stats["kv_pages_total"]
    return [done[r] for r in rids]


@pytest.fixture(scope="module")
def baseline():
    eng = _engine()
    return _run(eng), eng.stats["decode_steps"]


def _oracle(baseline_tokens):
    """A proposer that knows the baseline's continuation of each prompt."""
    full = [p + t for p, t in zip(PROMPTS, baseline_tokens)]

    def propose(tokens, k):
        for f in full:
            if f[: len(tokens)] == tokens:
                return f[len(tokens): len(tokens) + k]
        return []
    return propose


@pytest.mark.parametrize("kind", ["oracle", "wrong", "ngram"])
def test_speculation_returns_the_baseline_tokens(baseline, kind):
    tokens, steps = baseline
    # "wrong" drafts a token the baseline never emits: none can be accepted
    never = next(t for t in range(512) if all(t not in o for o in tokens))
    proposer = {"oracle": _oracle(tokens),
                "wrong": lambda toks, k: [never] * k, "ngram": None}[kind]
    eng = _engine(num_speculative_tokens=4, speculative_proposer=proposer)
    assert _run(eng) == tokens
    drafted, accepted = (eng.stats["spec_draft_tokens"],
                         eng.stats["spec_accepted_tokens"])
    assert drafted > 0
    if kind == "oracle":
        assert accepted == drafted
        assert eng.stats["decode_steps"] < steps
    elif kind == "wrong":
        assert accepted == 0


def test_sampled_request_is_not_speculated(baseline):
    tokens, _ = baseline
    extra = [((PROMPTS[0], 10), {"temperature": 0.8, "top_k": 20, "seed": 7})]
    plain = _run(_engine(), extra)
    spec = _run(_engine(num_speculative_tokens=4,
                        speculative_proposer=_oracle(tokens)), extra)
    assert spec == plain and plain[:3] == tokens


def test_config_errors():
    with pytest.raises(ValueError, match="paged"):
        _engine(kv_cache="contiguous", num_speculative_tokens=2)
    with pytest.raises(ValueError, match="paged"):
        LLMEngine(LLMConfig(model_id="llama-tiny", num_speculative_tokens=2))
    with pytest.raises(ValueError, match="device_sampling"):
        _engine(device_sampling=True, num_speculative_tokens=2)
    with pytest.raises(ValueError, match="spec_tokens=16"):
        _engine(num_speculative_tokens=16)  # 17 rows x REP 2 > 32
    with pytest.raises(ValueError):
        LLMConfig(num_speculative_tokens=-1)


@pytest.mark.gpu
@pytest.mark.parametrize("kv_dtype", [torch.bfloat16, torch.float8_e4m3fn])
def test_verify_step_gpu_logits(kv_dtype):
    """Teacher-forced PagedDecoder.verify, eager and captured, fed 4 forced
    tokens at a time with mixed q_lens, against the per-sequence KVCache
    path (the reference and criterion of test_paged_decoder_gpu_logits);
    then slot 0 is released and reused."""
    from ray_amd.llm.paged import PagedDecoder
    from ray_amd.models.llama import CONFIGS, KVCache, LlamaModel

    dev = torch.device("cuda:0")
    cfg = CONFIGS["llama-tiny"]
    torch.manual_seed(0)
    m = LlamaModel(cfg, dtype=torch.bfloat16).to(dev).eval()
    m.cosT, m.sinT = m.cosT.to(dev), m.sinT.to(dev)
    hd = cfg.hidden_size // cfg.num_heads
    prompts = [list(range(5, 15)), list(range(50, 58)),
               list(range(200, 221))]
    forced = [list(range(300, 308)), list(range(400, 408)),
              list(range(330, 338))]

    def reference(p, f):
        caches = [KVCache(1, 96, cfg.num_kv_heads, hd, dev, torch.bfloat16)
                  for _ in range(cfg.num_layers)]
        m(torch.tensor([p], device=dev), kv_caches=caches, pos0=0)
        rows = [m(torch.tensor([[t]], device=dev), kv_caches=caches,
                  pos0=len(p) + i)[0, -1].float() for i, t in enumerate(f)]
        return torch.stack(rows)

    def run(pd, slots):
        """slots: {slot: prompt index}; 8 forced tokens per slot, slot s
        taking 4 - s rows a call. Returns {slot: logits [8, V]}."""
        got = {s: [] for s in slots}
        fed = {s: 0 for s in slots}
        while any(fed[s] < 8 for s in slots):
            toks = torch.zeros(2, 4, dtype=torch.long, device=dev)
            ctx = torch.zeros(2, dtype=torch.int32)
            ql = torch.zeros(2, dtype=torch.int32)
            for s, i in slots.items():
                n = min(4 - s, 8 - fed[s])
                toks[s, :n] = torch.tensor(forced[i][fed[s]: fed[s] + n])
                ctx[s], ql[s] = len(prompts[i]) + fed[s], n
            lg = pd.verify(toks, ctx, ql).float()
            for s in slots:
                got[s].append(lg[s, : int(ql[s])].clone())
                fed[s] += int(ql[s])
                pd.set_slot_len(s, int(ctx[s]) + int(ql[s]))
        return {s: torch.cat(v) for s, v in got.items()}

    with torch.no_grad():
        refs = [reference(p, f) for p, f in zip(prompts, forced)]
        for capture in (False, True):
            pd = PagedDecoder(m, 2, 96, dev, num_pages=9, kv_dtype=kv_dtype,
                              spec_tokens=3)
            if capture:
                pd.capture()
                assert pd.verify_graph is not None
            for s in (0, 1):
                pd.prefill_slot(s, torch.tensor(prompts[s], device=dev),
                                reserve_tokens=len(prompts[s]) + 9)
            got = run(pd, {0: 0, 1: 1})
            pd.release_slot(0)
            pd.prefill_slot(0, torch.tensor(prompts[2], device=dev),
                            reserve_tokens=len(prompts[2]) + 9)
            got2 = run(pd, {0: 2})
            for out, ref in ((got[0], refs[0]), (got[1], refs[1]),
                             (got2[0], refs[2])):
                rel = (out - ref).norm(dim=-1) / (ref.norm(dim=-1) + 1e-6)
                assert float(rel.max()) < 0.05, (capture, rel.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("weight_dtype", ["auto", "fp8"])
def test_engine_gpu_end_to_end(weight_dtype):
    def run():
        eng = _engine(cpu=False, num_speculative_tokens=3,
                      weight_dtype=weight_dtype, max_loras=1)
        g = torch.Generator().manual_seed(0)
        eng.add_lora("a", {
            name: (torch.randn(16, mod.in_features, generator=g) * 0.2,
                   torch.randn(mod.out_features, 16, generator=g) * 0.2)
            for name, mod in eng.model.named_modules()
            if isinstance(mod, ops.LoraLinear)})
        out = _run(eng, [((PROMPTS[1], 11), {"lora": "a"})])
        assert (eng.stats["spec_accepted_tokens"]
                <= eng.stats["spec_draft_tokens"])
        return out

    first = run()
    assert [len(t) for t in first] == NEW + [11]
    assert all(0 <= t < 512 for out in first for t in out)
    assert run() == first
