"""Multi-LoRA serving: a mixed batch through the graph-captured PagedDecoder
(GPU) and the ContinuousBatchingEngine surface (CPU)."""
import copy

import pytest
import torch

from ray_amd import ops
from ray_amd.llm.engine import ContinuousBatchingEngine, LLMConfig, LLMEngine
from ray_amd.llm.paged import PagedDecoder
from ray_amd.models.llama import CONFIGS, LlamaModel, add_lora_slots

PROMPT_LENS, ADAPTERS, STEPS = (35, 3, 9, 5, 12), (0, -1, 1, 0, -1), 4


def _random_adapter(model, rank, std, seed):
    """{module path: (A [rank, K], B [N, rank])} for every adapted
    projection."""
    g = torch.Generator().manual_seed(seed)
    return {name: (torch.randn(rank, mod.in_features, generator=g) * std,
                   torch.randn(mod.out_features, rank, generator=g) * std)
            for name, mod in model.named_modules()
            if isinstance(mod, ops.LoraLinear)}


@torch.no_grad()
def _decode(model, prompts, fed, capture):
    dev = fed.device
    dec = PagedDecoder(model, len(prompts), 96, dev)
    if capture:
        dec.capture()
    for slot, p in enumerate(prompts):
        kw = {"lora_slot": ADAPTERS[slot]} if dec.lora_state else {}
        dec.prefill_slot(slot, p, p.numel() + STEPS, **kw)
    pos = torch.tensor(PROMPT_LENS, device=dev)
    out = []
    for i in range(STEPS):
        dec.seq_lens.copy_(pos + i + 1)
        out.append(dec.decode(fed[i], pos + i).float().clone())
    return torch.stack(out)  # [STEPS, B, V]


def _forward(model, prompts, fed, adapters):
    """[STEPS, B, V] from LlamaModel's full forward, one sequence at a time.
    Grad mode on (nothing requires grad) sends ops.lora_add to its torch
    composition."""
    out = []
    for b, p in enumerate(prompts):
        seq = torch.cat([p, fed[:, b]]).view(1, -1)
        if adapters[b] >= 0:
            model.lora_state.idx = torch.full(
                (seq.numel(),), adapters[b], dtype=torch.int32,
                device=seq.device)
        with torch.enable_grad():
            out.append(model(seq)[0, p.numel():].float())
        if adapters[b] >= 0:
            model.lora_state.idx = None
    return torch.stack(out, dim=1)


@pytest.mark.gpu
def test_mixed_batch_through_captured_decoder():
    """Slots with adapters 0 (rank 8, zero-padded to 16), 1 (rank 16) and
    none in one batch. The yardstick is the base decoder's distance from the
    base model's full forward."""
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    vocab = CONFIGS["llama-tiny"].vocab_size
    base = LlamaModel(CONFIGS["llama-tiny"]).to(dev).eval()
    base.requires_grad_(False)
    model = copy.deepcopy(base)
    add_lora_slots(model, 4, 16)
    for slot, (rank, scale) in enumerate(((8, 2.0), (16, 1.0))):
        for name, (A, B) in _random_adapter(model, rank, 0.05, slot).items():
            mod = model.get_submodule(name)
            mod.lora_A[slot, :rank] = A.to(dev)
            mod.lora_B[slot, :, :rank] = B.to(dev)
            mod.lora_scale[slot] = scale
    prompts = [torch.randint(0, vocab, (n,), device=dev) for n in PROMPT_LENS]
    fed = torch.randint(0, vocab, (STEPS, len(prompts)), device=dev)

    eager = _decode(model, prompts, fed, capture=False)
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, _decode(model, prompts, fed, capture=True))
    plain = _decode(base, prompts, fed, capture=False)
    none = [-1] * len(prompts)
    yardstick = float((_forward(base, prompts, fed, none) - plain).abs().max())
    err = float((_forward(model, prompts, fed, ADAPTERS) - eager).abs().max())
    print(f"lora decoder vs forward {err:.4e}; base decoder vs forward "
          f"{yardstick:.4e}")
    assert err <= 2 * yardstick
    for b, a in enumerate(ADAPTERS):
        if a < 0:
            assert torch.equal(eager[:, b], plain[:, b])
        else:
            assert float((eager[:, b] - plain[:, b]).abs().max()) > yardstick


def _engine(**kw):
    return ContinuousBatchingEngine(LLMConfig(
        model_id="llama-tiny", max_seq_len=128, max_batch_size=4,
        kv_cache="paged", max_loras=2, **kw))


def test_engine_surface_on_cpu():
    eng = _engine()
    assert eng.stats["loras_loaded"] == 0
    for i, name in enumerate("ab"):
        eng.add_lora(name, _random_adapter(eng.model, 8 * (i + 1), 0.2, i),
                     alpha=16.0)
    assert eng.stats["loras_loaded"] == 2
    prompt = list(range(7, 30))
    alone = {}
    for lora in ("a", "b", None):
        rid = eng.submit(prompt, 6, lora=lora)
        alone[lora] = eng.run_until_complete()[rid]
    assert len({tuple(v) for v in alone.values()}) == 3
    order = ["a", None, "b", "a", None, "b"]
    rids = [eng.submit(prompt, 6, lora=lora) for lora in order]
    mixed = eng.run_until_complete()
    assert [mixed[r] for r in rids] == [alone[lora] for lora in order]

    with pytest.raises(ValueError):
        eng.submit(prompt, 6, lora="c")
    with pytest.raises(ValueError):
        eng.add_lora("c", {})
    with pytest.raises(ValueError):  # a shape that does not fit
        _engine().add_lora("a", {"layers.0.attn.o_proj": (
            torch.zeros(8, 3), torch.zeros(256, 8))})
    with pytest.raises(ValueError):  # rank above max_lora_rank
        _engine().add_lora("a", {"layers.0.attn.o_proj": (
            torch.zeros(17, 256), torch.zeros(256, 17))})
    eng.submit(prompt, 6, lora="a")
    with pytest.raises(ValueError):
        eng.remove_lora("a")
    eng.step()
    with pytest.raises(ValueError):
        eng.remove_lora("a")
    eng.run_until_complete()
    eng.remove_lora("a")
    assert eng.stats["loras_loaded"] == 1
    for bad in (ContinuousBatchingEngine, LLMEngine):
        with pytest.raises(ValueError):
            bad(LLMConfig(model_id="llama-tiny", max_loras=2))
    with pytest.raises(ValueError):
        _engine(max_lora_rank=65)


def test_prefix_cache_is_per_adapter():
    eng = _engine(enable_prefix_caching=True)
    eng.add_lora("a", _random_adapter(eng.model, 16, 0.2, 0))
    prompt = list(range(40))

    def hits(lora):
        before = eng.stats["prefix_hit_tokens"]
        rid = eng.submit(prompt, 2, lora=lora)
        tokens = eng.run_until_complete()[rid]
        return eng.stats["prefix_hit_tokens"] - before, tokens

    assert hits(None)[0] == 0
    first = hits("a")
    assert first[0] == 0
    assert hits("a") == (32, first[1])
    # a re-registered name does not hit its predecessor's pages
    eng.remove_lora("a")
    eng.add_lora("a", _random_adapter(eng.model, 16, 0.2, 1))
    assert hits("a")[0] == 0
