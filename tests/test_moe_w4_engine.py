"""MXFP4 expert weights in the model (moe-tiny): quantize_experts_mxfp4 on
the CPU, MoEMLP in the PagedDecoder paths, captured graph against eager, and
the engine with weight_dtype="mxfp4"."""
import copy

import pytest
import torch

from ray_amd import ops
from ray_amd.llm.engine import ContinuousBatchingEngine, LLMConfig
from ray_amd.models.llama import (CONFIGS, LlamaModel, MoEMLP,
                                  quantize_experts_mxfp4)

CFG = CONFIGS["moe-tiny"]
NAMES = ("w_gate", "w_up", "w_down")


def _model(dev, dtype=torch.bfloat16):
    torch.manual_seed(0)
    m = LlamaModel(CFG, dtype=dtype).to(dev).eval()
    m.cosT, m.sinT = m.cosT.to(dev), m.sinT.to(dev)
    return m


def _dequantised(mlp, dtype):
    return [ops.dequantize_mxfp4(
        getattr(mlp, n + "_q").flatten(0, 1), getattr(mlp, n + "_s").flatten(0, 1),
        dtype).view(getattr(mlp, n + "_q").shape[:2] + (-1,)) for n in NAMES]


@torch.no_grad()
def test_quantize_experts_on_the_cpu():
    m = _model("cpu", torch.float32)
    plain = copy.deepcopy(m)
    quantize_experts_mxfp4(m)
    E, H, I = CFG.num_experts, CFG.hidden_size, CFG.intermediate_size
    for layer, ref in zip(m.layers, plain.layers):
        mlp = layer.mlp
        assert [n for n, _ in mlp.named_parameters()] == ["router.weight"]
        held = [getattr(mlp, n + t) for n in NAMES for t in ("_q", "_s")]
        assert all(t.dtype == torch.uint8 for t in held)
        assert sum(t.numel() for t in held) * 32 == 3 * E * H * I * 17
        for n, w in zip(NAMES, _dequantised(mlp, torch.float32)):
            getattr(ref.mlp, n).copy_(w)
    g = torch.Generator().manual_seed(0)
    tokens = torch.randint(0, CFG.vocab_size, (2, 24), generator=g)
    assert torch.equal(m(tokens), plain(tokens))


def _check_call(mlp, x, r, y):
    """One MoEMLP call against the float64 reference on the dequantised
    weights under the router kernel's routing: 2^-8 (|y| + A) + 2^-8 |r|."""
    H = x.shape[-1]
    x, r, y = (t.reshape(-1, H) for t in (x, r, y))
    idx, w = ops.moe_route(x, mlp.router.weight, mlp.top_k)
    x, r, idx, w = x.cpu(), r.cpu().double(), idx.cpu(), w.cpu()
    Wg, Wu, Wd = (t.cpu() for t in _dequantised(mlp, torch.bfloat16))
    ref = ops.moe_experts_ref(x, idx, w, Wg, Wu, Wd) + r
    A = torch.zeros_like(ref)
    for j in range(idx.shape[1]):
        e = idx[:, j].long()
        h = (torch.nn.functional.silu(
            torch.einsum("mh,mih->mi", x.double(), Wg[e].double()))
            * torch.einsum("mh,mih->mi", x.double(), Wu[e].double()))
        A += w[:, j:j + 1].double() * torch.einsum(
            "mi,mhi->mh", h.abs(), Wd[e].double().abs())
    bound = 2.0 ** -8 * (ref.abs() + A + r.abs())
    ratio = ((y.cpu().double() - ref).abs() / bound).max().item()
    print(f"MoEMLP mxfp4 {x.shape[0]} rows: max error/bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.gpu
@torch.no_grad()
def test_decoder_paths_and_captured_step():
    from ray_amd.llm.paged import PagedDecoder

    dev = torch.device("cuda:0")
    m = quantize_experts_mxfp4(_model(dev))
    pd = PagedDecoder(m, 3, 96, dev, prefill_chunk=64, spec_tokens=3)
    calls = []
    hooks = [layer.mlp.register_forward_hook(
        lambda mod, args, kw, out: calls.append(
            (mod, args[0].clone(), kw["residual"].clone(), out.clone())),
        with_kwargs=True) for layer in m.layers]
    lens = [37, 5, 9]
    for s, n in enumerate(lens):
        pd.prefill_slot(s, torch.arange(n, device=dev) * 7 % 500 + 3,
                        reserve_tokens=n + 16)

    def steps(first, count):
        out = []
        for i in range(first, first + count):
            pos = torch.tensor(lens, device=dev) + i
            for s in range(3):
                pd.set_slot_len(s, int(pos[s]) + 1)
            out.append(pd.decode(torch.tensor([11, 12, 13], device=dev) + i,
                                 pos).clone())
        return out

    steps(0, 3)
    ctx = torch.tensor(lens, dtype=torch.int32) + 3
    pd.verify(torch.arange(12, device=dev).view(3, 4) + 40, ctx,
              torch.tensor([4, 2, 3], dtype=torch.int32))
    # per layer: three prefills, three decode steps, one verify
    assert len(calls) == CFG.num_layers * 7
    for call in calls:
        _check_call(*call)
    for h in hooks:
        h.remove()
    eager = steps(3, 5)
    pd.capture()
    assert pd.graph is not None
    for a, b in zip(eager, steps(3, 5)):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_engine_serves_mxfp4_experts():
    prompts = [list(range(3, 3 + n)) for n in (5, 40, 17, 2, 33, 9)]
    new = [6, 3, 9, 12, 4, 7]

    def run(**kw):
        eng = ContinuousBatchingEngine(LLMConfig(
            model_id="moe-tiny", kv_cache="paged", weight_dtype="mxfp4",
            max_batch_size=4, **kw))
        assert all(hasattr(layer.mlp, "w_gate_q")
                   for layer in eng.model.layers)
        rids = [eng.submit(p, n) for p, n in zip(prompts, new)]
        done = eng.run_until_complete()
        return [done[r] for r in rids]

    first = run()
    assert [len(t) for t in first] == new
    assert run(use_hip_graph=False) == first
