"""Mixture-of-experts models (moe-tiny): the model on the CPU, MoEMLP in
the PagedDecoder paths, captured graph against eager, and the engine."""
import pytest
import torch

from ray_amd import ops
from ray_amd.llm.engine import ContinuousBatchingEngine, LLMConfig
from ray_amd.models.llama import CONFIGS, LlamaModel, MoEMLP

CFG = CONFIGS["moe-tiny"]


def _model(dev, dtype=torch.bfloat16):
    torch.manual_seed(0)
    m = LlamaModel(CFG, dtype=dtype).to(dev).eval()
    m.cosT, m.sinT = m.cosT.to(dev), m.sinT.to(dev)
    return m


def test_model_has_expert_blocks_and_trains():
    m = _model("cpu", torch.float32)
    E, H, I = CFG.num_experts, CFG.hidden_size, CFG.intermediate_size
    assert all(isinstance(layer.mlp, MoEMLP) for layer in m.layers)
    dense = LlamaModel(CONFIGS["llama-tiny"], dtype=torch.float32)
    assert m.num_params() - dense.num_params() == CFG.num_layers * (
        3 * E * H * I + E * H - 3 * H * I)
    chosen = []
    for layer in m.layers:
        layer.mlp.register_forward_pre_hook(
            lambda mod, args: chosen.append(ops.moe_route(
                args[0].detach().reshape(-1, H), mod.router.weight.detach(),
                mod.top_k)[0].unique().long()))
    g = torch.Generator().manual_seed(0)
    tokens = torch.randint(0, CFG.vocab_size, (2, 24), generator=g)
    m.train()(tokens, tokens.roll(-1, 1)).backward()
    for layer, used in zip(m.layers, chosen):
        mlp = layer.mlp
        assert torch.isfinite(mlp.router.weight.grad).all()
        for p in (mlp.w_gate, mlp.w_up, mlp.w_down):
            assert torch.isfinite(p.grad).all()
            assert (p.grad[used].abs().sum(dim=(1, 2)) > 0).all()


def _check_capture(mlp, x, r, y):
    """One MoEMLP call against the float64 experts reference under the
    routing the router kernel gives for the same input: the bound of
    tests/test_moe.py, 2^-8 (|y| + A) + 2^-8 |r|."""
    H = x.shape[-1]
    x, r, y = (t.reshape(-1, H) for t in (x, r, y))
    idx, w = ops.moe_route(x, mlp.router.weight, mlp.top_k)
    x, r, idx, w = x.cpu(), r.cpu().double(), idx.cpu(), w.cpu()
    Wg, Wu, Wd = (p.detach().cpu() for p in (mlp.w_gate, mlp.w_up, mlp.w_down))
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
    assert ((y.cpu().double() - ref).abs() <= bound).all()


@pytest.mark.gpu
@torch.no_grad()
def test_decoder_paths_run_the_expert_kernels():
    from ray_amd.llm.paged import PagedDecoder

    dev = torch.device("cuda:0")
    m = _model(dev)
    pd = PagedDecoder(m, 3, 96, dev, prefill_chunk=64, spec_tokens=3)
    calls = []
    for layer in m.layers:
        layer.mlp.register_forward_hook(
            lambda mod, args, kw, out: calls.append(
                (mod, args[0].clone(), kw["residual"].clone(), out.clone())),
            with_kwargs=True)
    lens = [37, 5, 9]
    for s, n in enumerate(lens):
        pd.prefill_slot(s, torch.arange(n, device=dev) * 7 % 500 + 3,
                        reserve_tokens=n + 8)
    for i in range(3):
        pos = torch.tensor(lens, device=dev) + i
        for s in range(3):
            pd.set_slot_len(s, int(pos[s]) + 1)
        pd.decode(torch.tensor([11, 12, 13], device=dev) + i, pos)
    ctx = torch.tensor(lens, dtype=torch.int32) + 3
    pd.verify(torch.arange(12, device=dev).view(3, 4) + 40, ctx,
              torch.tensor([4, 2, 3], dtype=torch.int32))
    # per layer: three prefills, three decode steps, one verify
    assert len(calls) == CFG.num_layers * 7
    assert {c[1].numel() // CFG.hidden_size for c in calls} == {37, 5, 9, 3,
                                                                12}
    for call in calls:
        _check_capture(*call)


@pytest.mark.gpu
@torch.no_grad()
def test_captured_step_is_bitwise_the_eager_step():
    from ray_amd.llm.paged import PagedDecoder

    dev = torch.device("cuda:0")
    pd = PagedDecoder(_model(dev), 3, 96, dev)
    lens = [21, 4, 0]  # slot 2 stays inactive
    for s, n in enumerate(lens[:2]):
        pd.prefill_slot(s, torch.arange(n, device=dev) * 5 % 500 + 1,
                        reserve_tokens=n + 8)

    def steps():
        out = []
        for i in range(5):
            pos = torch.tensor(lens, device=dev) + i
            for s in range(2):
                pd.set_slot_len(s, int(pos[s]) + 1)
            toks = torch.tensor([100, 200, 0], device=dev) + 3 * i
            out.append(pd.decode(toks, pos)[:2].clone())
        return out

    eager = steps()
    pd.capture()
    assert pd.graph is not None
    for a, b in zip(eager, steps()):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_engine_drains_mixed_requests():
    prompts = [list(range(3, 3 + n)) for n in (5, 40, 17, 2, 33, 9)]
    new = [6, 3, 9, 12, 4, 7]

    def run(**kw):
        eng = ContinuousBatchingEngine(LLMConfig(
            model_id="moe-tiny", kv_cache="paged", max_batch_size=4, **kw))
        rids = [eng.submit(p, n) for p, n in zip(prompts, new)]
        done = eng.run_until_complete()
        return [done[r] for r in rids]

    first = run()
    assert [len(t) for t in first] == new
    assert run(use_hip_graph=False) == first
    with pytest.raises(ValueError, match="not built yet"):
        run(weight_dtype="fp8")
