"""FP8 weight-only linear: quantize_weight_fp8, ops.linear_w8 (the
csrc/hip/linear_w8.hip skinny GEMM and its dequantise fallback), LinearW8,
quantize_linears_fp8 and LLMConfig.weight_dtype."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from ray_amd import ops
from ray_amd.llm import ContinuousBatchingEngine, LLMConfig
from ray_amd.llm.paged import PagedDecoder
from ray_amd.models import llama
from ray_amd.models.llama import CONFIGS, LlamaModel

FP8 = torch.float8_e4m3fn


def _dequant(wq, scale, dtype=torch.float32):
    return (wq.float() * scale[:, None]).to(dtype)


def _dev():
    return torch.device("cuda", 0)


# ---- CPU -----------------------------------------------------------------


def test_quantize_weight_fp8():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(6, 256, generator=g).bfloat16()
    w[2] = 0
    w[3, 5], w[3, 9] = w[3].abs().max(), -w[3].abs().max()
    wq, scale = ops.quantize_weight_fp8(w)
    assert wq.dtype == FP8 and scale.dtype == torch.float32
    amax = w.float().abs().amax(1)
    assert torch.equal(scale[amax > 0], (amax / 448)[amax > 0])
    assert scale[2] == 1 and (wq[2].view(torch.uint8) == 0).all()
    assert wq[3, 5].float() == 448 and wq[3, 9].float() == -448
    assert ((wq.view(torch.uint8) & 0x7F) != 0x7F).all()
    wq32, scale32 = ops.quantize_weight_fp8(w.float())
    assert torch.equal(wq32.view(torch.uint8), wq.view(torch.uint8))
    assert torch.equal(scale32, scale)


@pytest.mark.parametrize("rows", [1, 3, 40])
def test_linear_w8_cpu_is_dequantised_linear(rows):
    g = torch.Generator().manual_seed(rows)
    wq, scale = ops.quantize_weight_fp8(torch.randn(24, 128, generator=g))
    x = torch.randn(rows, 1, 128, generator=g)
    want = F.linear(x, _dequant(wq, scale))
    assert torch.equal(ops.linear_w8(x, wq, scale), want)
    assert torch.equal(ops.LinearW8(wq, scale)(x), want)


def _engine(**kw):
    return ContinuousBatchingEngine(LLMConfig(
        model_id="llama-tiny", max_seq_len=96, max_batch_size=2,
        use_hip_graph=False, **kw))


def test_weight_dtype_validation():
    with pytest.raises(ValueError):
        _engine(kv_cache="paged", weight_dtype="int4")
    with pytest.raises(ValueError):
        _engine(kv_cache="contiguous", weight_dtype="fp8")


def test_engine_fp8_weights_cpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    eng = _engine(kv_cache="paged", weight_dtype="fp8")
    ref = _engine(kv_cache="paged")
    saved = 0
    for name, mod in eng.model.named_modules():
        if isinstance(mod, ops.LinearW8):
            lin = ref.model.get_submodule(name)
            n, k = lin.weight.shape
            saved += n * k * lin.weight.element_size() - (n * k + 4 * n)
            lin.weight.data.copy_(_dequant(mod.wq, mod.scale))
    layers = CONFIGS["llama-tiny"].num_layers
    assert len([m for m in eng.model.modules()
                if isinstance(m, ops.LinearW8)]) == 5 * layers + 1
    assert ref.stats["weight_bytes"] - eng.stats["weight_bytes"] == saved > 0
    prompts = [[3, 1, 4, 1, 5, 9, 2, 6], list(range(40, 61))]
    outs = []
    for e in (eng, ref):
        ids = [e.submit(p, max_new_tokens=6) for p in prompts]
        done = e.run_until_complete()
        outs.append([done[i] for i in ids])
    assert outs[0] == outs[1]


# ---- GPU: the kernel -----------------------------------------------------

SHAPES = [(16, 128), (40, 256), (33, 2176), (512, 1024), (4096, 512)]


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """x, wq, scale as slices of buffers whose neighbouring rows are NaN
    (bf16, fp32) and 0x7F bytes, the fp64 reference and the bound."""
    g = torch.Generator().manual_seed(1000 * M + N + K)
    wq, scale = ops.quantize_weight_fp8(torch.randn(N, K, generator=g))
    x = torch.randn(M, K, generator=g).bfloat16()
    xb = torch.full((M + 2, K), float("nan"), dtype=torch.bfloat16)
    wb = torch.full((N + 2, K), 0x7F, dtype=torch.uint8)
    sb = torch.full((N + 2,), float("nan"))
    xb[1:-1], wb[1:-1], sb[1:-1] = x, wq.view(torch.uint8), scale
    ref = ops.linear_w8_ref(x, wq, scale).double()
    mag = x.double().abs() @ _dequant(wq, scale).double().abs().t()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag
    d = _dev()
    return (xb.to(d)[1:-1], wb.to(d).view(FP8)[1:-1], sb.to(d)[1:-1], ref,
            bound)


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [1, 2, 3, 8, 16, 17, 32])
def test_kernel_against_fp64_reference(M, N, K):
    x, wq, scale, ref, bound = _case(M, N, K)
    with torch.no_grad():
        y = ops._K.linear_w8(x, wq, scale)
        y32 = ops._K.linear_w8(x, wq, scale, tile=32)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    assert torch.equal(y, y32)  # the result does not depend on the grid
    y = y.double().cpu()
    assert torch.isfinite(y).all()
    assert ((y - ref).abs() <= bound).all(), ((y - ref).abs() - bound).max()


@pytest.mark.gpu
def test_kernel_converts_every_byte_exactly():
    n, k = torch.arange(256)[:, None], torch.arange(128)[None, :]
    b = ((n + k) % 256).to(torch.uint8)
    b[(b & 0x7F) == 0x7F] = 0
    wq = b.view(FP8)
    scale = torch.tensor([0.5, 2.0]).repeat(128)
    x = torch.zeros(32, 128, dtype=torch.bfloat16)
    x[torch.arange(32), 4 * torch.arange(32)] = 1
    assert set(b[:, ::4].flatten().tolist()) == set(range(256)) - {0x7F, 0xFF}
    want = (wq.float()[:, ::4] * scale[:, None]).bfloat16().t()
    with torch.no_grad():
        y = ops.linear_w8(x.to(_dev()), wq.to(_dev()), scale.to(_dev()))
    assert torch.equal(y.cpu(), want.contiguous())


@pytest.mark.gpu
def test_kernel_is_deterministic():
    x, wq, scale, _, _ = _case(17, 4096, 512)
    with torch.no_grad():
        a, b = ops.linear_w8(x, wq, scale), ops.linear_w8(x, wq, scale)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.gpu
def test_dispatch(monkeypatch):
    calls = []

    class Spy:
        def linear_w8(self, *a):
            calls.append(tuple(a[0].shape))
            return real.linear_w8(*a)

        def __getattr__(self, name):
            return getattr(real, name)

    real = ops._K
    monkeypatch.setattr(ops, "_K", Spy())
    g = torch.Generator().manual_seed(5)
    wq, scale = (t.to(_dev()) for t in ops.quantize_weight_fp8(
        torch.randn(64, 1024, generator=g)))
    x = torch.randn(33, 1024, generator=g).bfloat16().to(_dev())

    def fallback(x, wq, scale):
        return F.linear(x, _dequant(wq, scale, torch.bfloat16))

    with torch.no_grad():
        assert torch.equal(ops.linear_w8(x, wq, scale),
                           fallback(x, wq, scale))
        assert torch.equal(
            ops.linear_w8(x[:4, :192], wq[:, :192].contiguous(), scale),
            fallback(x[:4, :192], wq[:, :192], scale))
    with torch.enable_grad():
        assert torch.equal(ops.linear_w8(x[:4], wq, scale),
                           fallback(x[:4], wq, scale))
    assert calls == []
    with torch.no_grad():
        y = ops.linear_w8(x[:32].view(4, 8, 1024), wq, scale)
    assert calls == [(32, 1024)] and y.shape == (4, 8, 64)


# ---- GPU: the decoder ----------------------------------------------------

PROMPT_LENS, STEPS = (5, 16, 35), 8
# Max abs logit distance allowed between the fp8-weight decoder and the bf16
# decoder of a twin model holding (wq * scale).bfloat16(): twice what the
# existing bf16 PagedDecoder sits from LlamaModel's full-sequence forward on
# the same twin, prompts and steps. Measured on an MI355X: 7.8125e-3 for
# that yardstick (printed below), 1.1719e-2 for the fp8 decoder.
DECODER_TOL = 2 * 7.8125e-3


@torch.no_grad()
def _decode(model, prompts, fed, capture):
    dec = PagedDecoder(model, len(prompts), 64, _dev())
    if capture:
        dec.capture()
    for slot, p in enumerate(prompts):
        dec.prefill_slot(slot, p, p.numel() + STEPS)
    pos = torch.tensor(PROMPT_LENS, device=_dev())
    out = []
    for i in range(STEPS):
        dec.seq_lens.copy_(pos + i + 1)
        out.append(dec.decode(fed[i], pos + i).float().clone())
    return torch.stack(out)  # [STEPS, B, V]


@pytest.mark.gpu
@torch.no_grad()
def test_decoder_fp8_weights_eager_graph_and_twin():
    torch.manual_seed(3)
    vocab = CONFIGS["llama-tiny"].vocab_size
    model = LlamaModel(CONFIGS["llama-tiny"]).to(_dev()).eval()
    twin = copy.deepcopy(model)
    llama.quantize_linears_fp8(model)
    for name, mod in model.named_modules():
        assert not isinstance(mod, torch.nn.Linear)
        if isinstance(mod, ops.LinearW8):
            twin.get_submodule(name).weight.data.copy_(
                _dequant(mod.wq, mod.scale, torch.bfloat16))
    prompts = [torch.randint(0, vocab, (n,), device=_dev())
               for n in PROMPT_LENS]
    fed = torch.randint(0, vocab, (STEPS, len(prompts)), device=_dev())
    eager = _decode(model, prompts, fed, capture=False)
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, _decode(model, prompts, fed, capture=True))
    bf16 = _decode(twin, prompts, fed, capture=False)
    yardstick = max(float(
        (twin(torch.cat([p, fed[:, b]]).view(1, -1))[0, p.numel():].float()
         - bf16[:, b]).abs().max()) for b, p in enumerate(prompts))
    err = float((eager - bf16).abs().max())
    print(f"fp8 decoder vs bf16 twin {err:.4e}; bf16 decoder vs forward "
          f"{yardstick:.4e}")
    assert err <= DECODER_TOL
