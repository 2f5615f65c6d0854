"""MXFP4 weight-only linear: quantize_weight_mxfp4 / dequantize_mxfp4,
ops.linear_w4 (the csrc/hip/linear_w4.hip skinny GEMM, the dequantise kernel
and the torch fallback), LinearW4, quantize_linears_mxfp4 and
LLMConfig.weight_dtype="mxfp4"."""
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

GRID = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6])


def _dev():
    return torch.device("cuda", 0)


# ---- CPU -----------------------------------------------------------------


def test_quantize_weight_mxfp4():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(6, 128, generator=g).double()
    w[1, 32:64] = 0
    w[2, :32] *= 2.0 ** -140   # amax far below the lower clamp
    w[2, 32:64] *= 2.0 ** 130  # and above the upper one
    wq, sc = ops.quantize_weight_mxfp4(w)
    assert wq.shape == (6, 64) and sc.shape == (6, 4)
    assert wq.dtype == sc.dtype == torch.uint8
    amax = w.view(6, 4, 32).abs().amax(2).double()
    want = (torch.floor(torch.log2(amax)) - 2 + 127).clamp(2, 252)
    want[amax == 0] = 127
    assert torch.equal(sc.double(), want)
    assert sc[2, 0] == 2 and sc[2, 1] == 252 and (sc != 0xFF).all()
    assert sc[1, 1] == 127 and (wq[1, 16:32] == 0).all()


@pytest.mark.parametrize("code", [2, 100, 127, 252])
def test_grid_round_trip_ties_and_saturation(code):
    s = 2.0 ** (code - 127)
    vals = torch.cat([GRID, -GRID[1:], GRID, -GRID[1:], GRID[:2]]).double()
    w = (vals * s).view(1, 32)
    wq, sc = ops.quantize_weight_mxfp4(w)
    assert sc.item() == code
    assert torch.equal(ops.dequantize_mxfp4(wq, sc, torch.float64), w)
    ties = torch.tensor([.25, .75, 1.25, 1.75, 2.5, 3.5, 5, 6, -.25, -5])
    ties = torch.cat([ties, torch.zeros(22)]).double().view(1, 32) * s
    wq, sc = ops.quantize_weight_mxfp4(ties)
    got = ops.dequantize_mxfp4(wq, sc, torch.float64)[0, :10] / s
    assert got.tolist() == [0, 1, 1, 2, 2, 4, 4, 6, 0, -4]
    # amax 7.5 keeps the exponent of 4: 7.5 and 6.5 both saturate at 6
    over = torch.tensor([7.5, -6.5] + [0.0] * 30).double().view(1, 32) * s
    wq, sc = ops.quantize_weight_mxfp4(over)
    assert sc.item() == code
    assert (ops.dequantize_mxfp4(wq, sc, torch.float64)[0, :2] / s
            ).tolist() == [6, -6]


@pytest.mark.parametrize("rows", [1, 3, 40])
def test_linear_w4_cpu_is_dequantised_linear(rows):
    g = torch.Generator().manual_seed(rows)
    wq, sc = ops.quantize_weight_mxfp4(torch.randn(24, 128, generator=g))
    x = torch.randn(rows, 1, 128, generator=g)
    want = F.linear(x, ops.dequantize_mxfp4(wq, sc))
    assert torch.equal(ops.linear_w4(x, wq, sc), want)
    assert torch.equal(ops.LinearW4(wq, sc)(x), want)


def _engine(**kw):
    return ContinuousBatchingEngine(LLMConfig(
        model_id="llama-tiny", max_seq_len=96, max_batch_size=2,
        use_hip_graph=False, **kw))


def test_engine_mxfp4_weights_cpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ValueError):
        _engine(kv_cache="contiguous", weight_dtype="mxfp4")
    eng = _engine(kv_cache="paged", weight_dtype="mxfp4")
    ref = _engine(kv_cache="paged")
    saved, count = 0, 0
    for name, mod in eng.model.named_modules():
        if isinstance(mod, ops.LinearW4):
            lin = ref.model.get_submodule(name)
            n, k = lin.weight.shape
            saved += n * k * lin.weight.element_size() - n * k * 17 // 32
            lin.weight.data.copy_(ops.dequantize_mxfp4(mod.wq, mod.scales))
            count += 1
    assert count == 5 * CONFIGS["llama-tiny"].num_layers + 1
    assert ref.stats["weight_bytes"] - eng.stats["weight_bytes"] == saved > 0
    prompts = [[3, 1, 4, 1, 5, 9, 2, 6], list(range(40, 61))]
    outs = []
    for e in (eng, ref):
        ids = [e.submit(p, max_new_tokens=6) for p in prompts]
        done = e.run_until_complete()
        outs.append([done[i] for i in ids])
    assert outs[0] == outs[1]


# ---- GPU: the kernels ----------------------------------------------------

SHAPES = [(16, 128), (40, 256), (33, 2176), (512, 1024), (4096, 512)]


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """x, wq, scales as slices of buffers whose neighbouring rows are NaN
    (x) and 0xFF bytes, the fp64 reference and the bound."""
    g = torch.Generator().manual_seed(1000 * M + N + K)
    wq, sc = ops.quantize_weight_mxfp4(torch.randn(N, K, generator=g))
    x = torch.randn(M, K, generator=g).bfloat16()
    xb = torch.full((M + 2, K), float("nan"), dtype=torch.bfloat16)
    wb = torch.full((N + 2, K // 2), 0xFF, dtype=torch.uint8)
    sb = torch.full((N + 2, K // 32), 0xFF, dtype=torch.uint8)
    xb[1:-1], wb[1:-1], sb[1:-1] = x, wq, sc
    ref = ops.linear_w4_ref(x, wq, sc).double()
    mag = x.double().abs() @ ops.dequantize_mxfp4(
        wq, sc, torch.float64).abs().t()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag
    d = _dev()
    return xb.to(d)[1:-1], wb.to(d)[1:-1], sb.to(d)[1:-1], ref, bound


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [1, 2, 3, 8, 16, 17, 32])
def test_kernel_against_fp64_reference(M, N, K):
    x, wq, sc, ref, bound = _case(M, N, K)
    with torch.no_grad():
        y = ops._K.linear_w4(x, wq, sc)
        # the result depends neither on the tile nor on the split of K
        for tile in (64, 128):
            for split in (1, 2, 4, 8):
                assert torch.equal(
                    y.view(torch.int16),
                    ops._K.linear_w4(x, wq, sc, tile=tile,
                                     split=split).view(torch.int16))
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    y = y.double().cpu()
    assert torch.isfinite(y).all()
    assert ((y - ref).abs() <= bound).all(), ((y - ref).abs() - bound).max()


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [64, 128])
def test_kernel_converts_every_nibble_exactly(tile):
    """One-hot rows of x pick k = 32g + 8j + i for every lane group g and
    nibble position i of a dword (dword j = (g + i) % 4); down each run of
    16 rows every nibble value passes through each of them. -0
    (nibble 8) leaves an fp32 sum as +0, so values are compared, as
    torch.equal does."""
    codes = [2, 126, 127, 128, 252]
    n, k = torch.arange(16 * len(codes))[:, None], torch.arange(128)[None, :]
    nib = ((n + k) % 16).to(torch.uint8).view(-1, 64, 2)
    wq = nib[..., 0] | (nib[..., 1] << 4)
    # every code in every lane group: block g of row n has code (n/16 + g)
    sc = torch.tensor(codes, dtype=torch.uint8)[
        (n // 16 + torch.arange(4)[None, :]) % len(codes)]
    gi = torch.arange(32)
    ks = 32 * (gi // 8) + 8 * ((gi // 8 + gi % 8) % 4) + gi % 8
    x = torch.zeros(32, 128, dtype=torch.bfloat16)
    x[gi, ks] = 1
    want = ops.dequantize_mxfp4(wq, sc, torch.bfloat16)[:, ks].t()
    assert torch.isfinite(want).all()
    with torch.no_grad():
        y = ops._K.linear_w4(x.to(_dev()), wq.to(_dev()), sc.to(_dev()),
                             tile=tile)
    assert torch.equal(y.cpu(), want.contiguous())


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", [(33, 2176), (512, 1024)])
def test_dequant_kernel_is_bit_exact(N, K):
    _, wq, sc, _, _ = _case(1, N, K)
    want = ops.dequantize_mxfp4(wq.cpu(), sc.cpu(), torch.bfloat16)
    got = ops._K.dequant_mxfp4(wq.contiguous(), sc.contiguous()).cpu()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.gpu
def test_dispatch(monkeypatch):
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name in ("linear_w4", "dequant_mxfp4"):
                return lambda *a: (calls.append((name, tuple(a[0].shape))),
                                   getattr(real, name)(*a))[1]
            return getattr(real, name)

    real = ops._K
    monkeypatch.setattr(ops, "_K", Spy())
    g = torch.Generator().manual_seed(5)
    wq, sc = (t.to(_dev()) for t in ops.quantize_weight_mxfp4(
        torch.randn(64, 1024, generator=g)))
    x = torch.randn(33, 1024, generator=g).bfloat16().to(_dev())

    def fallback(x, wq, sc):
        return F.linear(x, ops.dequantize_mxfp4(wq, sc, torch.bfloat16))

    with torch.no_grad():
        assert torch.equal(
            ops.linear_w4(x[:4, :192], wq[:, :96].contiguous(),
                          sc[:, :6].contiguous()),
            fallback(x[:4, :192], wq[:, :96], sc[:, :6]))
    with torch.enable_grad():
        assert torch.equal(ops.linear_w4(x[:4], wq, sc),
                           fallback(x[:4], wq, sc))
    assert calls == []
    with torch.no_grad():
        assert torch.equal(ops.linear_w4(x, wq, sc), fallback(x, wq, sc))
        assert calls == [("dequant_mxfp4", (64, 512))]
        y = ops.linear_w4(x[:32].view(4, 8, 1024), wq, sc)
    assert calls[1:] == [("linear_w4", (32, 1024))] and y.shape == (4, 8, 64)


# ---- GPU: the decoder ----------------------------------------------------

PROMPT_LENS, STEPS = (5, 16, 35), 8


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
def test_decoder_mxfp4_weights_eager_graph_and_twin():
    """The yardstick is the bf16 decoder's own distance from LlamaModel's
    full forward on the twin; test_linear_w8.py established the factor 2.
    Measured values: PERFORMANCE.md, "MXFP4 weight-only decode"."""
    torch.manual_seed(3)
    vocab = CONFIGS["llama-tiny"].vocab_size
    model = LlamaModel(CONFIGS["llama-tiny"]).to(_dev()).eval()
    twin = copy.deepcopy(model)
    llama.quantize_linears_mxfp4(model)
    for name, mod in model.named_modules():
        assert not isinstance(mod, torch.nn.Linear)
        if isinstance(mod, ops.LinearW4):
            twin.get_submodule(name).weight.data.copy_(
                ops.dequantize_mxfp4(mod.wq, mod.scales, torch.bfloat16))
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
    print(f"mxfp4 decoder vs bf16 twin {err:.4e}; bf16 decoder vs forward "
          f"{yardstick:.4e}")
    assert err <= 2 * yardstick
