"""W8A16 GEMM for 33+ rows (csrc/hip/linear_w8_gemm.hip): the kernel against
the fp64 reference, exact conversion, determinism, the dispatch of
ops.linear_w8 and a PagedDecoder of 40 slots with fp8 weights."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from ray_amd import ops
from ray_amd.llm.paged import PagedDecoder
from ray_amd.models import llama
from ray_amd.models.llama import CONFIGS, LlamaModel

FP8 = torch.float8_e4m3fn
pytestmark = pytest.mark.gpu


def _dequant(wq, scale, dtype=torch.float32):
    return (wq.float() * scale[:, None]).to(dtype)


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """x, wq, scale as slices of buffers whose neighbouring rows are NaN
    (bf16, fp32) and 0x7F bytes, the fp64 reference and the bound: one bf16
    rounding plus fp32 accumulation, whatever the split of K."""
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


# 33: one past the skinny kernel; 64: a full tile; 65: one row into the
# 128-row tile; 129: one row into a second row tile. One column tile and
# three; K of two steps (split 4 leaves slices empty) and of 34 (uneven).
@pytest.mark.parametrize("split", [0, 1, 4])
@pytest.mark.parametrize("N,K", [(128, 128), (256, 1024), (384, 2176)])
@pytest.mark.parametrize("M", [33, 64, 65, 129])
def test_kernel_against_fp64_reference(M, N, K, split):
    x, wq, scale, ref, bound = _case(M, N, K)
    with torch.no_grad():
        y = ops._K.linear_w8_gemm(x, wq, scale, split=split)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    y = y.double().cpu()
    assert torch.isfinite(y).all()
    assert ((y - ref).abs() <= bound).all(), ((y - ref).abs() - bound).max()


def test_kernel_converts_every_byte_exactly():
    n, k = torch.arange(256)[:, None], torch.arange(128)[None, :]
    b = ((n + k) % 256).to(torch.uint8)
    b[(b & 0x7F) == 0x7F] = 0
    wq = b.view(FP8)
    scale = torch.tensor([0.5, 2.0]).repeat(128)
    x = torch.zeros(64, 128, dtype=torch.bfloat16)
    x[torch.arange(64), 2 * torch.arange(64)] = 1
    assert set(b[:, ::2].flatten().tolist()) == set(range(256)) - {0x7F, 0xFF}
    want = (wq.float()[:, ::2] * scale[:, None]).bfloat16().t()
    with torch.no_grad():
        y = ops._K.linear_w8_gemm(x.to(_dev()), wq.to(_dev()),
                                  scale.to(_dev()))
    assert torch.equal(y.cpu(), want.contiguous())


def test_kernel_is_deterministic():
    x, wq, scale, _, _ = _case(129, 384, 2176)
    with torch.no_grad():
        a = ops._K.linear_w8_gemm(x, wq, scale)
        b = ops._K.linear_w8_gemm(x, wq, scale)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_split_workspace_under_graph_capture():
    """The fp32 partials are allocated inside the captured region: several
    replays on fresh inputs against the eager result."""
    x, wq, scale, _, _ = _case(129, 384, 2176)
    xs = x.clone()
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops._K.linear_w8_gemm(xs, wq, scale, split=4)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = ops._K.linear_w8_gemm(xs, wq, scale, split=4)
        for k in (1.0, -0.5, 2.0):
            xs.copy_(x * k)
            graph.replay()
            assert torch.equal(y, ops._K.linear_w8_gemm(xs, wq, scale,
                                                         split=4))


def test_dispatch(monkeypatch):
    calls = []

    class Spy:
        def linear_w8(self, *a):
            calls.append(("skinny", a[0].shape[0]))
            return real.linear_w8(*a)

        def linear_w8_gemm(self, *a):
            calls.append(("gemm", a[0].shape[0]))
            return real.linear_w8_gemm(*a)

        def __getattr__(self, name):
            return getattr(real, name)

    real = ops._K
    monkeypatch.setattr(ops, "_K", Spy())
    g = torch.Generator().manual_seed(5)
    wq, scale = (t.to(_dev()) for t in ops.quantize_weight_fp8(
        torch.randn(256, 1024, generator=g)))
    x = torch.randn(200, 1024, generator=g).bfloat16().to(_dev())

    def route(rows):
        del calls[:]
        y = ops.linear_w8(x[:rows], wq, scale)
        fb = F.linear(x[:rows], _dequant(wq, scale, torch.bfloat16))
        return calls[0][0] if calls else "fallback", torch.equal(y, fb)

    with torch.no_grad():
        assert (256, 1024) not in ops._W8_GEMM_TABLE
        assert route(33) == ("fallback", True)
        monkeypatch.setitem(ops._W8_GEMM_TABLE, (256, 1024), 128)
        assert [route(r)[0] for r in (32, 33, 128, 129)] == [
            "skinny", "gemm", "gemm", "fallback"]
        with torch.enable_grad():
            assert route(33) == ("fallback", True)
        monkeypatch.delitem(ops._W8_GEMM_TABLE, (256, 1024))
        monkeypatch.setattr(ops, "_W8_GEMM_FORCE", True)
        assert route(200)[0] == "gemm" and calls == [("gemm", 200)]


# ---- the decoder ---------------------------------------------------------

PROMPT_LENS, STEPS = (35, 70) + (3, 9) * 19, 4
# Max abs logit distance allowed between the fp8-weight decoder (every
# linear of 33+ rows on the kernel) and the bf16 decoder of a twin model
# holding (wq * scale).bfloat16(): twice what the bf16 PagedDecoder sits
# from LlamaModel's full-sequence forward on the same twin, prompts and
# steps. Measured on an MI355X: 8.3008e-3 for that yardstick (printed
# below), 1.3672e-2 for the fp8 decoder.
DECODER_TOL = 2 * 8.3008e-3


@torch.no_grad()
def _decode(model, prompts, fed, capture):
    dec = PagedDecoder(model, len(prompts), 96, _dev())
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


@torch.no_grad()
def test_decoder_40_rows_eager_graph_and_twin(monkeypatch):
    monkeypatch.setattr(ops, "_W8_GEMM_FORCE", True)
    torch.manual_seed(3)
    vocab = CONFIGS["llama-tiny"].vocab_size
    model = LlamaModel(CONFIGS["llama-tiny"]).to(_dev()).eval()
    twin = copy.deepcopy(model)
    llama.quantize_linears_fp8(model)
    for name, mod in model.named_modules():
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
