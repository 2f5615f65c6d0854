"""W4A16 GEMM for 33+ rows (csrc/hip/linear_w4_gemm.hip): the kernel against
the fp64 reference, exact conversion, determinism, the dispatch of
ops.linear_w4 and a PagedDecoder of 40 slots with MXFP4 weights."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from ray_amd import ops
from ray_amd.llm.paged import PagedDecoder
from ray_amd.models import llama
from ray_amd.models.llama import CONFIGS, LlamaModel

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """x, wq, scales as slices of buffers whose neighbouring rows are NaN
    (x) and 0xFF bytes, the fp64 reference and the bound: one bf16 rounding
    plus fp32 accumulation, whatever the split of K."""
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


# 33: one past the skinny kernel; 64: a full low tile; 65: one row into the
# high tile; 129: one row into a second row tile. K of one step (forced
# splits leave slices empty), of 8 and of 17 (uneven slices); one, two and
# three column tiles.
@pytest.mark.parametrize("split", [0, 1, 4])
@pytest.mark.parametrize("N,K", [(128, 128), (256, 1024), (384, 2176)])
@pytest.mark.parametrize("M", [33, 64, 65, 129])
def test_kernel_against_fp64_reference(M, N, K, split):
    x, wq, sc, ref, bound = _case(M, N, K)
    with torch.no_grad():
        y = ops._K.linear_w4_gemm(x, wq, sc, split=split)
        # the result does not depend on the rows tile
        for rt in (64, 128):
            assert torch.equal(
                y.view(torch.int16),
                ops._K.linear_w4_gemm(x, wq, sc, split=split,
                                      rows_tile=rt).view(torch.int16))
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    y = y.double().cpu()
    assert torch.isfinite(y).all()
    assert ((y - ref).abs() <= bound).all(), ((y - ref).abs() - bound).max()


def test_kernel_converts_every_nibble_exactly():
    """x is the identity, so y is the dequantised weight transposed: every
    nibble value at every k of a step, the edge scale codes in every lane
    group. -0 (nibble 8) leaves an fp32 sum as +0, so values are compared,
    as torch.equal does."""
    codes = [2, 126, 127, 128, 252]
    n, k = torch.arange(128)[:, None], torch.arange(128)[None, :]
    nib = ((n + k) % 16).to(torch.uint8).view(-1, 64, 2)
    wq = nib[..., 0] | (nib[..., 1] << 4)
    sc = torch.tensor(codes, dtype=torch.uint8)[
        (n // 16 + torch.arange(4)[None, :]) % len(codes)]
    x = torch.eye(128, dtype=torch.bfloat16)
    want = ops.dequantize_mxfp4(wq, sc, torch.bfloat16).t()
    assert torch.isfinite(want).all()
    with torch.no_grad():
        y = ops._K.linear_w4_gemm(x.to(_dev()), wq.to(_dev()), sc.to(_dev()))
    assert torch.equal(y.cpu(), want.contiguous())


def test_deterministic_and_split_workspace_under_graph_capture():
    """Two eager calls are bit-equal; the fp32 partials are allocated inside
    the captured region: several replays on fresh inputs against eager."""
    x, wq, sc, _, _ = _case(129, 384, 2176)
    xs = x.clone()
    with torch.no_grad():
        a = ops._K.linear_w4_gemm(x, wq, sc)
        assert torch.equal(a.view(torch.int16),
                           ops._K.linear_w4_gemm(x, wq, sc).view(torch.int16))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops._K.linear_w4_gemm(xs, wq, sc, split=4)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = ops._K.linear_w4_gemm(xs, wq, sc, split=4)
        for k in (1.0, -0.5, 2.0):
            xs.copy_(x * k)
            graph.replay()
            assert torch.equal(y, ops._K.linear_w4_gemm(xs, wq, sc, split=4))


def test_dispatch(monkeypatch):
    calls = []
    names = {"linear_w4": "skinny", "linear_w4_gemm": "gemm",
             "dequant_mxfp4": "fallback"}

    class Spy:
        def __getattr__(self, name):
            if name in names:
                return lambda *a: (calls.append((names[name], a[0].shape[0])),
                                   getattr(real, name)(*a))[1]
            return getattr(real, name)

    real = ops._K
    monkeypatch.setattr(ops, "_K", Spy())
    g = torch.Generator().manual_seed(5)
    wq, sc = (t.to(_dev()) for t in ops.quantize_weight_mxfp4(
        torch.randn(256, 1024, generator=g)))
    x = torch.randn(200, 1024, generator=g).bfloat16().to(_dev())

    def route(rows, wq=wq, sc=sc):
        del calls[:]
        y = ops.linear_w4(x[:rows], wq, sc)
        fb = F.linear(x[:rows], ops.dequantize_mxfp4(wq, sc, torch.bfloat16))
        return calls[0][0] if calls else "torch", torch.equal(y, fb)

    with torch.no_grad():
        assert (256, 1024) not in ops._W4_GEMM_TABLE
        assert route(33) == ("fallback", True)
        monkeypatch.setitem(ops._W4_GEMM_TABLE, (256, 1024), 128)
        assert [route(r)[0] for r in (32, 33, 128, 129)] == [
            "skinny", "gemm", "gemm", "fallback"]
        with torch.enable_grad():
            assert route(33) == ("torch", True)
        monkeypatch.delitem(ops._W4_GEMM_TABLE, (256, 1024))
        monkeypatch.setattr(ops, "_W4_GEMM_FORCE", True)
        assert route(200)[0] == "gemm" and calls == [("gemm", 200)]
        assert route(200, wq[:64], sc[:64]) == ("fallback", True)


# ---- the decoder ---------------------------------------------------------

PROMPT_LENS, STEPS = (35, 70) + (3, 9) * 19, 4


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
    """Prefills of 35 and 70 rows and decode steps of 40 rows all on the
    kernel. The yardstick is the bf16 decoder's own distance from
    LlamaModel's full forward on the twin (as in test_linear_w4.py).
    Measured values: PERFORMANCE.md, "W4A16 GEMM for 33+ rows"."""
    monkeypatch.setattr(ops, "_W4_GEMM_FORCE", True)
    torch.manual_seed(3)
    vocab = CONFIGS["llama-tiny"].vocab_size
    model = LlamaModel(CONFIGS["llama-tiny"]).to(_dev()).eval()
    twin = copy.deepcopy(model)
    llama.quantize_linears_mxfp4(model)
    for name, mod in model.named_modules():
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
