"""ops.sample: the reference rules on hand-made rows, the HIP kernel against
the fp64 reference, determinism and graph capture, and the engines' top_k /
top_p / seed / device_sampling."""
import math

import pytest
import torch

from ray_amd import ops
from ray_amd.llm import ContinuousBatchingEngine, LLMConfig, LLMEngine

NEG = float("-inf")
U_MAX = 1.0 - 2.0 ** -24
FP32_GRID = 0.11


@pytest.mark.parametrize("x, T, k, p, u, token, kept", [
    # ties at the top-k threshold are all kept: k = 2 keeps 3, 2, 2
    ([1.0, 2.0, 3.0, 2.0, 0.0], 1.0, 2, 1.0, U_MAX, 3, 3),
    # ties at the top-p threshold: masses 4 : 2 : 2 : 1, 0.5 < 0.6 <= 8/9
    ([math.log(2), math.log(4), math.log(2), 0.0], 1.0, 0, 0.6, U_MAX, 2, 3),
    # top_p = 0 keeps the argmax set, both holders of the maximum
    ([0.0, 5.0, 1.0, 5.0], 1.0, 0, 0.0, 0.75, 3, 2),
    # top_k >= V is off
    ([0.0, 1.0, 2.0], 1.0, 3, 1.0, 0.0, 0, 3),
    # -inf is kept by no filter's count but never returned
    ([NEG, 0.0, NEG, 0.0, NEG], 1.0, 0, 1.0, 0.0, 1, 5),
    ([NEG, 0.0, NEG, 0.0, NEG], 1.0, 0, 1.0, U_MAX, 3, 5),
    # a greedy tie gives the lowest index; the other parameters are ignored
    ([1.0, 7.0, 7.0, 2.0], 0.0, 1, 0.1, 0.9, 1, 1),
    # u = 0 and u just below 1 give the first and the last kept token
    ([0.0, 3.0, 1.0, 3.0, 2.0], 2.0, 3, 1.0, 0.0, 1, 3),
    ([0.0, 3.0, 1.0, 3.0, 2.0], 2.0, 3, 1.0, U_MAX, 4, 3),
])
def test_reference_rules(x, T, k, p, u, token, kept):
    tok, n = ops.sample(torch.tensor([x]), T, k, p, u, return_kept=True)
    assert (tok.dtype, n.dtype) == (torch.int64, torch.int32)
    assert (int(tok), int(n)) == (token, kept)


PARAMS = [(0.0, 0, 1.0), (1.0, 0, 1.0), (0.7, 0, 1.0), (1.0, 50, 1.0),
          (1.0, 0, 0.9), (0.8, 40, 0.95), (1.5, 0, 0.5), "mixed"]
# "mixed": per-row parameters, greedy next to sampled rows
MIXED = [(0.0, 0, 1.0), (0.8, 40, 0.95), (1.0, 50, 1.0), (0.0, 5, 0.5),
         (1.5, 0, 0.5), (0.7, 0, 1.0)]
# (V, B, dtype); 140003 bf16 does not fit the registers and re-reads the row
SHAPES = [(V, B, dt) for V in (1, 7, 513, 1000, 128256) for B in (1, 3)
          for dt in (torch.bfloat16, torch.float32)]
SHAPES.append((140003, 1, torch.bfloat16))


@pytest.mark.gpu
@pytest.mark.parametrize("params", PARAMS, ids=str)
@pytest.mark.parametrize("V, B, dtype", SHAPES, ids=str)
def test_kernel_matches_reference(V, B, dtype, params):
    """64 draws per logits row, as batch rows over the same logits (B = 1:
    row stride 0; B = 3: rows of a [192, V + 8] buffer, so for most V the
    row starts are not 16-byte aligned).

    eps. The kernel's p_i is v_exp_f32(a_i), a_i = fl((x_i - max) * s) with
    s = fl(log2 e / T): a_i carries two roundings, |a_i| * 2^-23 in all, so
    p_i is off by a factor within 1 +- (|a_i| * 2^-23 * ln 2 + 2^-22), the
    last term for v_exp_f32 itself. Terms with |a_i| <= 32 are off by at
    most 2^-18 relative; beyond that p_i < 2^-32 and p_i * |a_i| is
    smaller still. The fixed point adds at most 2^-41 per term, 2^-24 * Z
    over 128k terms. A partial sum, and Z, are therefore within 2^-17 * Z
    of the fp64 values, inside the 2^-16 * Z the check was specified with;
    eps is twice that, 2^-15 * Z."""
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(4)
    base = torch.randn(B, V, generator=g) * 4
    if dtype == torch.float32:
        # distinct fp32 logits of a flat row are 1e-5 of the mass apart, so
        # no top-p threshold can be 4 eps from its neighbours: put them on
        # a grid whose points use every mantissa bit, which gives ties
        base = torch.round(base / FP32_GRID) * FP32_GRID
    base = base.to(dtype).to(dev)
    n_u = 64
    if B == 1:
        logits = base.expand(n_u, V)
    else:
        buf = torch.empty(B * n_u, V + 8, dtype=dtype, device=dev)
        logits = buf[:, :V]
        logits.copy_(base.repeat(n_u, 1))
    rows = B * n_u
    # row i has the logits of row i % B and the parameters of row i % period
    period = len(MIXED) if params == "mixed" else B
    per_row = [MIXED[i % period] if params == "mixed" else params
               for i in range(rows)]
    T = torch.tensor([q[0] for q in per_row], device=dev)
    k = torch.tensor([q[1] for q in per_row], dtype=torch.int32, device=dev)
    p = torch.tensor([q[2] for q in per_row], device=dev)
    u = torch.rand(rows, generator=g).clamp(max=U_MAX).to(dev)

    tok, kept = ops.sample(logits, T, k, p, u, return_kept=True)
    assert tok.shape == (rows,) and tok.dtype == torch.int64
    rtok, rkept = ops.sample_ref(logits[:period], T[:period], k[:period],
                                 p[:period], u[:period], return_kept=True)

    unique = total = 0
    for j in range(period):
        Tj, kj, pj = per_row[j]
        mine = torch.arange(j, rows, period, device=dev)
        t = tok[mine]
        if Tj <= 0:
            assert bool((t == rtok[j]).all()) and bool((kept[mine] == 1).all())
            continue
        x = logits[j].double()
        xs = torch.sort(x, descending=True).values
        keep = x >= xs[int(rkept[j]) - 1]
        assert int(keep.sum()) == int(rkept[j])
        w = torch.where(keep, torch.exp((x - xs[0]) / Tj), 0.0)
        Z = float(w.sum())
        eps = 2.0 ** -15 * Z
        if pj < 1:
            # the threshold mass is 4 eps away from top_p * Z1 on both sides
            k_keep = x >= xs[kj - 1] if 0 < kj < V else torch.ones_like(keep)
            Z1 = float(torch.exp((x[k_keep] - xs[0]) / Tj).sum())
            above = float(w[x > xs[int(rkept[j]) - 1]].sum())
            print("top-p margins / Z1", (Z - pj * Z1) / Z1,
                  (pj * Z1 - above) / Z1)
            assert Z - pj * Z1 >= 4 * 2.0 ** -15 * Z1
            assert above == 0 or pj * Z1 - above >= 4 * 2.0 ** -15 * Z1
        assert bool((kept[mine] == rkept[j]).all()), (kept[mine], rkept[j])
        assert bool(keep[t].all()), t
        cdf = torch.cat([w.new_zeros(1), torch.cumsum(w, 0)])
        target = u[mine].double() * Z
        dev_z = torch.maximum(cdf[t] - target, target - cdf[t + 1]) / Z
        print("largest deviation / Z", float(dev_z.max()))
        assert bool((dev_z <= 2.0 ** -15).all()), (t, dev_z)
        # draws with exactly one acceptable token
        ck = cdf[1:][keep]
        ck0 = torch.cat([ck.new_zeros(1), ck[:-1]])
        ok = ((ck0[None] - eps <= target[:, None])
              & (target[:, None] <= ck[None] + eps)).sum(1)
        unique += int((ok == 1).sum())
        total += mine.numel()
    if total:
        print("unique share", unique / total)
        assert unique >= 0.75 * total


@pytest.mark.gpu
def test_kernel_deterministic_and_capturable():
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(8, 128256, generator=g) * 4).bfloat16().to(dev)
    T = torch.full((8,), 0.8, device=dev)
    k = torch.tensor([0, 40] * 4, dtype=torch.int32, device=dev)
    p = torch.tensor([0.9, 0.9, 1.0, 1.0] * 2, device=dev)
    u = torch.rand(8, generator=g).to(dev)
    first = ops.sample(logits, T, k, p, u)
    assert torch.equal(first, ops.sample(logits, T, k, p, u))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.sample(logits, T, k, p, u)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.sample(logits, T, k, p, u)
    # other inputs, written in place, then several replays
    u.copy_(torch.rand(8, generator=g))
    T.copy_(torch.tensor([1.3, 0.0] * 4))
    eager = ops.sample(logits, T, k, p, u)
    assert not torch.equal(eager, first)
    for _ in range(3):
        graph.replay()
        assert torch.equal(out, eager)


def _run(engine_cls, requests, **cfg):
    eng = engine_cls(LLMConfig(model_id="llama-tiny", max_seq_len=96, **cfg))
    if engine_cls is LLMEngine:
        return [eng.generate(**r)["token_ids"] for r in requests]
    ids = [eng.submit(**r) for r in requests]
    done = eng.run_until_complete()
    return [done[i] for i in ids]


SEEDED = dict(prompt_ids=[3, 1, 4, 1, 5], max_new_tokens=10, temperature=0.9,
              top_k=20, top_p=0.9, seed=7)
OTHERS = [dict(prompt_ids=[9, 8, 7], max_new_tokens=12, temperature=1.0,
               top_p=0.8),
          dict(prompt_ids=list(range(20, 31)), max_new_tokens=6)]


@pytest.mark.parametrize("kv_cache", ["contiguous", "paged"])
def test_engine_seed_and_filters(kv_cache):
    cfg = dict(max_batch_size=3, use_hip_graph=False, kv_cache=kv_cache)
    alone = _run(ContinuousBatchingEngine, [SEEDED], **cfg)[0]
    assert len(alone) == 10
    # the same seed gives the same tokens inside a batch of other requests
    batch = _run(ContinuousBatchingEngine, OTHERS[:1] + [SEEDED] + OTHERS[1:],
                 **cfg)
    assert batch[1] == alone
    single = _run(LLMEngine, [SEEDED, SEEDED], use_hip_graph=False)
    assert single[0] == single[1] and len(single[0]) == 10
    # top_k = 1 leaves the maximum alone
    greedy = dict(prompt_ids=[2, 7, 1, 8], max_new_tokens=8)
    got = _run(ContinuousBatchingEngine,
               [greedy, dict(greedy, temperature=1.0, top_k=1)], **cfg)
    assert got[0] == got[1]


@pytest.mark.parametrize("bad", [dict(top_k=-1), dict(top_p=1.5),
                                 dict(top_p=-0.1)])
def test_engine_validation(bad):
    with pytest.raises(ValueError):
        LLMConfig(model_id="llama-tiny", **bad)
    eng = ContinuousBatchingEngine(LLMConfig(
        model_id="llama-tiny", max_seq_len=64, use_hip_graph=False))
    with pytest.raises(ValueError):
        eng.submit([1, 2, 3], **bad)


@pytest.mark.gpu
def test_engine_device_sampling():
    cfg = dict(max_batch_size=3, kv_cache="paged")
    greedy = [dict(prompt_ids=[2, 7, 1, 8], max_new_tokens=8),
              dict(prompt_ids=list(range(20, 31)), max_new_tokens=6)]
    requests = greedy + [SEEDED]
    host = _run(ContinuousBatchingEngine, requests, use_hip_graph=True, **cfg)
    graph = _run(ContinuousBatchingEngine, requests, use_hip_graph=True,
                 device_sampling=True, **cfg)
    eager = _run(ContinuousBatchingEngine, requests, use_hip_graph=False,
                 device_sampling=True, **cfg)
    # greedy: argmax on the host and in the kernel agree (no tie at the
    # maximum on these prompts); seeded: the same tokens on every path
    assert graph == host
    assert eager[2] == graph[2]
