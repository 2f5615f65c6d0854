"""Exact key-inclusion probes for the forward and paged attention kernels
(csrc/hip/{flash_attn_v7,flash_attn_v5,paged_attn,paged_attn_prefill}.hip).

Attention is permutation-invariant over (K, V) row pairs, so a forward kernel
can be wrong in three ways only: which keys a query row includes, which V row
goes with which K row, and arithmetic precision. With randn inputs a softmax
row spreads over many keys and one wrong key moves the output by about 1/N of
a value row, far below the project's 4e-2 tolerance once a row sees a few
hundred keys. The three probes here make a single wrong key an exact integer
miscount or an O(1) error:

counting (q = 0)
    Every score is 0, so every allowed key has P = 1 (exact in bf16; fp32 sums
    of ones are exact). V[j, d] = 1 if (j + 7 h) % D == d for key j of kv head
    h. For a row that may see the key set A: |exp(lse) - |A|| <= 0.25 and
    |out[d] |A| - #{j in A : bucket(j) == d}| <= 0.25. 0.25 is half the
    distance to a miscount, halved again; the bucket counts are at most 16
    here, so bf16 rounding of `out` contributes at most 16 * 2^-9. |A| and the
    counts come from the mask definition in this file, never from a kernel.
    For split decode the fp32 partials in the workspace are checked as sums:
    l over the non-empty splits is seq_len and o is v_scale * count, both
    exactly; m is 0 in a non-empty split and -inf in an empty one. How tokens
    are dealt to splits is the kernel's business and is not asserted.

needle (one key dominates)
    K, V randn; query row i is 4 k[target(i)] (exact in bf16), so the target
    scores 4 |k|^2 / sqrt(D) (about 45 at D = 128, 32 at D = 64) against a
    standard deviation of 4 for every other key. Allowed needle: the target is
    the last key the row may see, the fp64 reference is v[target], and a
    kernel that drops it is off by O(|v|). Forbidden needle: the target is
    the first key the row must not see (for the paged kernels a finite token
    at seq_len or ctx + q_len, in a tail slot or in the next page); a kernel
    that admits it returns v[target]. Compared with the fp64 reference at the
    project's 4e-2 atol and rtol: the power comes from the inputs.
    A running maximum taken before the mask is a different matter. At factor
    4 the masked needle sits about 30 nats above the allowed keys, P stays a
    normal fp32 number and the result is still right (measured on the
    defective fp32 reference below: no row lost). So there is a third kind,
    "strong": a forbidden needle at factor 16 (score about 180 at D = 128,
    standard deviation 16 for the rest), far enough above that every P
    underflows and such a kernel returns NaN.

precision (randn inputs)
    `_emulate` is the kernels' arithmetic in torch: fp32 softmax, P rounded to
    bf16, P.V in fp32, division by the fp32 row sum, output rounded to bf16.
    With e = ||x - ref64|| / ||ref64||, a kernel must have
    e_kernel <= 2 e_emul. The factor 2 is headroom for summation order, the
    hardware exp2 and deferred-max rescaling, none of which adds a rounding
    step. Both numbers are printed. Measured on an MI355X (kernel /
    emulation; profiles/attention_probes_tests.log has every line):
      flash v7 causal (2,8,2,512)   2.04e-3 / 1.98e-3
      flash T 256 Tk 300            2.31e-3 / 2.21e-3
      flash v5 T 384 causal         2.02e-3 / 1.97e-3
      decode (1000, 33), bf16       1.66e-3 / 1.91e-3   (fp32 P, splits 1, 8)
      decode (1000, 33), fp8        1.68e-3 / 2.04e-3
      prefill (100, 130) bf16, fp8  2.28e-3 / 2.17e-3, 2.31e-3 / 2.18e-3

The CPU tests at the top feed the three checkers the output of deliberately
defective fp64 references and assert that they are rejected, and that the
honest references pass.

All inputs are drawn on the CPU from seeded generators. Paged caches are NaN
(bf16) or 0x7F bytes (fp8) everywhere outside the rows a case writes.
"""
import functools
import math
import zlib

import pytest
import torch

from ray_amd import ops

PAGE = 16
FP8 = torch.float8_e4m3fn
NAN_BYTE = 0x7F
TOL = 4e-2          # the project's forward tolerance, atol = rtol
COUNT_CAP = 0.25    # half the distance to a miscount, halved again
NEEDLE_CAP = 1e-3   # honest allowed-needle reference against v[target]
SCALES = {"bf16": (1.0, 1.0), "fp8": (0.5, 2.0)}   # (k_scale, v_scale)
HEADS = [(4, 4), (8, 2), (8, 1)]
# query = factor * k[target], exact in bf16. "strong" is a forbidden needle
# whose score is past fp32's exponent range above every allowed key.
NEEDLE_FACTOR = {"allowed": 4, "forbidden": 4, "strong": 16}
FORBIDDEN = ("forbidden", "strong")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if not ops.HAVE_HIP_OPS:
        raise RuntimeError("HIP extension not built")
    return torch.device("cuda", 0)


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


# --------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------


def _attend64(q, k, v, mask, premask_max=False, dtype=torch.float64):
    """fp64 attention under an explicit mask. q [..., R, D]; k, v [..., N, D]
    with one row set per query head; mask [..., R, N], True = allowed.
    Returns out [..., R, D] and lse [..., R]; a row that may see nothing is
    zeros and -inf. premask_max is a defect for the self-tests: the maximum
    is taken over the unmasked scores (with dtype fp32, the exponent range a
    kernel has)."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    sm = s.masked_fill(~mask, float("-inf"))
    m = (s if premask_max else sm).amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(sm - m)
    l = p.sum(-1, keepdim=True)
    out = (p @ v) / l
    out = torch.where(mask.any(-1, keepdim=True), out, torch.zeros_like(out))
    return out, (m + l.log()).squeeze(-1)


def _emulate(q, k, v, mask, round_scores=False):
    """The kernels' two roundings in torch: fp32 softmax, P rounded to bf16,
    P.V in fp32, division by the fp32 row sum, output rounded to bf16.
    round_scores is a defect for the self-tests: scores rounded to bf16."""
    s = (q.float() @ k.float().transpose(-1, -2)) * (
        1.0 / math.sqrt(q.shape[-1]))
    if round_scores:
        s = s.bfloat16().float()
    s = s.masked_fill(~mask, float("-inf"))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    return ((p.bfloat16().float() @ v.float()) / l).bfloat16()


def _flash_mask(T, Tk, causal, q_offset=0):
    """Keys query row i of flash_attention may see: j < Tk, and under
    `causal` j <= i + q_offset."""
    i = torch.arange(T).view(T, 1)
    j = torch.arange(Tk).view(1, Tk)
    return (j <= i + q_offset) if causal else (j < Tk).expand(T, Tk)


def _onehot_v(Hkv, N, D):
    """V[h, j, d] = 1 if (j + 7 h) % D == d: key j of kv head h falls into
    bucket (j + 7 h) % D."""
    h = torch.arange(Hkv).view(Hkv, 1, 1)
    j = torch.arange(N).view(1, N, 1)
    d = torch.arange(D).view(1, 1, D)
    return ((j + 7 * h) % D == d).float()


def _expected_counts(mask, Hq, Hkv, D):
    """mask [R, N] -> |A| [R] and the bucket counts [Hq, R, D] of the keys
    each row may see."""
    cnt = mask.double() @ _onehot_v(Hkv, mask.shape[-1], D).double()
    return mask.sum(-1), cnt.repeat_interleave(Hq // Hkv, dim=0)


# --------------------------------------------------------------------------
# checkers
# --------------------------------------------------------------------------


def check_count(out, lse, n, cnt, v_scale=1.0, tag=""):
    """Counting probe. out [..., D]; lse [...] or None; n [...] = |A|;
    cnt [..., D] bucket counts. Rows with |A| = 0 must be exactly zero."""
    out, n, cnt = out.double(), n.double(), cnt.double()
    assert out.shape == cnt.shape and n.shape == out.shape[:-1], tag
    assert torch.isfinite(out).all(), f"{tag}: out not finite"
    assert (out[n == 0] == 0).all(), f"{tag}: empty row not zero"
    e_out = float((out * n.unsqueeze(-1) - v_scale * cnt).abs().max())
    if lse is None:
        print(f"{tag}: max |out |A| - count| {e_out:.3e}")
    else:
        assert lse.shape == n.shape and bool((n > 0).all()), tag
        assert torch.isfinite(lse).all(), f"{tag}: lse not finite"
        e_lse = float((lse.double().exp() - n).abs().max())
        print(f"{tag}: max |out |A| - count| {e_out:.3e}, "
              f"max |exp(lse) - |A|| {e_lse:.3e}")
        assert e_lse <= COUNT_CAP, f"{tag}: lse miscounts by {e_lse}"
    assert e_out <= COUNT_CAP, f"{tag}: out miscounts by {e_out}"


def check_needle(out, ref, tag=""):
    """Needle probe: out against the fp64 reference at the project's
    tolerance."""
    out, ref = out.double(), ref.double()
    assert out.shape == ref.shape, (tag, out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{tag}: out not finite"
    err = float((out - ref).abs().max())
    print(f"{tag}: max |out - ref| {err:.3e}")
    assert torch.allclose(out, ref, atol=TOL, rtol=TOL), f"{tag}: {err}"


def check_precision(out, emul, ref, tag=""):
    """e_kernel <= 2 e_emul, relative L2 against the fp64 reference."""
    ref = ref.double()
    assert out.shape == ref.shape == emul.shape, tag
    assert torch.isfinite(out).all(), f"{tag}: out not finite"
    e_k = float((out.double() - ref).norm() / ref.norm())
    e_e = float((emul.double() - ref).norm() / ref.norm())
    print(f"{tag}: e_kernel {e_k:.3e} e_emul {e_e:.3e}")
    assert e_k <= 2 * e_e, f"{tag}: kernel {e_k} emulation {e_e}"


def _old_check(out, ref):
    """What the suite did before: bf16 output against an fp32 reference."""
    return torch.allclose(out.bfloat16().float(), ref.float(), atol=TOL,
                          rtol=TOL)


# --------------------------------------------------------------------------
# dense (flash_attention) cases
# --------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _flash_case(kind, B, Hq, Hkv, T, Tk, causal, q_offset=0, D=128):
    """bf16 q [B,Hq,T,D], k, v [B,Hkv,Tk,D] and what the probe `kind`
    expects. kind: "count", "allowed", "forbidden", "strong" or "randn"."""
    g = _gen("flash", kind, B, Hq, Hkv, T, Tk, causal, q_offset, D)
    rep = Hq // Hkv
    mask = _flash_mask(T, Tk, causal, q_offset)
    assert bool(mask.any(-1).all())
    k = torch.randn(B, Hkv, Tk, D, generator=g).bfloat16()
    c = dict(k=k, mask=mask, causal=causal, q_offset=q_offset)
    if kind == "count":
        c["q"] = torch.zeros(B, Hq, T, D, dtype=torch.bfloat16)
        c["v"] = _onehot_v(Hkv, Tk, D).expand(B, Hkv, Tk, D).bfloat16()
        n, cnt = _expected_counts(mask, Hq, Hkv, D)
        c["n"] = n.expand(B, Hq, T)
        c["cnt"] = cnt.expand(B, Hq, T, D)
        return c
    c["v"] = torch.randn(B, Hkv, Tk, D, generator=g).bfloat16()
    kr = k.repeat_interleave(rep, dim=1)
    if kind == "randn":
        c["q"] = torch.randn(B, Hq, T, D, generator=g).bfloat16()
    else:
        last = torch.arange(T) + q_offset if causal else torch.full((T,),
                                                                     Tk - 1)
        if kind == "allowed":
            tgt = last
        else:
            # a row whose first forbidden key lies outside the tensor keeps
            # its allowed needle
            assert kind in FORBIDDEN and causal
            tgt = torch.where(last + 1 < Tk, last + 1, last)
            assert int((tgt > last).sum()) >= T - 1
        assert int(tgt.min()) >= 0 and int(tgt.max()) < Tk
        c["q"] = NEEDLE_FACTOR[kind] * kr[:, :, tgt]
        c["tgt"] = tgt
    c["kr"], c["vr"] = kr, c["v"].repeat_interleave(rep, dim=1)
    c["ref"], c["ref_lse"] = _attend64(c["q"], kr, c["vr"], mask)
    if kind == "randn":
        c["emul"] = _emulate(c["q"], kr, c["vr"], mask)
    return c


def _bthd(t):
    """The same values as a transpose view of [B,T,H,D] storage."""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def _packed(q, k, v):
    """q, k, v as the column sections of one packed [B,T,(Hq+2Hkv)*D]
    buffer."""
    B, Hq, T, D = q.shape
    Hkv = k.shape[1]
    qkv = torch.full((B, T, (Hq + 2 * Hkv) * D), float("nan"),
                     device=q.device, dtype=q.dtype)
    qs, ks, vs = ops._qkv_sections(qkv, Hq, Hkv)
    qs.copy_(q)
    ks.copy_(k)
    vs.copy_(v)
    return qs, ks, vs


def _run_flash(c, layout, dev):
    q, k, v = (c[x].to(dev) for x in "qkv")
    if layout == "bthd":
        q, k, v = _bthd(q), _bthd(k), _bthd(v)
        assert ops._is_bthd_view(q) and not q.is_contiguous()
    elif layout == "packed":
        q, k, v = _packed(q, k, v)
        assert ops._is_bthd_view(q, True) and q.stride(2) > q.shape[1] * 128
    else:
        assert layout == "bhtd"
    out, lse = ops.flash_attention(q, k, v, causal=c["causal"],
                                   q_offset=c["q_offset"], return_lse=True)
    assert out.dtype == torch.bfloat16 and out.shape == c["q"].shape
    return out.float().cpu(), lse.cpu()


# --------------------------------------------------------------------------
# paged cases
# --------------------------------------------------------------------------


def _store_as(x, fp8, scale):
    """x (fp32) as the elements a cache stores, and their fp32 values."""
    if fp8:
        s = ops.quantize_kv_fp8(x, scale)
        return s, s.float() * scale
    s = x.bfloat16()
    return s, s.float()


def _raw(t):
    """Bit view for exact copies of cache elements."""
    return t.view(torch.uint8 if t.dtype == FP8 else torch.int16)


def _pool(g, rows, Hkv, D, fp8):
    """K/V caches that are NaN everywhere (null page, spare pages, tail
    slots) except the given rows, and a block table that is a random
    permutation of pages 1.. with unused entries 0. rows: one (k, v) pair of
    stored elements [Hkv, n, D] per sequence."""
    pages = [-(-k.shape[1] // PAGE) for k, _ in rows]
    num_pages = 1 + sum(pages) + 3
    shape = (num_pages, Hkv, PAGE, D)
    if fp8:
        kc = torch.full(shape, NAN_BYTE, dtype=torch.uint8).view(FP8)
        vc = torch.full(shape, NAN_BYTE, dtype=torch.uint8).view(FP8)
    else:
        kc = torch.full(shape, float("nan"), dtype=torch.bfloat16)
        vc = torch.full(shape, float("nan"), dtype=torch.bfloat16)
    perm = (torch.randperm(num_pages - 1, generator=g) + 1).tolist()
    bt = torch.zeros(len(rows), max(1, max(pages)), dtype=torch.int32)
    for b, (kr, vr) in enumerate(rows):
        assert kr.dtype == kc.dtype and vr.dtype == vc.dtype
        for i in range(pages[b]):
            pg = perm.pop()
            bt[b, i] = pg
            r = min(PAGE, kr.shape[1] - i * PAGE)
            _raw(kc)[pg, :, :r] = _raw(kr)[:, i * PAGE:i * PAGE + r]
            _raw(vc)[pg, :, :r] = _raw(vr)[:, i * PAGE:i * PAGE + r]
    return kc, vc, bt


def _kv_rows(g, kind, n, Hkv, D, fmt):
    """Stored K/V rows [Hkv, n, D] of one sequence and their fp32 values.
    Counting V holds the codes 0 and 1 themselves, so its values are
    v_scale times the one-hot."""
    fp8 = fmt == "fp8"
    ks, vs = SCALES[fmt]
    k, kf = _store_as(torch.randn(Hkv, n, D, generator=g), fp8, ks)
    if kind == "count":
        onehot = _onehot_v(Hkv, n, D)
        v, vf = onehot.to(FP8 if fp8 else torch.bfloat16), onehot * vs
    else:
        v, vf = _store_as(torch.randn(Hkv, n, D, generator=g), fp8, vs)
    return k, v, kf, vf


@functools.lru_cache(maxsize=None)
def _decode_case(kind, D, Hq, Hkv, fmt, lens):
    """One decode batch. "forbidden" appends one finite token at position
    seq_len of every sequence (a tail slot, or slot 0 of one more page) and
    aims the query at it."""
    g = _gen("decode", kind, D, Hq, Hkv, fmt, lens)
    rep = Hq // Hkv
    B = len(lens)
    rows = []
    q = torch.zeros(B, Hq, D, dtype=torch.bfloat16)
    ref = torch.zeros(B, Hq, D, dtype=torch.float64)
    emul = torch.zeros(B, Hq, D, dtype=torch.bfloat16)
    for b, n in enumerate(lens):
        extra = 1 if kind in FORBIDDEN else 0
        k, v, kf, vf = _kv_rows(g, kind, n + extra, Hkv, D, fmt)
        rows.append((k, v))
        if kind == "count" or n == 0:
            continue
        kr = kf.repeat_interleave(rep, dim=0)
        vr = vf.repeat_interleave(rep, dim=0)
        if kind == "randn":
            q[b] = torch.randn(Hq, D, generator=g).bfloat16()
        else:
            qn = NEEDLE_FACTOR[kind] * kr[:, n - 1 + extra]
            q[b] = qn.bfloat16()
            assert torch.equal(q[b].float(), qn)
        mask = torch.ones(Hq, 1, n, dtype=torch.bool)
        qb = q[b].unsqueeze(1)
        ref[b] = _attend64(qb, kr[:, :n], vr[:, :n], mask)[0][:, 0]
        if kind == "randn":
            emul[b] = _emulate(qb, kr[:, :n], vr[:, :n], mask)[:, 0]
    kc, vc, bt = _pool(g, rows, Hkv, D, fmt == "fp8")
    c = dict(q=q, kc=kc, vc=vc, bt=bt, ref=ref, emul=emul, fmt=fmt,
             sl=torch.tensor(lens, dtype=torch.int32))
    if kind == "count":
        j = torch.arange(max(max(lens), 1)).view(1, -1)
        mask = j < torch.tensor(lens).view(B, 1)            # j < seq_len
        n, cnt = _expected_counts(mask, Hq, Hkv, D)
        c["n"] = n.view(B, 1).expand(B, Hq)
        c["cnt"] = cnt.transpose(0, 1)                      # [B, Hq, D]
    return c


def _run_decode(c, dev, splits, ws=None):
    ks, vs = SCALES[c["fmt"]]
    out = ops.paged_attention_decode(
        *(c[x].to(dev) for x in ("q", "kc", "vc", "bt", "sl")),
        num_splits=splits, workspace=ws, k_scale=ks, v_scale=vs)
    assert out.dtype == torch.bfloat16 and out.shape == c["q"].shape
    return out.float().cpu()


@functools.lru_cache(maxsize=None)
def _prefill_case(kind, D, Hq, Hkv, fmt, specs, Tq):
    """One prefill batch; specs is ((ctx, q_len), ...). Query row i of a
    sequence may see cache rows j <= ctx + i; rows i >= q_len give zeros.
    "forbidden" aims row i at key ctx + i + 1, which for the last row is one
    finite token appended at ctx + q_len. In the counting probe the query
    rows at or past q_len are NaN: the kernel must not read them."""
    g = _gen("prefill", kind, D, Hq, Hkv, fmt, specs, Tq)
    rep = Hq // Hkv
    B = len(specs)
    rows = []
    q = torch.randn(B, Tq, Hq, D, generator=g).bfloat16()
    if kind == "count":
        q.fill_(float("nan"))
    ref = torch.zeros(B, Tq, Hq, D, dtype=torch.float64)
    emul = torch.zeros(B, Tq, Hq, D, dtype=torch.bfloat16)
    n_all = torch.zeros(B, Tq, Hq)
    cnt_all = torch.zeros(B, Tq, Hq, D, dtype=torch.float64)
    for b, (ctx, ql) in enumerate(specs):
        assert ql <= Tq
        L = ctx + ql
        extra = 1 if kind in FORBIDDEN else 0
        k, v, kf, vf = _kv_rows(g, kind, L + extra, Hkv, D, fmt)
        rows.append((k, v))
        if ql == 0:
            continue
        i = torch.arange(ql).view(ql, 1)
        mask = torch.arange(L).view(1, L) <= ctx + i        # j <= ctx + i
        if kind == "count":
            q[b, :ql] = 0
            n, cnt = _expected_counts(mask, Hq, Hkv, D)
            n_all[b, :ql] = n.view(ql, 1)
            cnt_all[b, :ql] = cnt.transpose(0, 1)
            continue
        kr = kf.repeat_interleave(rep, dim=0)
        vr = vf.repeat_interleave(rep, dim=0)
        if kind != "randn":
            tgt = ctx + torch.arange(ql) + extra
            qn = NEEDLE_FACTOR[kind] * kr[:, tgt]            # [Hq, ql, D]
            q[b, :ql] = qn.transpose(0, 1).bfloat16()
            assert torch.equal(q[b, :ql].float(), qn.transpose(0, 1))
        qb = q[b, :ql].transpose(0, 1)
        ref[b, :ql] = _attend64(qb, kr[:, :L], vr[:, :L],
                                mask)[0].transpose(0, 1)
        if kind == "randn":
            emul[b, :ql] = _emulate(qb, kr[:, :L], vr[:, :L],
                                    mask).transpose(0, 1)
    kc, vc, bt = _pool(g, rows, Hkv, D, fmt == "fp8")
    return dict(q=q, kc=kc, vc=vc, bt=bt, ref=ref, emul=emul, fmt=fmt,
                n=n_all, cnt=cnt_all, specs=specs,
                ctx=torch.tensor([c for c, _ in specs], dtype=torch.int32),
                ql=torch.tensor([n for _, n in specs], dtype=torch.int32))


def _run_prefill(c, dev):
    ks, vs = SCALES[c["fmt"]]
    out = ops.paged_attention_prefill(
        *(c[x].to(dev) for x in ("q", "kc", "vc", "bt", "ctx", "ql")),
        k_scale=ks, v_scale=vs)
    assert out.dtype == torch.bfloat16 and out.shape == c["q"].shape
    for b, (_, n) in enumerate(c["specs"]):
        assert (out[b, n:] == 0).all(), f"row {b}: padding not zero"
    return out.float().cpu()


def _wide_tile_specs(B, Tq):
    """The mixed contexts and q_lens of test_prefill_kernel_wide_tile_dispatch
    (test_paged_prefill.py)."""
    return tuple(((13 * b) % 90, Tq if b % 5 else (7 * b) % (Tq + 1))
                 for b in range(B))


# --------------------------------------------------------------------------
# CPU: the probes reject defective references and accept the honest ones
# --------------------------------------------------------------------------

SELF_T = 768          # causal self-test shape: (1, 2, 1, 768)
SELF_L = 1000         # decode-like self-test: 8 query heads, one row, L keys


def _self_causal(kind):
    return _flash_case(kind, 1, 2, 1, SELF_T, SELF_T, True)


def _self_decode(kind):
    return _flash_case(kind, 1, 8, 1, 1, SELF_L, False)


def _with_mask(c, mask, premask_max=False, dtype=torch.float64):
    """The reference of case c under another mask."""
    if "kr" in c:
        kr, vr = c["kr"], c["vr"]
    else:
        rep = c["q"].shape[1] // c["k"].shape[1]
        kr = c["k"].repeat_interleave(rep, dim=1)
        vr = c["v"].repeat_interleave(rep, dim=1)
    return _attend64(c["q"], kr, vr, mask, premask_max, dtype)


def _ij(T, Tk):
    return torch.arange(T).view(T, 1), torch.arange(Tk).view(1, Tk)


def _defect_mask(name):
    """Causal T = 768 masks with one seeded defect."""
    i, j = _ij(SELF_T, SELF_T)
    ok = j <= i
    if name == "wide":          # one key too many, rows >= 256
        return ok | ((j == i + 1) & (i >= 256))
    if name == "no_diag":       # the diagonal key dropped, rows >= 256
        return ok & ~((j == i) & (i >= 256))
    if name == "sub_tile":      # one 32-key sub-tile skipped
        return ok & ~((j >= 320) & (j < 352))
    raise KeyError(name)


def _drop_mask(token):
    _, j = _ij(1, SELF_L)
    return j != token


def _rejects(check, *args):
    with pytest.raises(AssertionError):
        check(*args, tag="to be rejected")


def test_honest_references_pass_every_checker():
    for c in (_self_causal("count"), _self_decode("count")):
        out, lse = _with_mask(c, c["mask"])
        check_count(out, lse, c["n"], c["cnt"], tag="honest count")
        check_count(out.bfloat16(), lse.float(), c["n"], c["cnt"],
                    tag="honest count, rounded")
    for c in (_self_causal("allowed"), _self_decode("allowed"),
              _self_causal("forbidden")):
        check_needle(c["ref"], c["ref"], "honest needle")
        check_needle(c["ref"].bfloat16(), c["ref"], "honest needle, rounded")
    c = _flash_case("randn", 1, 2, 1, 256, 256, True)
    check_precision(c["emul"], c["emul"], c["ref"], "honest emulation")
    check_precision(c["ref"], c["emul"], c["ref"], "honest fp64")


@pytest.mark.parametrize("case", ["causal", "decode"])
def test_allowed_needle_reference_is_the_target_value_row(case):
    """The cap that makes a dropped target an O(|v|) error: the honest fp64
    reference is v[target] to NEEDLE_CAP."""
    c = _self_causal("allowed") if case == "causal" else _self_decode(
        "allowed")
    err = float((c["ref"] - c["vr"][:, :, c["tgt"]].double()).abs().max())
    print(f"{case}: max |ref - v[target]| {err:.3e}")
    assert err <= NEEDLE_CAP


@pytest.mark.parametrize("name", ["wide", "no_diag", "sub_tile"])
def test_count_probe_rejects_causal_mask_defects(name):
    c = _self_causal("count")
    out, lse = _with_mask(c, _defect_mask(name))
    _rejects(check_count, out, lse, c["n"], c["cnt"])
    _rejects(check_count, out, None, c["n"], c["cnt"])   # out alone, too
    honest, _ = _with_mask(c, c["mask"])
    _rejects(check_count, honest, lse, c["n"], c["cnt"])  # and lse alone


@pytest.mark.parametrize("token", [SELF_L - 1, 336, 0])
def test_count_probe_rejects_one_dropped_token(token):
    """Token seq_len - 1, a token at a split boundary (336 of 1000 at three
    splits) and the first token. On the same inputs the old allclose(4e-2)
    check accepts the defect."""
    c = _self_decode("count")
    out, lse = _with_mask(c, _drop_mask(token))
    _rejects(check_count, out, lse, c["n"], c["cnt"])
    _rejects(check_count, out, None, c["n"], c["cnt"])
    honest, _ = _with_mask(c, c["mask"])
    assert _old_check(out, honest)


def test_old_check_accepts_dropped_last_token_on_randn_inputs():
    """What the new tests add: with randn q, k, v at L = 1000 the check the
    suite had (bf16 output, allclose 4e-2) passes a reference that lost
    token seq_len - 1; the needle probe on the same shape does not."""
    c = _self_decode("randn")
    out, _ = _with_mask(c, _drop_mask(SELF_L - 1))
    err = float((out - c["ref"]).abs().max())
    print(f"randn, token {SELF_L - 1} dropped: max abs err {err:.3e}")
    assert err > 0 and _old_check(out, c["ref"])
    c = _self_decode("allowed")
    out, _ = _with_mask(c, _drop_mask(SELF_L - 1))
    _rejects(check_needle, out, c["ref"])
    _rejects(check_needle, out.bfloat16(), c["ref"])


def test_allowed_needle_rejects_dropped_diagonal():
    c = _self_causal("allowed")
    out, _ = _with_mask(c, _defect_mask("no_diag"))
    rows = (out - c["ref"]).abs().amax(-1) > 0.5
    print(f"diagonal dropped: {int(rows.sum())} rows off by more than 0.5")
    assert bool(rows[:, :, 256:].all()) and not bool(rows[:, :, :256].any())
    _rejects(check_needle, out, c["ref"])


@pytest.mark.parametrize("kind", FORBIDDEN)
def test_forbidden_needle_rejects_wide_mask(kind):
    c = _self_causal(kind)
    out, _ = _with_mask(c, _defect_mask("wide"))
    rows = (out - c["ref"]).abs().amax(-1) > 0.5
    print(f"mask one key wide: {int(rows.sum())} rows off by more than 0.5")
    assert bool(rows[:, :, 256:SELF_T - 1].all())
    _rejects(check_needle, out, c["ref"])


def test_strong_needle_rejects_max_taken_before_the_mask():
    """A running max over the unmasked scores loses a row only when the
    masked score is past fp32's exponent range (about 87 nats) above the
    allowed ones. The factor-4 needle sits about 30 nats above them: P is
    tiny but normal, the row sum scales with it and the result is right, so
    that needle cannot see this defect. The factor-16 needle scores about 180
    against a standard deviation of 16: every P underflows to 0 and the rows
    come out NaN."""
    c = _self_causal("forbidden")
    out, _ = _with_mask(c, c["mask"], premask_max=True, dtype=torch.float32)
    check_needle(out, c["ref"], "factor 4, max before mask")    # not seen
    c = _self_causal("strong")
    check_needle(c["ref"].bfloat16(), c["ref"], "honest strong needle")
    out, _ = _with_mask(c, c["mask"], premask_max=True, dtype=torch.float32)
    bad = ~torch.isfinite(out).all(-1)
    print(f"factor 16, max before mask: {int(bad.sum())} of {bad.numel()} "
          f"rows NaN")
    assert int(bad.sum()) > 0.9 * bad.numel()   # 1446 of 1536 as measured
    _rejects(check_needle, out, c["ref"])


def test_precision_bound_rejects_an_extra_rounding():
    """Scores rounded to bf16 before the softmax is one rounding more than
    the emulation has. On the needle inputs (scores of standard deviation 4)
    it costs 9.2e-3 against the emulation's 1.8e-3; on unit-variance randn
    scores it would stay inside the factor 2 (3.2e-3 against 2.0e-3)."""
    c = _self_causal("forbidden")
    emul = _emulate(c["q"], c["kr"], c["vr"], c["mask"])
    check_precision(emul, emul, c["ref"], "emulation")
    bad = _emulate(c["q"], c["kr"], c["vr"], c["mask"], round_scores=True)
    _rejects(check_precision, bad, emul, c["ref"])


def test_paged_pool_holds_the_rows_and_nothing_else():
    """The case builders themselves: a sequence's table entries lead to its
    seq_len rows and the one appended forbidden token, all finite; the null
    page, the tail slots and the spare pages are NaN; and the query is aimed
    at the forbidden token's key."""
    for fmt in ("bf16", "fp8"):
        lens = (1, 16, 33)
        c = _decode_case("forbidden", 64, 4, 2, fmt, lens)
        kf = c["kc"].float()
        finite = torch.isfinite(kf).all(-1).all(1)          # [page, slot]
        assert torch.equal(finite,
                           torch.isfinite(c["vc"].float()).all(-1).all(1))
        assert int(finite.sum()) == sum(lens) + len(lens)
        assert not bool(finite[0].any())                    # the null page
        for b, n in enumerate(lens):
            # unused table entries are 0, the null page
            flat = finite[c["bt"][b].long()].reshape(-1)
            assert bool(flat[:n + 1].all())
            assert not bool(flat[n + 1:].any())
            assert int(c["bt"][b, n // PAGE]) != 0          # token n's page
        ks, _ = SCALES[fmt]
        # the query is four times the forbidden token's stored key
        pg = int(c["bt"][2, 33 // PAGE])
        assert torch.equal(c["q"][2, 0].float(),
                           4 * ks * kf[pg, 0, 33 % PAGE])


# --------------------------------------------------------------------------
# GPU: flash_attention (flash_attn_v7 at T % 256 == 0, else flash_attn_v5)
# --------------------------------------------------------------------------

# (layout, B, Hq, Hkv, T, Tk, causal, q_offset)
CAUSAL_768 = [(lay, 1, 4, 2, 768, 768, True, 0)
              for lay in ("bhtd", "bthd", "packed")]
FLASH_COUNT = CAUSAL_768 + [
    ("bhtd", 1, 4, 2, 256, 40, False, 0),
    ("bhtd", 1, 4, 2, 256, 300, False, 0),
    ("bhtd", 1, 4, 2, 256, 1024, False, 0),
    ("bhtd", 1, 4, 2, 256, 576, True, 320),
    ("bhtd", 1, 4, 2, 384, 384, True, 0),      # the 128-row kernel
    ("bhtd", 1, 4, 2, 384, 384, False, 0),
    ("bhtd", 1, 4, 2, 200, 200, True, 0),      # padded to 256 inside
    ("bhtd", 1, 4, 2, 200, 200, False, 0),
]
FLASH_NEEDLE = [(kind,) + s for kind in ("allowed", "forbidden")
                for s in CAUSAL_768 + [
                    ("bhtd", 1, 4, 2, 256, 576, True, 320),
                    ("bhtd", 1, 4, 2, 384, 384, True, 0)]] + [
    ("allowed", "bhtd", 1, 4, 2, 256, 300, False, 0),
    ("allowed", "bhtd", 1, 4, 2, 384, 384, False, 0),
    ("strong", "bhtd", 1, 4, 2, 768, 768, True, 0),
    ("strong", "bhtd", 1, 4, 2, 256, 576, True, 320),
    ("strong", "bhtd", 1, 4, 2, 384, 384, True, 0),
]


def _flash_id(p):
    p = tuple(p)
    kind = p[0] + "-" if p[0] in NEEDLE_FACTOR else ""
    lay, B, Hq, Hkv, T, Tk, causal, qo = p[-8:]
    return (f"{kind}{lay}-B{B}Hq{Hq}Hkv{Hkv}T{T}Tk{Tk}"
            f"{'c' if causal else 'f'}{qo}")


@pytest.mark.gpu
@pytest.mark.parametrize("p", FLASH_COUNT, ids=_flash_id)
def test_flash_count_probe(p):
    dev = _gpu()
    layout, shape = p[0], p[1:]
    c = _flash_case("count", *shape)
    out, lse = _run_flash(c, layout, dev)
    check_count(out, lse, c["n"], c["cnt"], tag=_flash_id(p))


@pytest.mark.gpu
@pytest.mark.parametrize("p", FLASH_NEEDLE, ids=_flash_id)
def test_flash_needle_probe(p):
    dev = _gpu()
    kind, layout, shape = p[0], p[1], p[2:]
    c = _flash_case(kind, *shape)
    out, lse = _run_flash(c, layout, dev)
    check_needle(out, c["ref"], _flash_id(p))
    assert torch.allclose(lse.double(), c["ref_lse"], atol=2e-2, rtol=2e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 8, 2, 512, 512, True, 0),
                                   (1, 4, 2, 256, 300, False, 0),
                                   (1, 4, 2, 384, 384, True, 0)],
                         ids=lambda s: _flash_id(("bhtd",) + s))
def test_flash_precision_bound(shape):
    dev = _gpu()
    c = _flash_case("randn", *shape)
    out, _ = _run_flash(c, "bhtd", dev)
    check_precision(out, c["emul"], c["ref"], _flash_id(("bhtd",) + shape))


# --------------------------------------------------------------------------
# GPU: paged_attention_decode
# --------------------------------------------------------------------------

COUNT_LENS = (0, 1, 15, 16, 17, 33, 255, 256, 257, 1000)
NEEDLE_LENS = (1, 15, 16, 17, 33, 256, 257, 1000)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_count_probe(D, Hq, Hkv, fmt):
    """64 splits of at most 63 pages leaves empty splits in every row."""
    dev = _gpu()
    c = _decode_case("count", D, Hq, Hkv, fmt, COUNT_LENS)
    _, vs = SCALES[fmt]
    B = len(COUNT_LENS)
    n, cnt = c["n"], c["cnt"]
    for S in (1, 3, 8, 64):
        tag = f"decode {fmt} D{D} Hq{Hq} Hkv{Hkv} splits {S}"
        ws = None
        if S > 1:
            ws = torch.full((B * Hq * S * (D + 2),), float("nan"),
                            dtype=torch.float32, device=dev)
        out = _run_decode(c, dev, S, ws)
        check_count(out, None, n, cnt, vs, tag)
        if S == 1:
            continue
        # the partials: ws_o [B,Hq,S,D], then ws_ml [B,Hq,S,2] = (m, l)
        ws = ws.cpu()
        o = ws[:B * Hq * S * D].view(B, Hq, S, D).double()
        m, l = ws[B * Hq * S * D:].view(B, Hq, S, 2).double().unbind(-1)
        full = m == 0
        assert bool((full | (m == float("-inf"))).all()), tag
        assert bool((full.any(-1) == (n > 0)).all()), tag
        zero = torch.zeros((), dtype=torch.float64)
        l_sum = torch.where(full, l, zero).sum(-1)
        o_sum = torch.where(full.unsqueeze(-1), o, zero).sum(2)
        assert torch.equal(l_sum, n.double()), tag
        assert torch.equal(o_sum, vs * cnt), tag
        if S == 64:
            assert bool((~full).any(-1).all()), tag


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(NEEDLE_FACTOR))
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_needle_probe(D, Hq, Hkv, fmt, kind):
    dev = _gpu()
    c = _decode_case(kind, D, Hq, Hkv, fmt, NEEDLE_LENS)
    for S in (1, 3, 8):
        check_needle(_run_decode(c, dev, S), c["ref"],
                     f"decode {kind} {fmt} D{D} Hq{Hq} Hkv{Hkv} splits {S}")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_decode_precision_bound(fmt):
    dev = _gpu()
    c = _decode_case("randn", 128, 8, 2, fmt, (1000, 33))
    for S in (1, 8):
        check_precision(_run_decode(c, dev, S), c["emul"], c["ref"],
                        f"decode {fmt} lens (1000, 33) splits {S}")


# --------------------------------------------------------------------------
# GPU: paged_attention_prefill (no LSE output: the `out` checks only)
# --------------------------------------------------------------------------

PREFILL_SHAPES = [(0, 1), (15, 17), (60, 70), (100, 130), (5, 260)]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("ctx,Tq", PREFILL_SHAPES)
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_count_probe(D, ctx, Tq, fmt):
    dev = _gpu()
    c = _prefill_case("count", D, 8, 2, fmt, ((ctx, Tq),), Tq)
    check_count(_run_prefill(c, dev), None, c["n"], c["cnt"],
                SCALES[fmt][1], f"prefill {fmt} D{D} ctx{ctx} Tq{Tq}")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("B,Tq", [(64, 3), (22, 260)])
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_count_probe_wide_tile_dispatch(D, B, Tq, fmt):
    """Both shapes are past the 512 blocks of 128 query rows at which the
    binding launches 256-row tiles; mixed contexts, short and empty rows."""
    dev = _gpu()
    assert -(-Tq // 128) * 8 * B >= 512
    c = _prefill_case("count", D, 8, 2, fmt, _wide_tile_specs(B, Tq), Tq)
    check_count(_run_prefill(c, dev), None, c["n"], c["cnt"],
                SCALES[fmt][1], f"prefill wide {fmt} D{D} B{B} Tq{Tq}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(NEEDLE_FACTOR))
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("ctx,Tq", [(15, 17), (100, 130), (5, 260)])
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_needle_probe(D, ctx, Tq, fmt, kind):
    dev = _gpu()
    c = _prefill_case(kind, D, 8, 2, fmt, ((ctx, Tq),), Tq)
    check_needle(_run_prefill(c, dev), c["ref"],
                 f"prefill {kind} {fmt} D{D} ctx{ctx} Tq{Tq}")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_prefill_precision_bound(fmt):
    dev = _gpu()
    c = _prefill_case("randn", 128, 8, 2, fmt, ((100, 130),), 130)
    check_precision(_run_prefill(c, dev), c["emul"], c["ref"],
                    f"prefill {fmt} ctx100 Tq130")
