"""ray_amd.ops — hand-written CDNA4 HIP kernels with torch autograd.

Each op has a plain-PyTorch fp32 reference (`*_ref`) used on CPU and in
numerics tests. On a GPU box the HIP extension is REQUIRED: if a CUDA
tensor reaches an op and `ray_amd._hip_ops` is missing, we raise rather
than silently falling back to eager torch.
"""
from __future__ import annotations

import os

import torch

try:
    from ray_amd import _hip_ops as _K

    HAVE_HIP_OPS = True
except ImportError:  # CPU-only environment without a built extension
    _K = None
    HAVE_HIP_OPS = False


def _require_ext(name: str):
    if _K is None:
        raise RuntimeError(
            f"ray_amd HIP extension not built but {name} was called on a GPU "
            "tensor. Run `python ray_amd/csrc/build.py`."
        )


# --------------------------------------------------------------------------
# RMSNorm
# --------------------------------------------------------------------------


def rmsnorm_ref(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5):
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * inv * w.float()).to(x.dtype)


class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, eps):
        _require_ext("rmsnorm")
        # save what the kernel read: backward reads the same buffers
        x = x.contiguous()
        w = w.contiguous()
        y, inv = _K.rmsnorm_fwd(x, w, eps)
        ctx.save_for_backward(x, w, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, inv = ctx.saved_tensors
        dx, dw = _K.rmsnorm_bwd(dy.contiguous(), x, w, inv)
        return dx, dw.to(w.dtype), None


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5):
    if not x.is_cuda:
        # autograd-capable reference path
        xf = x.float()
        inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        return (xf * inv * w.float()).to(x.dtype)
    return _RMSNorm.apply(x, w, eps)


# test hook: False sends LlamaModel's training path back to separate
# residual adds and norms (for monkeypatch, like _WGRAD_FORCE)
_FUSED_ADD_NORM = True


class _AddRMSNorm(torch.autograd.Function):
    """s = x + r and h = rmsnorm(s), one forward kernel. Backward is one
    call: the norm's dx with the gradient of s added in the kernel's store
    (rounded as the bf16 add of the two tensors), which is the gradient of
    both x and r."""

    @staticmethod
    def forward(ctx, x, r, w, eps):
        _require_ext("add_rmsnorm")
        ctx.set_materialize_grads(False)
        w = w.contiguous()
        s, h, inv = _K.add_rmsnorm_fwd(x.contiguous(), r.contiguous(), w, eps)
        ctx.save_for_backward(s, w, inv)
        return s, h

    @staticmethod
    def backward(ctx, g_s, g_h):
        if g_h is None:
            return g_s, g_s, None, None
        s, w, inv = ctx.saved_tensors
        dx, dw = _K.rmsnorm_bwd_res(
            g_h.contiguous(), s, w, inv,
            None if g_s is None else g_s.contiguous())
        return dx, dx, dw.to(w.dtype), None


def add_rmsnorm(x: torch.Tensor, r: torch.Tensor, w: torch.Tensor,
                eps: float = 1e-5):
    """(s, h) with s = x + r and h = rmsnorm(s, w, eps)."""
    if not x.is_cuda:
        s = x + r
        return s, rmsnorm(s, w, eps)
    return _AddRMSNorm.apply(x, r, w, eps)


class RMSNorm(torch.nn.Module):
    def __init__(self, dim: int, eps: float = 1e-5, dtype=torch.bfloat16):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(dim, dtype=dtype))
        self.eps = eps

    def forward(self, x):
        return rmsnorm(x, self.weight, self.eps)


# --------------------------------------------------------------------------
# SwiGLU
# --------------------------------------------------------------------------


def swiglu_ref(a: torch.Tensor, b: torch.Tensor):
    return (torch.nn.functional.silu(a.float()) * b.float()).to(a.dtype)


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        _require_ext("swiglu")
        a = a.contiguous()
        b = b.contiguous()
        ctx.save_for_backward(a, b)
        return _K.swiglu_fwd(a, b)

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        da, db = _K.swiglu_bwd(dy.contiguous(), a, b)
        return da, db


def swiglu(a: torch.Tensor, b: torch.Tensor):
    if not a.is_cuda:
        return torch.nn.functional.silu(a) * b
    return _SwiGLU.apply(a, b)


# --------------------------------------------------------------------------
# RoPE
# --------------------------------------------------------------------------


def rope_tables(T: int, D: int, base: float = 500000.0, device="cpu"):
    """Host-precomputed cos/sin [T, D/2] fp32 (guide §B: no device trig)."""
    half = D // 2
    inv_freq = 1.0 / (
        base ** (torch.arange(0, half, dtype=torch.float64) / half)
    )
    t = torch.arange(T, dtype=torch.float64)
    ang = torch.outer(t, inv_freq)
    return (
        ang.cos().float().contiguous().to(device),
        ang.sin().float().contiguous().to(device),
    )


def rope_ref(x: torch.Tensor, cosT: torch.Tensor, sinT: torch.Tensor):
    """x: [B, T, Hn, D]; rotate halves (LLaMA convention)."""
    B, T, Hn, D = x.shape
    half = D // 2
    x1 = x[..., :half].float()
    x2 = x[..., half:].float()
    c = cosT[:T].view(1, T, 1, half)
    s = sinT[:T].view(1, T, 1, half)
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(x.dtype)


class _Rope(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cosT, sinT, n_heads, T):
        _require_ext("rope")
        ctx.meta = (cosT, sinT, n_heads, T)
        # fused-QKV slices ([H,D]-contiguous, strided (b,t) rows) go
        # straight to the kernel — RoPE doubles as the gather
        if not (x.dim() == 4 and x.stride(3) == 1
                and x.stride(2) == x.size(3)
                and x.stride(0) == x.size(1) * x.stride(1)):
            x = x.contiguous()
        return _K.rope_apply(x, cosT, sinT, n_heads, T, 1)

    @staticmethod
    def backward(ctx, dy):
        cosT, sinT, n_heads, T = ctx.meta
        dx = _K.rope_apply(dy.contiguous(), cosT, sinT, n_heads, T, -1)
        return dx, None, None, None, None


def rope(x: torch.Tensor, cosT: torch.Tensor, sinT: torch.Tensor):
    """x: [B, T, Hn, D] bf16."""
    B, T, Hn, D = x.shape
    if not x.is_cuda:
        return rope_ref(x, cosT, sinT)
    return _Rope.apply(x, cosT[:T].contiguous(), sinT[:T].contiguous(), Hn, T)


def linear_sb(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """Small-batch linear for decode (csrc/hip/gemv.hip): one wave per
    output row streams W once. Measured vs hipBLASLt
    (tools/gemv_ab.py): wins 1.4-2x at rows<=2 with N<=8192 (the
    qkv/o projections at decode batch 1-2); hipBLASLt already runs
    near-bandwidth (5.7+ TB/s) at larger N/K, so those shapes fall
    back. VALU-bound above rows=2 (each W element costs `rows` fmas)."""
    K = x.shape[-1]
    rows = x.numel() // K
    if (
        _K is not None
        and x.is_cuda
        and x.dtype == torch.bfloat16
        and weight.dtype == torch.bfloat16
        and rows <= 2
        and weight.shape[0] <= 8192
        and K % 512 == 0
        and not torch.is_grad_enabled()
    ):
        y = _K.gemv(x.reshape(rows, K).contiguous(), weight)
        return y.view(*x.shape[:-1], weight.shape[0])
    return torch.nn.functional.linear(x, weight)


# --------------------------------------------------------------------------
# FP8 weight-only linear for decode (csrc/hip/linear_w8.hip)
# --------------------------------------------------------------------------

def quantize_weight_fp8(w: torch.Tensor):
    """[N, K] finite weights -> (wq float8_e4m3fn [N, K], scale fp32 [N]).
    Per output channel scale = amax(|w[n, :]|) / 448 (1 for a row of
    zeros) and wq = e4m3fn_rne(clamp(fp32(w) / scale, -448, 448)): the
    saturating rule of quantize_kv_fp8 with a per-row scale, so no byte
    is a NaN. The weight dequantises as wq.float() * scale[:, None]."""
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    wq = (wf / scale[:, None]).clamp(-FP8_MAX, FP8_MAX)
    return wq.to(torch.float8_e4m3fn), scale


def linear_w8_ref(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor):
    """fp64 reference of linear_w8, returned as fp32."""
    w = wq.float().double() * scale.double()[:, None]
    return (x.double() @ w.t()).float()


# (N, K) -> the largest row count that goes to linear_w8_gemm
# (csrc/hip/linear_w8_gemm.hip) instead of dequantise + F.linear. A shape
# enters, with the largest M up to which it won at every measured M
# (64, 128, 256, 512, 1024, 2048), only if the kernel's slowest repetition
# beat the fallback's fastest in tools/linear_w8_bench.py --gemm (times in
# the comments, µs at the listed M, kernel median / fallback median).
# Shapes not listed keep the fallback.
_W8_GEMM_TABLE: dict = {
    # llama3-8b; all five won at every measured M, times at M = 2048
    (6144, 4096): 2048,     # qkv:      117.0 /  181.1 (M = 64:  21.4 /  115.7)
    (4096, 4096): 2048,     # o_proj:    76.2 /  128.2 (M = 64:  14.2 /   81.5)
    (14336, 4096): 2048,    # gate/up:  321.7 /  454.8 (M = 64:  29.9 /  320.2)
    (4096, 14336): 2048,    # down:     287.5 /  494.4 (M = 64:  29.0 /  342.4)
    (128256, 4096): 2048,   # lm_head: 3263.2 / 4173.3 (M = 64: 190.5 / 2810.4)
    # llama3-1b, likewise
    (3072, 2048): 2048,     # qkv:       40.3 /   59.6 (M = 64:  10.5 /   41.6)
    (2048, 2048): 2048,     # o_proj:    24.7 /   45.4 (M = 64:  10.1 /   37.5)
    (8192, 2048): 2048,     # gate/up:   82.4 /  120.4 (M = 64:  13.5 /   79.6)
    (2048, 8192): 2048,     # down:      76.8 /  134.8 (M = 64:  16.0 /   87.1)
    (128256, 2048): 2048,   # lm_head: 1654.4 / 2139.1 (M = 64:  85.6 / 1431.4)
}

# test hook: send every qualifying call of 33+ rows to the kernel
_W8_GEMM_FORCE = False


def linear_w8(x: torch.Tensor, wq: torch.Tensor,
              scale: torch.Tensor) -> torch.Tensor:
    """x[..., K] · (wq[N, K] * scale[N])^T with fp8 weights (see
    quantize_weight_fp8). bf16 GPU activations with K % 128 == 0, grad off
    and contiguous, 16-byte-aligned operands run a kernel that reads one
    byte per weight: the skinny-GEMM kernel for at most 32 rows, and the
    W8A16 GEMM kernel (linear_w8_gemm: prefill chunks, decode steps of more
    than 32 sequences) for 33 rows up to the limit _W8_GEMM_TABLE lists for
    the shape (N, K), N % 128 == 0. Everything else (CPU, shapes and row
    counts that are not listed, odd shapes, grad on) dequantises the weight
    to the activation dtype and calls F.linear, which costs a bf16 copy of
    the weight per call."""
    K = x.shape[-1]
    rows = x.numel() // K
    if x.is_cuda:
        _require_ext("linear_w8")
        N = wq.shape[0]
        gemm = (rows > 32 and N % 128 == 0 and
                (_W8_GEMM_FORCE or rows <= _W8_GEMM_TABLE.get((N, K), 0)))
        if (x.dtype == torch.bfloat16 and (1 <= rows <= 32 or gemm)
                and K % 128 == 0
                and not torch.is_grad_enabled() and wq.is_contiguous()
                and wq.data_ptr() % 16 == 0):
            x2 = x.reshape(rows, K).contiguous()
            if x2.data_ptr() % 16 == 0:
                if gemm:
                    y = _K.linear_w8_gemm(x2, wq, scale.contiguous())
                else:
                    y = _K.linear_w8(x2, wq, scale.contiguous())
                return y.view(*x.shape[:-1], wq.shape[0])
    w = (wq.float() * scale[:, None]).to(x.dtype)
    return torch.nn.functional.linear(x, w)


class LinearW8(torch.nn.Module):
    """A bias-free linear whose weight is stored as fp8 bytes plus one fp32
    scale per output channel (buffers `wq`, `scale`); it holds no bf16
    copy of the weight."""

    def __init__(self, wq: torch.Tensor, scale: torch.Tensor):
        super().__init__()
        self.out_features, self.in_features = wq.shape
        self.register_buffer("wq", wq)
        self.register_buffer("scale", scale)

    @classmethod
    def from_linear(cls, linear: torch.nn.Linear) -> "LinearW8":
        if linear.bias is not None:
            raise ValueError("LinearW8 has no bias")
        return cls(*quantize_weight_fp8(linear.weight))

    def forward(self, x):
        return linear_w8(x, self.wq, self.scale)


# --------------------------------------------------------------------------
# MXFP4 weight-only linear for decode (csrc/hip/linear_w4.hip)
# --------------------------------------------------------------------------

# magnitude of e2m1 code 0..7; bit 3 of a nibble is the sign
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
MXFP4_BLOCK = 32


def quantize_weight_mxfp4(w: torch.Tensor):
    """[N, K] finite weights, K % 32 == 0 -> (wq uint8 [N, K/2], scales
    uint8 [N, K/32]): OCP MXFP4. Each block of 32 consecutive k has one e8m0
    scale code = clamp(floor(log2(amax)) - 2 + 127, 2, 252) (127 for a block
    of zeros); its elements are w / 2^(code-127) rounded to the nearest
    e2m1 value (0, 0.5, 1, 1.5, 2, 3, 4, 6 and a sign bit), ties to the even
    mantissa, saturating at +-6. Element 2i is the low nibble of byte i and
    2i+1 the high nibble. Codes stay inside 2..252 so that every
    dequantised value is zero or a normal bf16; no NaN code is produced."""
    N, K = w.shape
    if K % MXFP4_BLOCK:
        raise ValueError(f"quantize_weight_mxfp4: K = {K} is not a multiple "
                         f"of {MXFP4_BLOCK}")
    wf = w.detach().double().reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = wf.abs().amax(dim=2)
    # frexp: amax = m * 2^e with 0.5 <= m < 1, so floor(log2(amax)) = e - 1
    e = torch.frexp(amax)[1].to(torch.int64) - 1
    code = torch.where(amax > 0, (e - 2 + 127).clamp(2, 252),
                       torch.full_like(e, 127))
    v = (wf.abs() * torch.exp2((127 - code).double())[..., None]).clamp(max=6.0)
    # the grid has step 0.5 below 2, 1 below 4 and 2 up to 6; torch.round
    # rounds halves to even, which is the even mantissa on each step
    q = torch.where(v < 2, torch.round(v * 2) / 2,
                    torch.where(v < 4, torch.round(v), torch.round(v / 2) * 2))
    grid = torch.tensor(_E2M1, dtype=torch.float64, device=w.device)
    nib = torch.bucketize(q, grid).to(torch.uint8)
    nib = nib | ((wf < 0) & (nib > 0)).to(torch.uint8) * 8
    nib = nib.reshape(N, K // 2, 2)
    return nib[..., 0] | (nib[..., 1] << 4), code.to(torch.uint8)


def quantize_expert_weights_mxfp4(w: torch.Tensor):
    """quantize_weight_mxfp4 of expert weights [E, N, K], expert by expert
    (the fp64 temporaries stay at one expert's size): wq uint8 [E, N, K/2]
    and scales uint8 [E, N, K/32], what ops.moe_experts takes with
    `scales`."""
    pairs = [quantize_weight_mxfp4(w[e]) for e in range(w.shape[0])]
    return (torch.stack([p[0] for p in pairs]),
            torch.stack([p[1] for p in pairs]))


def dequantize_mxfp4(wq: torch.Tensor, scales: torch.Tensor,
                     dtype=torch.float32) -> torch.Tensor:
    """The weight [N, K] that (wq, scales) of quantize_weight_mxfp4 stand
    for, by table lookup; exact in bf16, fp32 and fp64."""
    N = wq.shape[0]
    nib = torch.stack((wq & 15, wq >> 4), dim=-1).reshape(N, -1).long()
    # every product is exact in fp32 already (codes 2..252)
    wide = torch.float64 if dtype == torch.float64 else torch.float32
    table = torch.tensor(_E2M1 + tuple(-m for m in _E2M1), dtype=wide,
                         device=wq.device)
    scale = torch.exp2(scales.to(wide) - 127)
    w = table[nib] * scale.repeat_interleave(MXFP4_BLOCK, dim=1)
    return w.to(dtype)


def linear_w4_ref(x: torch.Tensor, wq: torch.Tensor, scales: torch.Tensor):
    """fp64 reference of linear_w4, returned as fp32."""
    w = dequantize_mxfp4(wq, scales, torch.float64)
    return (x.double() @ w.t()).float()


# (N, K) -> the largest row count that goes to linear_w4_gemm
# (csrc/hip/linear_w4_gemm.hip) instead of dequant_mxfp4 + F.linear. The
# rule is _W8_GEMM_TABLE's: a shape enters, with the largest M up to which it
# won at every measured M (64, 96, 128, 256, 512, 1024, 2048), only if the
# kernel's slowest repetition beat the fallback's fastest in
# tools/linear_w8_bench.py --gemm --weights mxfp4 (times in the comments, µs
# at the listed M, kernel median / fallback median). dequant_mxfp4 is a
# cheap pass, so the limits end below 2048: beyond them, and for shapes not
# listed, the fallback stays (PERFORMANCE.md has the losing rows).
_W4_GEMM_TABLE: dict = {
    # llama3-8b
    (6144, 4096): 512,      # qkv:      36.6 /  51.4 (M = 64:  14.7 /  39.7)
    (4096, 4096): 1024,     # o_proj:   38.5 /  50.9 (M = 64:  13.0 /  34.0)
    (14336, 4096): 512,     # gate/up:  73.1 /  90.1 (M = 64:  27.1 /  64.1)
    (4096, 14336): 256,     # down:     48.2 /  86.9 (M = 64:  28.1 /  74.6)
    #                         (lost at 512: 112.8 / 116.5, slowest 113.4
    #                         against the fallback's fastest 112.4)
    (128256, 4096): 512,    # lm_head: 652.5 / 882.3 (M = 64: 127.9 / 576.9)
    # llama3-1b
    (3072, 2048): 1024,     # qkv:      21.3 /  31.4 (M = 64:  11.1 /  23.3)
    (2048, 2048): 2048,     # o_proj:   22.6 /  29.7 (M = 64:  10.6 /  23.3)
    (8192, 2048): 1024,     # gate/up:  42.8 /  48.8 (M = 64:  12.7 /  32.8)
    (2048, 8192): 256,      # down:     30.9 /  39.4 (M = 64:  13.9 /  38.2)
    #                         (lost at 512: 49.6 / 42.3)
    (128256, 2048): 512,    # lm_head: 347.7 / 442.4 (M = 64:  63.2 / 298.8)
}

# test hook: send every qualifying call of 33+ rows to the kernel
_W4_GEMM_FORCE = False


def linear_w4(x: torch.Tensor, wq: torch.Tensor,
              scales: torch.Tensor) -> torch.Tensor:
    """x[..., K] · dequant(wq[N, K/2], scales[N, K/32])^T with MXFP4 weights
    (see quantize_weight_mxfp4). bf16 GPU activations with K % 128 == 0,
    grad off and contiguous, 16-byte-aligned operands run a kernel that
    reads 17/32 byte per weight: the W4A16 skinny-GEMM kernel for 1 to 32
    rows, and the W4A16 GEMM kernel (linear_w4_gemm: prefill chunks, decode
    steps of more than 32 sequences) for 33 rows up to the limit
    _W4_GEMM_TABLE lists for the shape (N, K), N % 128 == 0. More rows, and
    shapes that are not listed, dequantise with one kernel pass and call
    F.linear, which costs a bf16 copy of the weight per call. Everything
    else (CPU, other dtypes, odd K, grad on) dequantises in torch to the
    activation dtype and calls F.linear."""
    K = x.shape[-1]
    rows = x.numel() // K
    if (x.is_cuda and x.dtype == torch.bfloat16 and rows >= 1
            and K % 128 == 0 and not torch.is_grad_enabled()
            and wq.is_contiguous() and scales.is_contiguous()
            and wq.data_ptr() % 16 == 0 and scales.data_ptr() % 4 == 0):
        _require_ext("linear_w4")
        N = wq.shape[0]
        gemm = (rows > 32 and N % 128 == 0 and
                (_W4_GEMM_FORCE or rows <= _W4_GEMM_TABLE.get((N, K), 0)))
        x2 = x.reshape(rows, K).contiguous() if gemm or rows <= 32 else None
        if gemm and x2.data_ptr() % 16 == 0:
            return _K.linear_w4_gemm(x2, wq, scales).view(*x.shape[:-1], N)
        if rows > 32:
            return torch.nn.functional.linear(x, _K.dequant_mxfp4(wq, scales))
        if x2.data_ptr() % 16 == 0:
            y = _K.linear_w4(x2, wq, scales)
            return y.view(*x.shape[:-1], wq.shape[0])
    return torch.nn.functional.linear(x, dequantize_mxfp4(wq, scales, x.dtype))


class LinearW4(torch.nn.Module):
    """A bias-free linear whose weight is stored as MXFP4: two e2m1 elements
    per byte plus one e8m0 scale byte per 32 (buffers `wq`, `scales`); it
    holds no bf16 copy of the weight."""

    def __init__(self, wq: torch.Tensor, scales: torch.Tensor):
        super().__init__()
        self.out_features, self.in_features = wq.shape[0], 2 * wq.shape[1]
        self.register_buffer("wq", wq)
        self.register_buffer("scales", scales)

    @classmethod
    def from_linear(cls, linear: torch.nn.Linear) -> "LinearW4":
        if linear.bias is not None:
            raise ValueError("LinearW4 has no bias")
        return cls(*quantize_weight_mxfp4(linear.weight))

    def forward(self, x):
        return linear_w4(x, self.wq, self.scales)


# --------------------------------------------------------------------------
# Linear with a hand-written weight-gradient GEMM (csrc/hip/gemm_wgrad.hip)
# --------------------------------------------------------------------------

WGRAD_M_GRANULE = 128  # tokens: the kernel's loop handles two 64-token tiles

# (N, K, problems) -> use gemm_wgrad for dW[N,K] = dy^T x. A shape enters
# only if the kernel's slowest repetition beat torch's fastest in
# tools/gemm_wgrad_bench.py at M = 32768 (times in the comments, ms,
# kernel median / torch median). Shapes not listed go to torch.
_WGRAD_TABLE: dict = {
    (14336, 4096, 1): True,   # gate / up alone: 3.160 / 3.755
    (4096, 14336, 1): True,   # down:            3.105 / 3.767
    (14336, 4096, 2): True,   # gate + up:       6.013 / 7.544
    (4096, 4096, 1): True,    # o_proj:          0.820 / 0.933
    (128256, 4096, 1): True,  # lm_head:        29.159 / 30.042
    # qkv (6144, 4096): 1.410 / 1.414, slowest 1.431 against torch's
    # fastest 1.405: stays with torch (384 blocks = 1.5 waves of 256 CUs)
}

# test hook: send every qualifying shape to the kernel
_WGRAD_FORCE = False


def _wgrad_switch_on() -> bool:
    return not os.environ.get("RAY_AMD_NO_WGRAD_GEMM")


def _wgrad_listed(N: int, K: int, problems: int = 1) -> bool:
    if N % 256 or K % 256:
        return False
    return _WGRAD_FORCE or (N, K, problems) in _WGRAD_TABLE


def _wgrad_operand_ok(t: torch.Tensor) -> bool:
    return (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 2
            and t.stride(1) == 1 and t.stride(0) % 8 == 0
            and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0
            and t.shape[1] % 256 == 0 and t.shape[1] > 0
            and t.stride(0) * 64 < 2 ** 30)


def _wgrad_rows_ok(M: int) -> bool:
    return M >= WGRAD_M_GRANULE and M % WGRAD_M_GRANULE == 0


def gemm_wgrad(dy: torch.Tensor, x: torch.Tensor, out=None) -> torch.Tensor:
    """dW[N,K] = dy[M,N]^T @ x[M,K] with the HIP kernel; raises when the
    operands do not qualify (callers that want a fallback use `_wgrad`)."""
    _require_ext("gemm_wgrad")
    if not (_wgrad_operand_ok(dy) and _wgrad_operand_ok(x)
            and dy.shape[0] == x.shape[0] and _wgrad_rows_ok(dy.shape[0])):
        raise ValueError(
            "gemm_wgrad: needs bf16 GPU operands [M,N], [M,K] with M % 128 "
            "== 0, N % 256 == 0, K % 256 == 0 and 16-byte-aligned rows")
    if out is not None and not (_wgrad_operand_ok(out) and tuple(out.shape)
                                == (dy.shape[1], x.shape[1])):
        raise ValueError("gemm_wgrad: out must be a bf16 [N,K] GPU tensor "
                         "with 16-byte-aligned rows")
    return _K.gemm_wgrad(dy, x, out)


def gemm_wgrad_grouped(dy0: torch.Tensor, dy1: torch.Tensor,
                       x: torch.Tensor):
    """Two weight gradients that share x, one launch."""
    _require_ext("gemm_wgrad")
    if not (_wgrad_operand_ok(dy0) and _wgrad_operand_ok(dy1)
            and _wgrad_operand_ok(x) and dy0.shape == dy1.shape
            and dy0.stride(0) == dy1.stride(0)
            and dy0.shape[0] == x.shape[0] and _wgrad_rows_ok(x.shape[0])):
        raise ValueError("gemm_wgrad_grouped: operands do not qualify")
    o0, o1 = _K.gemm_wgrad_grouped(dy0, dy1, x)
    return o0, o1


def _wgrad_use_kernel(dy2, x2, problems=1) -> bool:
    return (_K is not None and _wgrad_switch_on()
            and _wgrad_listed(dy2.shape[1], x2.shape[1], problems)
            and _wgrad_operand_ok(dy2) and _wgrad_operand_ok(x2)
            and _wgrad_rows_ok(dy2.shape[0]))


def _wgrad(dy2: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
    if _wgrad_use_kernel(dy2, x2):
        return _K.gemm_wgrad(dy2, x2, None)
    return dy2.t() @ x2


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        return torch.nn.functional.linear(x, weight)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = dy @ weight
        if ctx.needs_input_grad[1]:
            dw = _wgrad(dy.reshape(-1, dy.shape[-1]),
                        x.reshape(-1, x.shape[-1]))
        return dx, dw


def _linear_custom(x, weight, bias=None) -> bool:
    return (bias is None and x.is_cuda and weight.is_cuda
            and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
            and weight.dim() == 2 and torch.is_grad_enabled()
            and _wgrad_switch_on())


def linear(x: torch.Tensor, weight: torch.Tensor, bias=None) -> torch.Tensor:
    """F.linear whose weight gradient runs on gemm_wgrad for the shapes
    listed in _WGRAD_TABLE. Everything else (CPU, non-bf16, bias, no
    grad, RAY_AMD_NO_WGRAD_GEMM=1, unlisted shapes) is plain F.linear."""
    if _linear_custom(x, weight, bias) and _wgrad_listed(*weight.shape):
        return _LinearFn.apply(x, weight)
    return torch.nn.functional.linear(x, weight, bias)


class Linear(torch.nn.Linear):
    """nn.Linear (same parameters, same state_dict) routed through
    `ops.linear`."""

    def forward(self, x):
        return linear(x, self.weight, self.bias)


# --------------------------------------------------------------------------
# Batched per-row LoRA (csrc/hip/lora.hip)
# --------------------------------------------------------------------------

LORA_RANKS = (16, 32, 64)


def lora_ref(y, x, A, B, scale, idx, dtype=torch.float64):
    """The rule, out of place: row m of the result is
    y[m] + scale[s] * (x[m] @ A[s].T) @ B[s].T with s = idx[m], and y[m]
    itself where idx[m] is -1 (such a row's x is not read). y [M, N],
    x [M, K], A [S, R, K], B [S, N, R], scale [S], idx [M] integers. The
    products are taken in `dtype`, which is also the result's."""
    out = y.to(dtype).clone()
    for s in idx.unique().tolist():
        if s < 0:
            continue
        rows = (idx == s).nonzero().flatten()
        h = x.index_select(0, rows).to(dtype) @ A[s].to(dtype).t()
        out.index_add_(0, rows,
                       (h @ B[s].to(dtype).t()) * scale[s].to(dtype))
    return out


def lora_add(y, x, A, B, scale, idx, split: int = 0):
    """y[m] += scale[s] * (x[m] @ A[s].T) @ B[s].T with s = idx[m], in
    place; returns y. bf16 GPU operands with grad off, R in LORA_RANKS,
    K % 128 == 0 and N % 128 == 0 run the two HIP kernels, which read idx on
    the device (`split` forces their number of K slices). Everything else
    (CPU, other dtypes or shapes) computes lora_ref in fp32 (fp64 for fp64
    operands) and copies it into y."""
    M, K = x.shape
    N, R = B.shape[1], B.shape[2]
    if (x.is_cuda and x.dtype == torch.bfloat16 and y.dtype == torch.bfloat16
            and A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16
            and not torch.is_grad_enabled() and R in LORA_RANKS
            and K % 128 == 0 and N % 128 == 0 and 1 <= M < 2 ** 22
            and x.is_contiguous() and y.is_contiguous()
            and x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0):
        _require_ext("lora_add")
        return _K.lora_add(y, x, A, B, scale, idx.int(), split)
    wide = torch.float64 if x.dtype == torch.float64 else torch.float32
    y.copy_(lora_ref(y, x, A, B, scale, idx, wide))
    return y


class LoraState:
    """What the LoraLinear modules of one model share: `idx`, the int32
    row -> adapter slot tensor of the current call (-1: no adapter), or
    None while no adapter is in play."""

    def __init__(self):
        self.idx = None


class LoraLinear(torch.nn.Module):
    """A projection (ops.Linear, LinearW8 or LinearW4) with `max_loras`
    adapter slots of rank `rank` on top: buffers lora_A [S, R, K], lora_B
    [S, N, R] and lora_scale [S], all zero until an adapter is copied in.
    forward is the base's, plus lora_add on the flattened rows while
    state.idx is set."""

    def __init__(self, base: torch.nn.Module, max_loras: int, rank: int,
                 state: "LoraState" = None):
        super().__init__()
        if rank not in LORA_RANKS:
            raise ValueError(f"LoRA rank must be one of {LORA_RANKS}")
        if not 1 <= max_loras <= 64:
            raise ValueError("max_loras must be 1..64")
        self.base = base
        self.in_features, self.out_features = (base.in_features,
                                               base.out_features)
        self.state = state if state is not None else LoraState()
        ref = next(iter((*base.parameters(), *base.buffers())))
        dtype = (ref.dtype if ref.dtype.is_floating_point
                 and ref.element_size() > 1 else torch.bfloat16)
        kw = {"device": ref.device, "dtype": dtype}
        self.register_buffer("lora_A", torch.zeros(
            max_loras, rank, self.in_features, **kw))
        self.register_buffer("lora_B", torch.zeros(
            max_loras, self.out_features, rank, **kw))
        self.register_buffer("lora_scale", torch.zeros(
            max_loras, device=ref.device, dtype=torch.float32))

    def add(self, y, x):
        """The adapters' part, added in place to y = base(x)."""
        idx = self.state.idx
        if idx is None:
            return y
        y2 = y.reshape(-1, self.out_features)
        x2 = x.reshape(-1, self.in_features)
        if not y2.is_contiguous() or y2.data_ptr() != y.data_ptr():
            raise ValueError("LoraLinear: the base's output must be "
                             "contiguous")
        lora_add(y2, x2.contiguous(), self.lora_A, self.lora_B,
                 self.lora_scale, idx)
        return y

    def forward(self, x):
        return self.add(self.base(x), x)


# --------------------------------------------------------------------------
# Mixture-of-experts FFN (csrc/hip/moe.hip)
# --------------------------------------------------------------------------

MOE_MAX_EXPERTS = 64
MOE_MAX_TOP_K = 8
MOE_MAX_ROWS = 65536
# Rows from which moe_ffn, outside graph capture, runs the per-expert
# hipBLASLt composition instead of the routed kernels (measured in
# tools/moe_bench.py, PERFORMANCE.md "Mixture of experts"). A captured step
# has at most 64 * (K + 1) rows and always runs the kernels.
MOE_COMPOSE_MIN_ROWS = 512
# The same threshold for MXFP4 expert weights (`scales` given): there the
# composition also pays one dequantise pass per chosen expert and projection.
# The kernels keep a row count only where their slowest repetition beat the
# composition's fastest in tools/moe_bench.py --weights mxfp4 (µs, Mixtral
# shapes, kernels' slowest / composition's fastest):
#   M = 256:   670.6 / 2569.5      M = 512:  1122.5 / 2751.4
#   M = 1024: 2392.8 / 3093.1      M = 1536: 3366.1 / 3382.6, and in another
#   run 3587.2 / 3366.7 (lost);    M = 2048: 4484.2 / 3679.2 (lost)
# so they keep every measured M up to 1024; 1536 is a tie that went both ways.
MOE_W4_COMPOSE_MIN_ROWS = 1025


def moe_route_ref(x, router_w, top_k: int, dtype=torch.float64):
    """The routing rule: logits x @ router_w.T in `dtype`, the top_k largest
    of a row (ties to the lower expert index, slot 0 the largest) and the
    softmax over those top_k logits. Returns idx [M, k] int32 and w [M, k]
    in `dtype` (fp32 when `dtype` is narrower)."""
    wide = dtype if dtype in (torch.float32, torch.float64) else torch.float32
    logits = x.to(wide) @ router_w.to(wide).t()
    # a stable descending sort keeps the lower index first among equals
    order = torch.sort(logits, dim=-1, descending=True, stable=True).indices
    idx = order[:, :top_k]
    w = torch.softmax(logits.gather(1, idx), dim=-1)
    return idx.int(), w


def _moe_expert_weights(e, dtype, w_gate, w_up, w_down, scales):
    """Expert e's three weights in `dtype`; with `scales` they are MXFP4 and
    only this expert is dequantised (exact; on the GPU in bf16 with grad off,
    one dequant_mxfp4 kernel pass each)."""
    if scales is None:
        return w_gate[e].to(dtype), w_up[e].to(dtype), w_down[e].to(dtype)
    if dtype == torch.bfloat16 and w_gate.is_cuda \
            and not torch.is_grad_enabled():
        _require_ext("dequant_mxfp4")
        return tuple(_K.dequant_mxfp4(wq[e], s[e])
                     for wq, s in zip((w_gate, w_up, w_down), scales))
    return tuple(dequantize_mxfp4(wq[e], s[e], dtype)
                 for wq, s in zip((w_gate, w_up, w_down), scales))


def moe_experts_ref(x, idx, w, w_gate, w_up, w_down, dtype=torch.float64,
                    scales=None):
    """y[m] = sum_j w[m, j] * (h_j @ w_down[e].T), h_j = silu(x[m] @
    w_gate[e].T) * (x[m] @ w_up[e].T), e = idx[m, j], one index_select ->
    matmul -> index_add_ per expert, in `dtype`. In float64 h is kept exact;
    otherwise h is rounded to bf16 once, like the kernels, and the result is
    returned unrounded in `dtype`. Entries of idx outside 0..E-1 add nothing.
    With `scales` the weights are MXFP4 (see moe_experts), dequantised one
    chosen expert at a time."""
    M, k = idx.shape
    E = w_gate.shape[0]
    xw = x.to(dtype)
    flat = idx.reshape(-1).long()
    out = torch.zeros(M, k, x.shape[1], dtype=dtype, device=x.device)
    pairs = out.view(M * k, -1)
    for e in range(E):
        p = (flat == e).nonzero().flatten()
        if p.numel() == 0:
            continue
        xe = xw.index_select(0, p // k)
        wg, wu, wd = _moe_expert_weights(e, dtype, w_gate, w_up, w_down,
                                         scales)
        h = torch.nn.functional.silu(xe @ wg.t()) * (xe @ wu.t())
        if dtype != torch.float64:
            h = h.bfloat16().to(dtype)
        pairs.index_add_(0, p, (h @ wd.t())
                         * w.reshape(-1)[p].to(dtype).unsqueeze(1))
    y = out[:, 0].clone()
    for j in range(1, k):  # slot order, as the combine kernel
        y += out[:, j]
    return y


def _moe_check(x, E, H, top_k, w_gate=None, w_up=None, w_down=None,
               scales=None):
    if x.dim() != 2 or x.shape[1] != H:
        raise ValueError(f"moe: x must be [M, {H}], got {tuple(x.shape)}")
    if not 1 <= x.shape[0] <= MOE_MAX_ROWS:
        raise ValueError(f"moe: 1 to {MOE_MAX_ROWS} rows, got {x.shape[0]}")
    if not 2 <= E <= MOE_MAX_EXPERTS:
        raise ValueError(f"moe: 2 to {MOE_MAX_EXPERTS} experts, got {E}")
    if not (1 <= top_k <= MOE_MAX_TOP_K and top_k <= E):
        raise ValueError(f"moe: top_k must be 1..{MOE_MAX_TOP_K} and at most "
                         f"the {E} experts, got {top_k}")
    if H % 128:
        raise ValueError(f"moe: hidden size {H} is not a multiple of 128")
    if w_gate is None:
        return
    I = w_gate.shape[1]
    if I % 128:
        raise ValueError(f"moe: expert width {I} is not a multiple of 128")
    if scales is not None:
        if len(scales) != 3:
            raise ValueError("moe: scales must be (s_gate, s_up, s_down)")
        want = ((E, I, H // 2), (E, I, H // 32), (E, I, H // 2),
                (E, I, H // 32), (E, H, I // 2), (E, H, I // 32))
        have = (w_gate, scales[0], w_up, scales[1], w_down, scales[2])
        if any(t.dtype != torch.uint8 or tuple(t.shape) != s
               for t, s in zip(have, want)):
            raise ValueError(
                "moe: with scales, w_gate and w_up must be uint8 [E, I, H/2] "
                "with scales [E, I, H/32] and w_down uint8 [E, H, I/2] with "
                "scales [E, H, I/32]")
        return
    if (tuple(w_gate.shape) != (E, I, H) or tuple(w_up.shape) != (E, I, H)
            or tuple(w_down.shape) != (E, H, I)):
        raise ValueError("moe: w_gate and w_up must be [E, I, H] and w_down "
                         "[E, H, I]")
    if not (x.dtype == w_gate.dtype == w_up.dtype == w_down.dtype):
        raise ValueError("moe: x and the expert weights must share a dtype")


def _moe_on_device(x) -> bool:
    return (x.is_cuda and x.dtype == torch.bfloat16
            and not torch.is_grad_enabled())


def moe_route(x, router_w, top_k: int, with_lists: bool = False):
    """idx [M, k] int32 and w [M, k] fp32 of moe_route_ref for x [M, H] and
    router_w [E, H]. bf16 GPU operands with grad off run moe_route_kernel;
    `with_lists` then also returns the per-expert pair lists the expert
    kernels read (None on the torch path). Everything else computes
    moe_route_ref in fp32 (fp64 for fp64 operands)."""
    if router_w.dim() != 2:
        raise ValueError("moe_route: router_w must be [E, H]")
    E, H = router_w.shape
    _moe_check(x, E, H, top_k)
    if x.dtype != router_w.dtype:
        raise ValueError("moe_route: x and router_w must share a dtype")
    if _moe_on_device(x):
        _require_ext("moe_route")
        idx, w, lists = _K.moe_route(x.contiguous(), router_w.contiguous(),
                                     top_k)
    else:
        wide = torch.float64 if x.dtype == torch.float64 else torch.float32
        idx, w = moe_route_ref(x, router_w, top_k, wide)
        lists = None
    return (idx, w, lists) if with_lists else (idx, w)


def _moe_compose(x, idx, w, w_gate, w_up, w_down, residual, scales=None):
    """The torch composition. Off the GPU: moe_experts_ref in fp32 (fp64 for
    fp64 operands), the kernels' rounding points. bf16 on the GPU with grad
    off (the large-M dispatch of moe_ffn): three bf16 hipBLASLt GEMMs per
    expert, which also round gate, up and the down product to bf16. MXFP4
    weights (`scales`) are dequantised to x's dtype one chosen expert at a
    time, so a bf16 copy of all the experts never exists."""
    if _moe_on_device(x):
        M, k = idx.shape
        flat = idx.reshape(-1).long()
        pairs = torch.zeros(M * k, x.shape[1], dtype=torch.float32,
                            device=x.device)
        for e in range(w_gate.shape[0]):
            p = (flat == e).nonzero().flatten()
            if p.numel() == 0:
                continue
            xe = x.index_select(0, p // k)
            wg, wu, wd = _moe_expert_weights(e, x.dtype, w_gate, w_up,
                                             w_down, scales)
            h = swiglu(xe @ wg.t(), xe @ wu.t())
            pairs.index_add_(0, p, (h @ wd.t()).float()
                             * w.reshape(-1)[p].unsqueeze(1))
        y = pairs.view(M, k, -1).sum(dim=1)
    else:
        wide = torch.float64 if x.dtype == torch.float64 else torch.float32
        y = moe_experts_ref(x, idx, w, w_gate, w_up, w_down, wide, scales)
    if residual is not None:
        y = y + residual.to(y.dtype)
    return y.to(x.dtype)


def _moe_dims(w_gate, scales):
    """(E, H) of expert weights [E, I, H], or of MXFP4 ones [E, I, H/2]."""
    return w_gate.shape[0], w_gate.shape[2] * (1 if scales is None else 2)


def moe_experts(x, idx, w, w_gate, w_up, w_down, residual=None, lists=None,
                scales=None, split=0):
    """The routed expert FFNs: moe_experts_ref for given idx [M, k] and
    w [M, k], plus `residual` [M, H], rounded once to x's dtype. bf16 GPU
    operands with grad off run the HIP kernels over `lists` (moe_route's;
    built from idx on the device when None). Everything else runs the torch
    composition with the same rounding points.

    With `scales=(s_gate, s_up, s_down)` the expert weights are MXFP4, as
    quantize_expert_weights_mxfp4 gives them: w_gate, w_up uint8 [E, I, H/2]
    with scales uint8 [E, I, H/32], w_down uint8 [E, H, I/2] with scales
    [E, H, I/32]. The kernels (csrc/hip/moe_w4.hip) read 17/32 byte per
    weight and compute with exactly the values dequantize_mxfp4 returns;
    `split` forces the K slices of the down kernel (1, 2, 4, 8; 0: by the
    shapes), which the result does not depend on."""
    if w_gate.dim() != 3:
        raise ValueError("moe_experts: w_gate must be [E, I, H]")
    E, H = _moe_dims(w_gate, scales)
    if idx.dim() != 2 or tuple(w.shape) != tuple(idx.shape) \
            or idx.shape[0] != x.shape[0]:
        raise ValueError("moe_experts: idx and w must be [M, k]")
    _moe_check(x, E, H, idx.shape[1], w_gate, w_up, w_down, scales)
    if residual is not None and (residual.shape != x.shape
                                 or residual.dtype != x.dtype):
        raise ValueError("moe_experts: residual must match x")
    if not _moe_on_device(x):
        return _moe_compose(x, idx, w, w_gate, w_up, w_down, residual, scales)
    _require_ext("moe_experts")
    idx = idx.int().contiguous()
    if lists is None:
        lists = _K.moe_align(idx, E)
    res = None if residual is None else residual.contiguous()
    if scales is not None:
        return _K.moe_experts_w4(
            x.contiguous(), idx, w.float().contiguous(), lists,
            w_gate.contiguous(), scales[0].contiguous(), w_up.contiguous(),
            scales[1].contiguous(), w_down.contiguous(),
            scales[2].contiguous(), res, split)
    return _K.moe_experts(
        x.contiguous(), idx, w.float().contiguous(), lists,
        w_gate.contiguous(), w_up.contiguous(), w_down.contiguous(), res)


def moe_ffn(x, router_w, w_gate, w_up, w_down, top_k: int, residual=None,
            scales=None, split=0):
    """moe_experts over moe_route: the whole mixture-of-experts FFN of
    x [M, H]. On the GPU the kernels serve every M inside a graph capture;
    outside one, M >= MOE_COMPOSE_MIN_ROWS (MOE_W4_COMPOSE_MIN_ROWS for
    MXFP4 weights, `scales` as in moe_experts) goes to the per-expert
    hipBLASLt composition (it reads the routing on the host)."""
    if w_gate.dim() != 3 or router_w.dim() != 2 \
            or router_w.shape[0] != w_gate.shape[0]:
        raise ValueError("moe_ffn: router_w [E, H] and w_gate [E, I, H]")
    idx, w, lists = moe_route(x, router_w, top_k, with_lists=True)
    min_rows = (MOE_COMPOSE_MIN_ROWS if scales is None
                else MOE_W4_COMPOSE_MIN_ROWS)
    if (lists is not None and x.shape[0] >= min_rows
            and not torch.cuda.is_current_stream_capturing()):
        _moe_check(x, *_moe_dims(w_gate, scales), top_k, w_gate, w_up,
                   w_down, scales)
        return _moe_compose(x, idx, w, w_gate, w_up, w_down, residual,
                            scales)
    return moe_experts(x, idx, w, w_gate, w_up, w_down, residual, lists,
                       scales, split)


class _SwigluMlpIn(torch.autograd.Function):
    """gate = x W_gate^T, up = x W_up^T. Backward: one grouped weight
    gradient launch (both share x). dx is the sum of the two dgrad GEMMs,
    each rounded to bf16, exactly what autograd computes for two linears
    (accumulating inside the second GEMM rounds once less; see
    PERFORMANCE.md for why that is not done)."""

    @staticmethod
    def forward(ctx, x, w_gate, w_up):
        ctx.save_for_backward(x, w_gate, w_up)
        return (torch.nn.functional.linear(x, w_gate),
                torch.nn.functional.linear(x, w_up))

    @staticmethod
    def backward(ctx, d_gate, d_up):
        x, w_gate, w_up = ctx.saved_tensors
        dg2 = d_gate.reshape(-1, d_gate.shape[-1])
        du2 = d_up.reshape(-1, d_up.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        dx = dwg = dwu = None
        if ctx.needs_input_grad[0]:
            dx = (dg2 @ w_gate + du2 @ w_up).view(x.shape)
        need_g, need_u = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if (need_g and need_u and dg2.stride() == du2.stride()
                and _wgrad_use_kernel(dg2, x2, 2)
                and _wgrad_operand_ok(du2)):
            dwg, dwu = _K.gemm_wgrad_grouped(dg2, du2, x2)
        else:
            if need_g:
                dwg = _wgrad(dg2, x2)
            if need_u:
                dwu = _wgrad(du2, x2)
        return dx, dwg, dwu


def swiglu_mlp_in(x: torch.Tensor, w_gate: torch.Tensor,
                  w_up: torch.Tensor):
    """The two input projections of a SwiGLU MLP -> (gate, up)."""
    if (_linear_custom(x, w_gate) and _linear_custom(x, w_up)
            and w_gate.shape == w_up.shape):
        return _SwigluMlpIn.apply(x, w_gate, w_up)
    return linear(x, w_gate), linear(x, w_up)


# --------------------------------------------------------------------------
# Cross entropy (fused, bf16 logits)
# --------------------------------------------------------------------------


def cross_entropy_ref(logits: torch.Tensor, target: torch.Tensor):
    return torch.nn.functional.cross_entropy(
        logits.float(), target.long(), ignore_index=-100, reduction="mean"
    )


class _FusedCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        _require_ext("cross_entropy")
        logits = logits.contiguous()
        t32 = target.to(torch.int32).contiguous()
        loss, mx, lse = _K.ce_fwd(logits, t32)
        nvalid = (t32 >= 0).sum().clamp(min=1)
        ctx.save_for_backward(logits, t32, mx, lse, nvalid)
        return loss.sum() / nvalid.float()

    @staticmethod
    def backward(ctx, dloss):
        logits, t32, mx, lse, nvalid = ctx.saved_tensors
        per_row = (dloss / nvalid.float()).expand(logits.size(0)).contiguous()
        dl = _K.ce_bwd(logits, t32, mx, lse, per_row)
        return dl, None


def cross_entropy(logits: torch.Tensor, target: torch.Tensor):
    """Mean CE over rows where target != -100. logits [N, V] bf16.

    Every negative target counts as ignored; an all-ignored batch gives
    loss 0 and zero gradient (the row count is clamped to 1). A target
    >= V is not checked on the GPU: the kernel reads logits[row, target]
    out of bounds. Guarding it needs a host sync, so the caller must
    pass targets in [0, V) or negative."""
    if not logits.is_cuda:
        return cross_entropy_ref(logits, target)
    return _FusedCE.apply(logits, target)


class _ChunkedLmHeadCE(torch.autograd.Function):
    """Fused lm_head + cross entropy, row-chunked: the [N, V] logits
    are never materialized whole (N=B*T=32k, V=128k bf16 = 8.4 GB at
    the flagship shape — plus its stored-activation copy). Forward
    computes the loss per chunk; backward RECOMPUTES each chunk's
    logits and uses the fused CE kernels for dlogits, folding straight
    into dX and a fp32 dW accumulator. Costs one extra lm_head GEMM,
    saves ~15 GB peak (headroom for larger micro-batches)."""

    @staticmethod
    def forward(ctx, x, weight, target, chunk_rows):
        _require_ext("cross_entropy")
        x = x.contiguous()
        t32 = target.to(torch.int32).contiguous()
        N = x.shape[0]
        nvalid = (t32 >= 0).sum().clamp(min=1)
        loss_sum = torch.zeros((), dtype=torch.float32, device=x.device)
        for s in range(0, N, chunk_rows):
            e = min(s + chunk_rows, N)
            logits = (x[s:e] @ weight.t()).contiguous()
            l, mx, lse = _K.ce_fwd(logits, t32[s:e])
            loss_sum += l.sum()
        ctx.save_for_backward(x, weight, t32, nvalid)
        ctx.chunk = chunk_rows
        return loss_sum / nvalid.float()

    @staticmethod
    def backward(ctx, dloss):
        x, w, t32, nvalid = ctx.saved_tensors
        N = x.shape[0]
        chunk = ctx.chunk
        dx = torch.empty_like(x)
        dw_acc = torch.zeros_like(w, dtype=torch.float32)
        scale = dloss / nvalid.float()
        for s in range(0, N, chunk):
            e = min(s + chunk, N)
            logits = (x[s:e] @ w.t()).contiguous()
            _, mx, lse = _K.ce_fwd(logits, t32[s:e])
            per_row = scale.expand(e - s).contiguous()
            dl = _K.ce_bwd(logits, t32[s:e], mx, lse, per_row)
            dx[s:e] = dl @ w
            dw_acc += (dl.t() @ x[s:e]).float()
        return dx, dw_acc.to(w.dtype), None, None


def lm_head_cross_entropy(x: torch.Tensor, weight: torch.Tensor,
                          target: torch.Tensor,
                          chunk_rows: int = 8192) -> torch.Tensor:
    """Chunked fused projection + CE; x [N, H] bf16, weight [V, H]."""
    if not x.is_cuda:
        return cross_entropy_ref(x.float() @ weight.t().float(), target)
    return _ChunkedLmHeadCE.apply(x, weight, target, chunk_rows)


# --------------------------------------------------------------------------
# Fused AdamW
# --------------------------------------------------------------------------


class FusedAdamW:
    """AdamW with fp32 states (+ fp32 master weights for bf16 params),
    one fused HIP kernel launch per tensor. CPU fallback uses torch ops."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.95), eps=1e-8,
                 weight_decay=0.1):
        self.params = [p for p in params if p.requires_grad]
        self.lr = lr
        self.beta1, self.beta2 = betas
        self.eps = eps
        self.wd = weight_decay
        self.t = 0
        self.state = {}
        for p in self.params:
            st = {"m": torch.zeros_like(p, dtype=torch.float32),
                  "v": torch.zeros_like(p, dtype=torch.float32)}
            if p.dtype == torch.bfloat16:
                st["master"] = p.detach().float().clone()
            self.state[id(p)] = st

    @property
    def param_groups(self):
        return [{"params": self.params, "lr": self.lr}]

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0):
        self.t += 1
        for p in self.params:
            if p.grad is None:
                continue
            st = self.state[id(p)]
            if p.is_cuda:
                _require_ext("adamw")
                _K.adamw_step(
                    p.data, p.grad.contiguous(), st["m"], st["v"],
                    st.get("master", st["m"]), self.lr, self.beta1,
                    self.beta2, self.eps, self.wd, self.t, grad_scale,
                )
            else:
                g = p.grad.float() * grad_scale
                st["m"].mul_(self.beta1).add_(g, alpha=1 - self.beta1)
                st["v"].mul_(self.beta2).addcmul_(g, g, value=1 - self.beta2)
                bc1 = 1 - self.beta1 ** self.t
                bc2 = 1 - self.beta2 ** self.t
                pf = st.get("master", None)
                if pf is None:
                    pf = p.data.float()
                upd = (st["m"] / bc1) / ((st["v"] / bc2).sqrt() + self.eps)
                pf -= self.lr * (upd + self.wd * pf)
                if "master" in st:
                    p.data.copy_(pf.to(p.dtype))
                else:
                    p.data.copy_(pf)

    def state_dict(self):
        return {"t": self.t, "lr": self.lr}

    def load_state_dict(self, sd):
        self.t = sd.get("t", 0)
        self.lr = sd.get("lr", self.lr)


# --------------------------------------------------------------------------
# RL scans
# --------------------------------------------------------------------------


def gae_ref(rewards, values, cont, gamma, lam):
    """rewards/cont [T,B] fp32, values [T+1,B]. Returns (adv, vtarg)."""
    T, B = rewards.shape
    adv = torch.zeros_like(rewards)
    running = torch.zeros(B, dtype=rewards.dtype)
    for t in reversed(range(T)):
        delta = rewards[t] + gamma * cont[t] * values[t + 1] - values[t]
        running = delta + gamma * lam * cont[t] * running
        adv[t] = running
    return adv, adv + values[:-1]


def gae(rewards, values, cont, gamma=0.99, lam=0.95):
    if not rewards.is_cuda:
        return gae_ref(rewards, values, cont, gamma, lam)
    _require_ext("gae")
    out = _K.gae(rewards.contiguous(), values.contiguous(),
                 cont.contiguous(), gamma, lam)
    return out[0], out[1]


def vtrace_ref(log_rhos, rewards, values, cont, gamma, rho_clip=1.0,
               c_clip=1.0, rho_pg_clip=1.0):
    """Reference recursion (cf. vtrace_torch_v2.py:73 semantics)."""
    T, B = rewards.shape
    rhos = log_rhos.exp()
    rho = rhos.clamp(max=rho_clip)
    cs = rhos.clamp(max=c_clip)
    vs = torch.zeros_like(rewards)
    diff = torch.zeros(B, dtype=rewards.dtype)
    for t in reversed(range(T)):
        delta = rho[t] * (rewards[t] + gamma * cont[t] * values[t + 1] - values[t])
        cur = delta + gamma * cont[t] * cs[t] * diff
        vs[t] = values[t] + cur
        diff = cur
    pg = torch.zeros_like(rewards)
    for t in range(T):
        vs_next = values[t + 1] if t == T - 1 else vs[t + 1]
        pg[t] = rhos[t].clamp(max=rho_pg_clip) * (
            rewards[t] + gamma * cont[t] * vs_next - values[t]
        )
    return vs, pg


def vtrace(log_rhos, rewards, values, cont, gamma=0.99, rho_clip=1.0,
           c_clip=1.0, rho_pg_clip=1.0):
    if not rewards.is_cuda:
        return vtrace_ref(log_rhos, rewards, values, cont, gamma, rho_clip,
                          c_clip, rho_pg_clip)
    _require_ext("vtrace")
    out = _K.vtrace(log_rhos.contiguous(), rewards.contiguous(),
                    values.contiguous(), cont.contiguous(), gamma,
                    rho_clip, c_clip, rho_pg_clip)
    return out[0], out[1]


# --------------------------------------------------------------------------
# Image normalize (Data preprocessing)
# --------------------------------------------------------------------------


def img_normalize_ref(x_u8, mean, std):
    xf = x_u8.float() / 255.0
    out = (xf - mean.view(1, 1, 1, -1)) / std.view(1, 1, 1, -1)
    return out.permute(0, 3, 1, 2).contiguous().bfloat16()


def img_normalize(x_u8: torch.Tensor, mean: torch.Tensor, std: torch.Tensor):
    """uint8 NHWC -> bf16 NCHW normalized."""
    if not x_u8.is_cuda:
        return img_normalize_ref(x_u8, mean, std)
    _require_ext("img_normalize")
    return _K.img_normalize(
        x_u8.contiguous(), mean.float().contiguous(),
        (1.0 / std.float()).contiguous()
    )


# --------------------------------------------------------------------------
# Flash attention (fused CDNA4 forward with LSE output, and backward)
# --------------------------------------------------------------------------


def flash_attention_ref(q, k, v, causal=True):
    """fp32 reference; q [B,Hq,T,D], k/v [B,Hkv,Tk,D] (GQA)."""
    import math

    B, Hq, T, D = q.shape
    Hkv = k.shape[1]
    rep = Hq // Hkv
    kf = k.float().repeat_interleave(rep, dim=1)
    vf = v.float().repeat_interleave(rep, dim=1)
    s = torch.matmul(q.float(), kf.transpose(-1, -2)) / math.sqrt(D)
    if causal:
        Tk = k.shape[2]
        mask = torch.ones(T, Tk, dtype=torch.bool, device=q.device).tril_(
            Tk - T
        )
        s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    out = torch.matmul(torch.softmax(s, -1), vf)
    return out.to(q.dtype), lse


def _is_bthd_view(t, wide=False):
    """[B,H,T,D] tensor that is a transpose view of [B,T,H,D] storage
    (the model's natural post-RoPE layout) — the kernels read it
    directly, no transpose-contiguous copy. With `wide`, the token row may
    be wider than H*D: strides (T*rs, D, rs, 1) with rs >= H*D, as the q,
    k and v column sections of one packed [B,T,(Hq+2Hkv)*D] GEMM output
    have. A wider row must keep every head vector 16-byte aligned
    (rs % 8 == 0 and an aligned start) and inside the kernels' 32-bit
    staging offsets (the same bounds as csrc/ops.hip attn_layout)."""
    B, H, T, D = t.shape
    st = t.stride()
    rs = st[2]
    if not (st[3] == 1 and st[1] == D and st[0] == T * rs):
        return False
    if rs == H * D:
        return True
    return (wide and rs > H * D and rs % 8 == 0
            and t.data_ptr() % 16 == 0
            and T * rs < 2 ** 31 and 64 * rs < 2 ** 30)


def _attn_operands(q, k, v):
    """q, k, v in a layout the kernels read, and whether that is the BTHD
    view: the tensors as they are if T % 256 == 0 and all three are BTHD
    views, wide rows included, k and v at one row stride (only the 256-row
    kernels read those), else contiguous copies."""
    if q.shape[2] % 256 == 0 and _is_bthd_view(q, True) \
            and _is_bthd_view(k, True) and _is_bthd_view(v, True) \
            and k.stride(2) == v.stride(2):
        return q, k, v, True
    return q.contiguous(), k.contiguous(), v.contiguous(), False


class _FlashAttnFn(torch.autograd.Function):
    """Training flash attention: HIP forward with LSE, then the prep, dQ
    and dK/dV backward kernels (csrc/ops.hip picks the 256-row or the
    128-row set from T). Requires T == Tk, T % 128 == 0, D == 128 (the
    Llama training shape)."""

    @staticmethod
    def forward(ctx, q, k, v, causal):
        qc, kc, vc, bthd = _attn_operands(q, k, v)
        out, lse = _K.flash_attn_fwd(qc, kc, vc, causal, 0, True)
        ctx.save_for_backward(qc, kc, vc, out, lse)
        ctx.causal = causal
        ctx.bthd = bthd
        return out

    @staticmethod
    def backward(ctx, d_out):
        q, k, v, out, lse = ctx.saved_tensors
        if ctx.bthd:
            if not _is_bthd_view(d_out):
                d_out = d_out.transpose(1, 2).contiguous().transpose(1, 2)
        else:
            d_out = d_out.contiguous()
        dq, dk, dv = _K.flash_attn_bwd(
            q, k, v, out, d_out, lse, ctx.causal
        )
        return dq, dk, dv, None


def flash_attention(q, k, v, causal: bool = True, q_offset: int = 0,
                    return_lse: bool = False):
    """Fused CDNA4 flash attention. q [B,Hq,T,128] bf16 (GQA k/v
    [B,Hkv,Tk,128]). Inference pads T to 128 internally; the
    differentiable path (any input requires_grad) additionally needs
    T == Tk and T % 128 == 0 and supports backward via the HIP
    fa_bwd kernels."""
    if not q.is_cuda:
        out, lse = flash_attention_ref(q, k, v, causal)
        return (out, lse) if return_lse else out
    _require_ext("flash_attention")
    B, Hq, T, D = q.shape
    needs_grad = torch.is_grad_enabled() and (
        q.requires_grad or k.requires_grad or v.requires_grad
    )
    if needs_grad:
        if return_lse or q_offset:
            raise NotImplementedError(
                "flash_attention backward does not support return_lse/"
                "q_offset (ring attention calls the backward kernels "
                "itself, see ray_amd/parallel/sequence.py)"
            )
        if T % 128 != 0 or T != k.shape[2]:
            raise NotImplementedError(
                "flash_attention backward requires T == Tk and "
                "T % 128 == 0"
            )
        return _FlashAttnFn.apply(q, k, v, causal)
    pad = (-T) % 128
    if pad:
        q = torch.nn.functional.pad(q, (0, 0, 0, pad))
    # a padded q is a contiguous copy, never a BTHD view
    qc, kc, vc, _ = _attn_operands(q, k, v)
    r = _K.flash_attn_fwd(qc, kc, vc, causal, q_offset, return_lse)
    out = r[0][:, :, :T] if pad else r[0]
    if return_lse:
        lse = r[1][:, :, :T] if pad else r[1]
        return out, lse
    return out


# test hook: False sends Attention.forward back to split + rope + flash
# attention (for monkeypatch, like _WGRAD_FORCE)
_FUSED_QKV_ATTN = True


def _qkv_sections(qkv, n_heads, n_kv_heads):
    """The q, k, v column sections of packed [B,T,(Hq+2Hkv)*D] as
    [B,H,T,D] views."""
    B, T, W = qkv.shape
    D = W // (n_heads + 2 * n_kv_heads)
    q, k, v = qkv.split([n_heads * D, n_kv_heads * D, n_kv_heads * D], dim=-1)
    return (q.view(B, T, n_heads, D).transpose(1, 2),
            k.view(B, T, n_kv_heads, D).transpose(1, 2),
            v.view(B, T, n_kv_heads, D).transpose(1, 2))


def _qkv_packed_ok(qkv, n_heads, n_kv_heads):
    """Whether the fused path reads this packed buffer as it is."""
    if not (_K is not None and qkv.is_cuda and qkv.dtype == torch.bfloat16
            and qkv.dim() == 3 and qkv.shape[1] % 256 == 0
            and qkv.shape[2] == (n_heads + 2 * n_kv_heads) * 128
            and n_heads % n_kv_heads == 0
            and qkv.stride(2) == 1
            and qkv.stride(0) == qkv.shape[1] * qkv.stride(1)
            and not qkv._is_view()):
        return False
    return all(_is_bthd_view(t, True)
               for t in _qkv_sections(qkv, n_heads, n_kv_heads))


class _QkvRopeAttn(torch.autograd.Function):
    """RoPE in place on the q and k sections of the packed projection
    output, flash attention on the three section views; backward writes
    dq, dk, dv into one packed buffer and un-rotates it in place."""

    @staticmethod
    def forward(ctx, qkv, cosT, sinT, n_heads, n_kv_heads):
        ctx.set_materialize_grads(False)
        _K.rope_qk_inplace(qkv, cosT, sinT, n_heads, n_kv_heads, 1)
        ctx.mark_dirty(qkv)
        q, k, v = _qkv_sections(qkv, n_heads, n_kv_heads)
        out, lse = _K.flash_attn_fwd(q, k, v, True, 0, True)
        ctx.save_for_backward(qkv, out, lse, cosT, sinT)
        ctx.heads = (n_heads, n_kv_heads)
        # a tensor written in place has to be an output as well
        return out, qkv

    @staticmethod
    def backward(ctx, d_out, d_rot):
        qkv, out, lse, cosT, sinT = ctx.saved_tensors
        n_heads, n_kv_heads = ctx.heads
        if d_rot is not None:
            raise NotImplementedError(
                "qkv_rope_attention: the rotated buffer is not an output")
        q, k, v = _qkv_sections(qkv, n_heads, n_kv_heads)
        if not _is_bthd_view(d_out):
            d_out = d_out.transpose(1, 2).contiguous().transpose(1, 2)
        d_qkv = torch.empty(qkv.shape, dtype=qkv.dtype, device=qkv.device)
        _K.flash_attn_bwd(q, k, v, out, d_out, lse, True, d_qkv)
        _K.rope_qk_inplace(d_qkv, cosT, sinT, n_heads, n_kv_heads, -1)
        return d_qkv, None, None, None, None


def qkv_rope_attention(qkv, cosT, sinT, n_heads, n_kv_heads):
    """Causal self-attention from the packed projection output
    qkv [B,T,(Hq+2Hkv)*D] (q heads, k heads, v heads along the last
    dimension) with RoPE on q and k; returns [B,T,Hq*D]. On the GPU, for
    bf16, D == 128 and T % 256 == 0, qkv is rotated IN PLACE and the
    kernels read and write the packed layout; anything else runs split,
    `rope` and `flash_attention`."""
    B, T, W = qkv.shape
    D = W // (n_heads + 2 * n_kv_heads)
    cosT, sinT = cosT[:T], sinT[:T]
    if (_FUSED_QKV_ATTN and _qkv_packed_ok(qkv, n_heads, n_kv_heads)
            and cosT.is_contiguous() and sinT.is_contiguous()
            and cosT.data_ptr() % 16 == 0 and sinT.data_ptr() % 16 == 0):
        out, _ = _QkvRopeAttn.apply(qkv, cosT, sinT, n_heads, n_kv_heads)
        return out.transpose(1, 2).reshape(B, T, n_heads * D)
    q, k, v = qkv.split([n_heads * D, n_kv_heads * D, n_kv_heads * D], dim=-1)
    v = v.reshape(B, T, n_kv_heads, D)
    q = rope(q.view(B, T, n_heads, D), cosT, sinT).transpose(1, 2)
    k = rope(k.view(B, T, n_kv_heads, D), cosT, sinT).transpose(1, 2)
    v = v.contiguous().transpose(1, 2)
    out = flash_attention(q, k, v, causal=True)
    return out.transpose(1, 2).reshape(B, T, n_heads * D)


# --------------------------------------------------------------------------
# Paged-KV decode attention (serving; csrc/hip/paged_attn.hip)
# --------------------------------------------------------------------------

PAGE_SIZE = 16
FP8_MAX = 448.0  # largest finite float8_e4m3fn


def _check_kv_scale(scale) -> float:
    scale = float(scale)
    if not (scale > 0.0 and scale != float("inf")):
        raise ValueError(f"KV cache scale must be positive and finite, got "
                         f"{scale!r}")
    return scale


def quantize_kv_fp8(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """The fp8 KV-cache storage rule, in plain torch:
    e4m3fn_rne(clamp(fp32(x) * fp32(1/scale), -448, 448)). The clamp is
    explicit and comes first, so nothing depends on how the conversion
    treats overflow (a bare .to(float8_e4m3fn) gives NaN above 464). The
    stored value dequantises as stored.float() * scale."""
    scale = _check_kv_scale(scale)
    # a 0-d fp32 tensor: the multiply is an fp32 multiply on every backend
    inv = torch.tensor(1.0 / scale, dtype=torch.float32, device=x.device)
    y = (x.float() * inv).clamp(-FP8_MAX, FP8_MAX)
    return y.to(torch.float8_e4m3fn)


def _to_kv_cache(x: torch.Tensor, cache: torch.Tensor, scale: float):
    """x as the elements `cache` stores."""
    if cache.dtype == torch.float8_e4m3fn:
        return quantize_kv_fp8(x, scale)
    return x.to(cache.dtype)


def paged_attention_ref(q, k_cache, v_cache, block_table, seq_lens,
                        k_scale=1.0, v_scale=1.0):
    """fp32 reference. q [B,Hq,D]; k_cache/v_cache
    [num_pages,Hkv,page,D]; block_table [B,max_pages]; seq_lens [B].
    Gathers each row's pages, slices to seq_len, GQA by
    repeat_interleave. Rows with seq_len 0 give zeros. Cache values are
    cache.float() * scale (the fp8 pools' dequantisation)."""
    import math

    B, Hq, D = q.shape
    _, Hkv, page, _ = k_cache.shape
    rep = Hq // Hkv
    out = torch.zeros(B, Hq, D, dtype=torch.float32, device=q.device)
    lens = seq_lens.tolist()
    for b in range(B):
        n = int(lens[b])
        if n <= 0:
            continue
        pages = block_table[b, : (n + page - 1) // page].long()
        # [P,Hkv,page,D] -> [Hkv, P*page, D]
        k = k_cache[pages].permute(1, 0, 2, 3).reshape(Hkv, -1, D)[:, :n]
        v = v_cache[pages].permute(1, 0, 2, 3).reshape(Hkv, -1, D)[:, :n]
        kf = (k.float() * k_scale).repeat_interleave(rep, dim=0)
        vf = (v.float() * v_scale).repeat_interleave(rep, dim=0)
        s = torch.einsum("hd,htd->ht", q[b].float(), kf) / math.sqrt(D)
        out[b] = torch.einsum("ht,htd->hd", torch.softmax(s, -1), vf)
    return out.to(q.dtype)


def default_num_splits(B: int, Hkv: int, max_len: int, device=None) -> int:
    """KV splits so that B*Hkv*splits is one to two times the CU count,
    capped at one split per 256 tokens of the longest possible row."""
    cus = 256
    if torch.cuda.is_available():
        cus = torch.cuda.get_device_properties(
            device if device is not None else 0
        ).multi_processor_count
    # two blocks per CU when the split count allows it: each SIMD then
    # holds two waves, and one wave's loads hide the other's math
    want = (2 * cus) // max(1, B * Hkv)
    return max(1, min(want, -(-max_len // 256)))


def paged_attention_decode(q, k_cache, v_cache, block_table, seq_lens,
                           num_splits=None, workspace=None, k_scale=1.0,
                           v_scale=1.0):
    """Single-token attention over a paged KV cache. q [B,Hq,D] ->
    [B,Hq,D]. num_splits=None picks a value from the block table's
    capacity (no host sync on seq_lens); graph-capturing callers pass a
    fixed value and may pass a static fp32 `workspace` of
    B*Hq*num_splits*(D+2) elements. The caches are bf16, or
    float8_e4m3fn holding value / scale (see quantize_kv_fp8)."""
    if not q.is_cuda:
        return paged_attention_ref(q, k_cache, v_cache, block_table,
                                   seq_lens, k_scale, v_scale)
    _require_ext("paged_attention_decode")
    if num_splits is None:
        num_splits = default_num_splits(
            q.shape[0], k_cache.shape[1],
            block_table.shape[1] * k_cache.shape[2], q.device)
    return _K.paged_attn_decode(q, k_cache, v_cache, block_table, seq_lens,
                                int(num_splits), workspace, float(k_scale),
                                float(v_scale))


def rope_append_paged_ref(q, k, v, cosT, sinT, pos, block_table, k_cache,
                          v_cache, k_scale=1.0, v_scale=1.0):
    """Reference for rope_append_paged: rotate-halves RoPE of q/k at
    each row's own position (fp32 tables), rotated k and raw v written
    in place into page block_table[b, pos//page] slot pos%page; rows
    with pos < 0 are skipped (zero q_rot). fp8 caches store
    quantize_kv_fp8 of the rotated k (rounded to k's dtype first) and of
    v. Returns q_rot [B,Hq,D]."""
    B, Hq, D = q.shape
    page = k_cache.shape[2]
    q_rot = torch.zeros(B, Hq, D, dtype=q.dtype, device=q.device)
    for b, p in enumerate(pos.tolist()):
        if p < 0:
            continue
        c, s = cosT[p : p + 1], sinT[p : p + 1]
        q_rot[b] = rope_ref(q[b].reshape(1, 1, Hq, D), c, s)[0, 0]
        pg = int(block_table[b, p // page])
        k_cache[pg, :, p % page] = _to_kv_cache(
            rope_ref(k[b].reshape(1, 1, -1, D), c, s)[0, 0], k_cache, k_scale)
        v_cache[pg, :, p % page] = _to_kv_cache(v[b], v_cache, v_scale)
    return q_rot


def rope_append_paged(q, k, v, cosT, sinT, pos, block_table, k_cache,
                      v_cache, k_scale=1.0, v_scale=1.0):
    """Fused decode-step RoPE + paged KV append (one launch). q
    [B,Hq,D], k/v [B,Hkv,D] (fused-QKV slices accepted as they are),
    pos [B] int32. Updates k_cache/v_cache in place, returns rotated
    q."""
    if not q.is_cuda:
        return rope_append_paged_ref(q, k, v, cosT, sinT, pos, block_table,
                                     k_cache, v_cache, k_scale, v_scale)
    _require_ext("rope_append_paged")
    return _K.rope_append_paged(q, k, v, cosT, sinT, pos, block_table,
                                k_cache, v_cache, float(k_scale),
                                float(v_scale))


def kv_append_paged_ref(k, v, pos0, block_table_row, k_cache, v_cache,
                        k_scale=1.0, v_scale=1.0):
    """Reference for kv_append_paged: rows k[t], v[t] of [T,Hkv,D] (k
    already rotated) are written in place to cache row pos0 + t of the
    pages in block_table_row [max_pages], quantised by quantize_kv_fp8
    when the cache is fp8. Rows whose page index is past the table, or
    whose page id is outside the pool, are not written."""
    page = k_cache.shape[2]
    num_pages = k_cache.shape[0]
    table = block_table_row.tolist()
    for t in range(k.shape[0]):
        p = int(pos0) + t
        if p // page >= len(table):
            continue
        pg = int(table[p // page])
        if pg < 0 or pg >= num_pages:
            continue
        k_cache[pg, :, p % page] = _to_kv_cache(k[t], k_cache, k_scale)
        v_cache[pg, :, p % page] = _to_kv_cache(v[t], v_cache, v_scale)


def kv_append_paged(k, v, pos0, block_table_row, k_cache, v_cache,
                    k_scale=1.0, v_scale=1.0):
    """Append T already-rotated K rows and V rows [T,Hkv,D] of one
    sequence at cache rows pos0 .. pos0+T-1 (one launch). Updates the
    caches in place."""
    if not k.is_cuda:
        return kv_append_paged_ref(k, v, pos0, block_table_row, k_cache,
                                   v_cache, k_scale, v_scale)
    _require_ext("kv_append_paged")
    _K.kv_append_paged(k, v, int(pos0), block_table_row, k_cache, v_cache,
                       float(k_scale), float(v_scale))


# --------------------------------------------------------------------------
# Paged-KV prefill attention (serving; csrc/hip/paged_attn_prefill.hip)
# --------------------------------------------------------------------------


def paged_attention_prefill_ref(q, k_cache, v_cache, block_table, ctx_lens,
                                q_lens, k_scale=1.0, v_scale=1.0):
    """fp32 reference. q [B,Tq,Hq,D] is a chunk of queries at positions
    ctx_lens[b] .. ctx_lens[b]+Tq-1 whose own K/V are already in the
    pages. Gathers each row's pages as paged_attention_ref does, then
    masks causally with the ctx offset: query row i sees cache rows
    j <= ctx_lens[b] + i. Rows i >= q_lens[b] are zeros."""
    import math

    B, Tq, Hq, D = q.shape
    _, Hkv, page, _ = k_cache.shape
    rep = Hq // Hkv
    out = torch.zeros(B, Tq, Hq, D, dtype=torch.float32, device=q.device)
    ctxs, qls = ctx_lens.tolist(), q_lens.tolist()
    for b in range(B):
        ctx, n = int(ctxs[b]), min(int(qls[b]), Tq)
        if n <= 0:
            continue
        L = ctx + n
        pages = block_table[b, : (L + page - 1) // page].long()
        # [P,Hkv,page,D] -> [Hkv, P*page, D]
        k = k_cache[pages].permute(1, 0, 2, 3).reshape(Hkv, -1, D)[:, :L]
        v = v_cache[pages].permute(1, 0, 2, 3).reshape(Hkv, -1, D)[:, :L]
        kf = (k.float() * k_scale).repeat_interleave(rep, dim=0)
        vf = (v.float() * v_scale).repeat_interleave(rep, dim=0)
        s = torch.einsum("thd,hjd->htj", q[b, :n].float(), kf) / math.sqrt(D)
        i = torch.arange(n, device=q.device).view(n, 1)
        j = torch.arange(L, device=q.device).view(1, L)
        s = s.masked_fill(j > ctx + i, float("-inf"))
        out[b, :n] = torch.einsum("htj,hjd->thd", torch.softmax(s, -1), vf)
    return out.to(q.dtype)


def paged_attention_prefill(q, k_cache, v_cache, block_table, ctx_lens,
                            q_lens, k_scale=1.0, v_scale=1.0):
    """Causal attention from a chunk of query tokens to a paged KV
    cache. q [B,Tq,Hq,D] bf16 contiguous -> [B,Tq,Hq,D]; ctx_lens [B]
    int32 rows cached before the chunk, q_lens [B] int32 valid query
    rows. The chunk's K/V must already be appended to the pages."""
    if not q.is_cuda:
        return paged_attention_prefill_ref(q, k_cache, v_cache, block_table,
                                           ctx_lens, q_lens, k_scale, v_scale)
    _require_ext("paged_attention_prefill")
    return _K.paged_attn_prefill(q, k_cache, v_cache, block_table, ctx_lens,
                                 q_lens, float(k_scale), float(v_scale))


# --------------------------------------------------------------------------
# Paged-KV verify attention for speculative decoding
# (csrc/hip/paged_attn_verify.hip)
# --------------------------------------------------------------------------

# Tq * (Hq // Hkv) of one verify call: the query columns of one MFMA tile
VERIFY_MAX_ROWS = 32


def paged_attention_verify(q, k_cache, v_cache, block_table, ctx_lens,
                           q_lens, num_splits=None, workspace=None,
                           k_scale=1.0, v_scale=1.0):
    """Causal attention from a few query tokens per sequence (a verify
    step's last token and drafts) to a paged KV cache, split over KV like
    paged_attention_decode. Semantics, shapes and reference are those of
    paged_attention_prefill (the CPU path is paged_attention_prefill_ref);
    Tq * (Hq // Hkv) <= VERIFY_MAX_ROWS. num_splits=None picks a value from
    the block table's capacity; graph-capturing callers pass a fixed value
    and, for num_splits > 1, a static fp32 `workspace` of
    B*Tq*Hq*num_splits*(D+2) elements."""
    if not q.is_cuda:
        return paged_attention_prefill_ref(q, k_cache, v_cache, block_table,
                                           ctx_lens, q_lens, k_scale, v_scale)
    _require_ext("paged_attention_verify")
    if num_splits is None:
        num_splits = default_num_splits(
            q.shape[0], k_cache.shape[1],
            block_table.shape[1] * k_cache.shape[2], q.device)
    return _K.paged_attn_verify(q, k_cache, v_cache, block_table, ctx_lens,
                                q_lens, int(num_splits), workspace,
                                float(k_scale), float(v_scale))


def rope_append_paged_multi_ref(q, k, v, cosT, sinT, pos0, q_lens,
                                block_table, k_cache, v_cache, k_scale=1.0,
                                v_scale=1.0):
    """Reference for rope_append_paged_multi: rope_append_paged_ref row by
    row, token i of sequence b at position pos0[b] + i, skipped (zero
    q_rot, no write) where pos0[b] < 0 or i >= q_lens[b]."""
    B, Tq = q.shape[:2]
    q_rot = torch.zeros(q.shape, dtype=q.dtype, device=q.device)
    live = pos0 >= 0
    for i in range(Tq):
        pos = torch.where(live & (q_lens > i), pos0 + i,
                          torch.full_like(pos0, -1))
        q_rot[:, i] = rope_append_paged_ref(
            q[:, i], k[:, i], v[:, i], cosT, sinT, pos, block_table, k_cache,
            v_cache, k_scale, v_scale)
    return q_rot


def rope_append_paged_multi(q, k, v, cosT, sinT, pos0, q_lens, block_table,
                            k_cache, v_cache, k_scale=1.0, v_scale=1.0):
    """Fused verify-step RoPE + paged KV append (one launch). q
    [B,Tq,Hq,D], k/v [B,Tq,Hkv,D] (fused-QKV slices accepted as they
    are), pos0 [B] int32 position of each sequence's row 0 (-1: inactive),
    q_lens [B] int32 rows to write. Row (b, i) is rotated at pos0[b] + i;
    rotated k and raw v go to the pages for i < q_lens[b]. Updates the
    caches in place, returns rotated q [B,Tq,Hq,D] (zeros for rows that are
    not written)."""
    if not q.is_cuda:
        return rope_append_paged_multi_ref(q, k, v, cosT, sinT, pos0, q_lens,
                                           block_table, k_cache, v_cache,
                                           k_scale, v_scale)
    _require_ext("rope_append_paged_multi")
    return _K.rope_append_paged_multi(q, k, v, cosT, sinT, pos0, q_lens,
                                      block_table, k_cache, v_cache,
                                      float(k_scale), float(v_scale))


# --------------------------------------------------------------------------
# Token sampling: temperature, top-k, top-p, inverse-CDF draw
# --------------------------------------------------------------------------


def _sample_params(B, device, temperature, top_k, top_p, u):
    def row(v, dtype):
        if not torch.is_tensor(v):
            return torch.full((B,), v, dtype=dtype, device=device)
        return v.to(device=device, dtype=dtype).expand(B).contiguous()

    return (row(temperature, torch.float32), row(top_k, torch.int32),
            row(top_p, torch.float32), row(u, torch.float32))


def sample_ref(logits: torch.Tensor, temperature, top_k, top_p, u,
               return_kept: bool = False):
    """fp64 reference of `sample`, on the logits' device. Per row, with x the
    logits [V] (-inf allowed and never chosen):

    1. temperature <= 0: the lowest index of the maximum; n_kept = 1.
    2. 0 < top_k < V: keep x >= the k-th largest value (ties kept).
    3. p_i = exp((x_i - max x) / temperature) on kept tokens, else 0.
    4. top_p < 1: with Z1 the kept mass, keep x >= tau, tau the largest
       value with sum{p_i : x_i >= tau} >= top_p * Z1 (ties kept; the
       maximum always stays).
    5. With Z the kept mass, the token is the smallest kept index i with
       sum{p_j : j <= i} > u * Z, or the last kept index if there is none.

    Returns tokens int64 [B], and n_kept int32 [B] with return_kept."""
    B, V = logits.shape
    temperature, top_k, top_p, u = _sample_params(
        B, logits.device, temperature, top_k, top_p, u)
    tokens = torch.empty(B, dtype=torch.long, device=logits.device)
    n_kept = torch.ones(B, dtype=torch.int32, device=logits.device)
    for r in range(B):
        x = logits[r].double()
        T, k, tp = float(temperature[r]), int(top_k[r]), float(top_p[r])
        if T <= 0:
            tokens[r] = int((x == x.max()).nonzero()[0])
            continue
        keep = torch.ones(V, dtype=torch.bool, device=x.device)
        if 0 < k < V:
            keep = x >= torch.sort(x, descending=True).values[k - 1]
        p = torch.where(keep, torch.exp((x - x.max()) / T), 0.0)
        if tp < 1:
            xs, order = torch.sort(x, descending=True)
            reach = (torch.cumsum(p[order], 0) >= tp * p.sum()).nonzero()
            tau = xs[int(reach[0])] if tp > 0 and reach.numel() else xs[0]
            keep &= x >= tau
            p = torch.where(keep, p, 0.0)
        above = (torch.cumsum(p, 0) > float(u[r]) * p.sum()) & keep
        kept_idx = keep.nonzero()
        tokens[r] = int(above.nonzero()[0]) if above.any() else int(
            kept_idx[-1])
        n_kept[r] = int(keep.sum())
    return (tokens, n_kept) if return_kept else tokens


def sample(logits: torch.Tensor, temperature, top_k, top_p, u,
           return_kept: bool = False):
    """One token per row of logits [B, V] under per-row temperature [B],
    top_k [B], top_p [B] and random number u [B] in [0, 1) (Python scalars
    broadcast); the rules are in sample_ref. The draw is an inverse CDF in
    index order with u an input, so the result is a pure function of the
    arguments. bf16 and fp32 GPU logits whose last dimension is contiguous
    (any row stride) run the one-launch HIP kernel (csrc/hip/sample.hip);
    everything else runs sample_ref. Returns tokens int64 [B], and with
    return_kept also n_kept int32 [B], the tokens that survived the filters."""
    if (logits.is_cuda and logits.dtype in (torch.bfloat16, torch.float32)
            and logits.dim() == 2
            and (logits.shape[1] == 1 or logits.stride(1) == 1)):
        _require_ext("sample")
        tokens, n_kept = _K.sample(logits, *_sample_params(
            logits.shape[0], logits.device, temperature, top_k, top_p, u))
        return (tokens, n_kept) if return_kept else tokens
    return sample_ref(logits, temperature, top_k, top_p, u, return_kept)
