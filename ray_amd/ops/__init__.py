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
