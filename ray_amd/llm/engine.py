"""LLM engine: prefill + hipGraph decode over the ray_amd Llama.

There is no network/checkpoint access in this environment, so models
are random-init of the named architecture (same as bench.py); the
serving data path (prefill, KV cache, graph-captured decode loop,
sampling) is the real one.
"""
from __future__ import annotations

import random
import time
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import torch

from ray_amd import ops
from ray_amd.models.llama import (
    CONFIGS,
    BatchedDecoder,
    GraphedDecoder,
    KVCache,
    LlamaModel,
    add_lora_slots,
    quantize_experts_mxfp4,
    quantize_linears_fp8,
    quantize_linears_mxfp4,
)


@dataclass
class LLMConfig:
    # A key of models.llama.CONFIGS. "mixtral-8x7b" and "moe-tiny" are
    # mixture-of-experts models: ContinuousBatchingEngine with
    # kv_cache="paged" only, expert weights in bf16 or, with
    # weight_dtype="mxfp4", in MXFP4 (ops.moe_ffn).
    model_id: str = "llama-tiny"
    max_seq_len: int = 512
    max_batch_size: int = 1
    dtype: str = "bfloat16"
    use_hip_graph: bool = True
    temperature: float = 0.0
    # ContinuousBatchingEngine only: "contiguous" (BatchedDecoder) or
    # "paged" (PagedDecoder over a page pool). kv_num_pages counts the
    # reserved null page; default fits max_batch_size x max_seq_len.
    kv_cache: str = "contiguous"
    kv_num_pages: Optional[int] = None
    # Paged cache only. enable_prefix_caching: prompts that start with
    # the same full 16-token pages share those pages and skip their
    # prefill. prefill_chunk_tokens: run a prompt through the model at
    # most that many tokens at a time.
    enable_prefix_caching: bool = False
    prefill_chunk_tokens: Optional[int] = None
    # Paged cache only. kv_cache_dtype: "auto" (the model dtype), "bf16"
    # or "fp8" ("fp8_e4m3" is the same): fp8 pages hold one byte per
    # element, K / kv_k_scale and V / kv_v_scale as OCP e4m3fn, so the
    # same kv_num_pages take half the memory.
    kv_cache_dtype: str = "auto"
    kv_k_scale: float = 1.0
    kv_v_scale: float = 1.0
    # ContinuousBatchingEngine with kv_cache="paged" only. weight_dtype:
    # "auto" or "bf16" (the model dtype) or "fp8" ("fp8_e4m3" is the same):
    # every projection and lm_head hold one byte per weight plus an fp32
    # scale per output channel (ops.LinearW8), and decode reads them with
    # the fp8 skinny-GEMM kernel. "mxfp4": they hold OCP MXFP4 instead, two
    # e2m1 elements per byte and one e8m0 scale byte per 32 of them, 17/32
    # byte per weight (ops.LinearW4), read by the W4A16 skinny-GEMM kernel.
    # Activations stay in the model dtype. On a model with experts "mxfp4"
    # also stores the expert weights as MXFP4 (the routed W4A16 expert
    # kernels; the routers stay in the model dtype); "fp8" with such a model
    # is not built and raises ValueError.
    weight_dtype: str = "auto"
    # ContinuousBatchingEngine with kv_cache="paged" only. max_loras > 0
    # gives every decoder-layer projection that many LoRA adapter slots of
    # rank max_lora_rank (rounded up to 16, 32 or 64; adapters of smaller
    # rank are stored zero-padded). add_lora(name, tensors) fills a slot,
    # submit(..., lora=name) runs a request with it, and requests with
    # different adapters, or none, decode in the same batch: the adapters'
    # part is two HIP kernels per projection that read each row's slot from
    # device memory (ops.lora_add), over bf16, fp8 or MXFP4 base weights.
    max_loras: int = 0
    max_lora_rank: int = 16
    # Sampling defaults of a request (each can be given per request).
    # top_k: keep the k largest logits, ties at the k-th kept (0: off).
    # top_p: then keep the smallest set of largest logits whose mass reaches
    # top_p (1: off). seed: the request draws from its own
    # random.Random(seed), so its tokens do not depend on what else is in
    # the batch (None: the engine's generator). A request that sets none of
    # the three samples as before (argmax or torch.multinomial); the others
    # go through ops.sample, whose rules are in ops.sample_ref.
    top_k: int = 0
    top_p: float = 1.0
    seed: Optional[int] = None
    # ContinuousBatchingEngine only: sample the whole batch with one
    # ops.sample call per step. The step then makes one host-to-device copy
    # (the parameters of all slots, from one pinned tensor) and one
    # device-to-host copy (the tokens) instead of one synchronisation and
    # two scalar writes per slot.
    device_sampling: bool = False
    # ContinuousBatchingEngine with kv_cache="paged" only, and not together
    # with device_sampling. num_speculative_tokens = K > 0: a step runs
    # each greedy request's last token plus up to K draft tokens through the
    # model at once (PagedDecoder.verify) and keeps the drafts the model
    # agrees with, so its tokens are those of K = 0 in fewer steps.
    # (K + 1) * (num_heads // num_kv_heads) must be <= ops.VERIFY_MAX_ROWS.
    # speculative_proposer(tokens so far, k) returns up to k draft tokens;
    # None is prompt lookup: what followed the most recent earlier occurrence
    # of the last n tokens, n from speculative_ngram down to 1. Requests
    # that sample (temperature > 0, top-k, top-p or a seed) are not
    # speculated: they take one token per step, drawn exactly as with K = 0.
    num_speculative_tokens: int = 0
    speculative_ngram: int = 3
    speculative_proposer: Optional[Callable[[List[int], int],
                                            List[int]]] = None

    def __post_init__(self):
        _check_sampling(self.top_k, self.top_p)
        if (int(self.num_speculative_tokens) != self.num_speculative_tokens
                or self.num_speculative_tokens < 0):
            raise ValueError("num_speculative_tokens must be an integer "
                             f">= 0, got {self.num_speculative_tokens!r}")
        if self.speculative_ngram < 1:
            raise ValueError("speculative_ngram must be at least 1")


def _check_sampling(top_k, top_p):
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"top_k must be an integer >= 0, got {top_k!r}")
    if not 0.0 <= top_p <= 1.0:
        raise ValueError(f"top_p must be in [0, 1], got {top_p!r}")


_U_MAX = 1.0 - 2.0 ** -24  # the largest fp32 below 1


class _Sampling:
    """What the engines share: per-request sampling parameters and the
    per-row path through ops.sample."""

    def _init_sampling(self):
        self._rng = random.Random()

    def _request_sampling(self, temperature, top_k, top_p, seed) -> dict:
        c = self.config
        top_k = c.top_k if top_k is None else top_k
        top_p = c.top_p if top_p is None else top_p
        seed = c.seed if seed is None else seed
        _check_sampling(top_k, top_p)
        rng = None if seed is None else random.Random(seed)
        return {
            "temperature": float(c.temperature if temperature is None
                                 else temperature),
            "top_k": int(top_k), "top_p": float(top_p), "rng": rng,
            # False: the argmax / torch.multinomial path of _sample
            "filtered": top_k > 0 or top_p < 1.0 or rng is not None,
        }

    def _next_u(self, req: dict) -> float:
        return min((req["rng"] or self._rng).random(), _U_MAX)

    def _sample_request(self, logits: torch.Tensor, req: dict) -> int:
        """One token for one request from its logits row [V]."""
        if not req["filtered"]:
            return self._sample(logits, req["temperature"])
        tok = ops.sample(logits.view(1, -1), req["temperature"],
                         req["top_k"], req["top_p"], self._next_u(req))
        return int(tok.item())


# LLMConfig.kv_cache_dtype -> page dtype (None: the model dtype)
_KV_CACHE_DTYPES = {
    "auto": None,
    "bf16": torch.bfloat16,
    "fp8": torch.float8_e4m3fn,
    "fp8_e4m3": torch.float8_e4m3fn,
}

_WEIGHT_DTYPES = ("auto", "bf16", "fp8", "fp8_e4m3", "mxfp4")


def _lora_rank(config: LLMConfig) -> int:
    """0 without adapter slots, else max_lora_rank rounded up to a rank
    the kernels have."""
    if config.max_loras < 0 or config.max_loras > 64:
        raise ValueError("max_loras must be 0..64")
    if config.max_loras == 0:
        return 0
    for r in ops.LORA_RANKS:
        if 1 <= config.max_lora_rank <= r:
            return r
    raise ValueError(f"max_lora_rank must be 1..{ops.LORA_RANKS[-1]}, got "
                     f"{config.max_lora_rank!r}")


def ngram_propose(tokens: List[int], k: int, ngram: int = 3) -> List[int]:
    """Prompt-lookup drafts: for n from `ngram` down to 1, find the most
    recent earlier occurrence of the last n tokens and return the up to k
    tokens that followed it; [] when no n matches."""
    L = len(tokens)
    for n in range(min(ngram, L - 1), 0, -1):
        tail = tokens[L - n:]
        for start in range(L - n - 1, -1, -1):
            if tokens[start:start + n] == tail:
                return tokens[start + n:start + n + k]
    return []


def _quantized_weights(config: LLMConfig):
    """None for model-dtype weights, else "fp8" or "mxfp4"."""
    if config.weight_dtype not in _WEIGHT_DTYPES:
        raise ValueError(
            f"weight_dtype must be one of {sorted(_WEIGHT_DTYPES)}, got "
            f"{config.weight_dtype!r}")
    if config.weight_dtype.startswith("fp8"):
        return "fp8"
    return "mxfp4" if config.weight_dtype == "mxfp4" else None


class LLMEngine(_Sampling):
    def __init__(self, config: LLMConfig):
        self.config = config
        self._init_sampling()
        wq = _quantized_weights(config)
        if wq:
            raise ValueError(f"weight_dtype='{wq}' needs "
                             "ContinuousBatchingEngine with kv_cache='paged'")
        if _lora_rank(config):
            raise ValueError("max_loras needs ContinuousBatchingEngine "
                             "with kv_cache='paged'")
        if config.num_speculative_tokens:
            raise ValueError("num_speculative_tokens needs "
                             "ContinuousBatchingEngine with kv_cache='paged'")
        cfg = CONFIGS[config.model_id]
        if cfg.num_experts:
            raise ValueError("a model with experts needs "
                             "ContinuousBatchingEngine with kv_cache='paged'")
        self.model_cfg = cfg
        self.device = (
            torch.device("cuda", 0)
            if torch.cuda.is_available()
            else torch.device("cpu")
        )
        dtype = (
            torch.bfloat16 if self.device.type == "cuda" else torch.float32
        )
        torch.manual_seed(0)
        self.model = LlamaModel(cfg, dtype=dtype).to(self.device).eval()
        self.model.cosT = self.model.cosT.to(self.device)
        self.model.sinT = self.model.sinT.to(self.device)
        self.max_T = min(config.max_seq_len, cfg.max_seq_len)
        self.decoder: Optional[GraphedDecoder] = None
        if self.device.type == "cuda" and config.use_hip_graph:
            self.decoder = GraphedDecoder(self.model, 1, self.max_T, self.device)
            self.decoder.capture()
        self.stats = {"requests": 0, "tokens_generated": 0, "decode_s": 0.0}

    def _sample(self, logits: torch.Tensor, temperature: float) -> int:
        if temperature <= 0:
            return int(logits.argmax(-1).item())
        probs = torch.softmax(logits.float() / temperature, dim=-1)
        return int(torch.multinomial(probs, 1).item())

    @torch.no_grad()
    def generate(self, prompt_ids: List[int], max_new_tokens: int = 32,
                 temperature: Optional[float] = None,
                 top_k: Optional[int] = None, top_p: Optional[float] = None,
                 seed: Optional[int] = None) -> dict:
        req = self._request_sampling(temperature, top_k, top_p, seed)
        cfg = self.model_cfg
        prompt_ids = [t % cfg.vocab_size for t in prompt_ids][: self.max_T - max_new_tokens - 1]
        toks = torch.tensor([prompt_ids], device=self.device)
        t0 = time.perf_counter()
        if self.decoder is not None:
            # prefill into the decoder's caches token-position-wise via
            # eager path, then graph decode
            caches = [
                _ViewCache(self.decoder.cache_k[i], self.decoder.cache_v[i])
                for i in range(cfg.num_layers)
            ]
            logits = self.model(toks, kv_caches=caches, pos0=0)[:, -1]
        else:
            caches = [
                KVCache(1, self.max_T, cfg.num_kv_heads,
                        cfg.hidden_size // cfg.num_heads, self.device,
                        self.model.dtype)
                for _ in range(cfg.num_layers)
            ]
            logits = self.model(toks, kv_caches=caches, pos0=0)[:, -1]
        prefill_s = time.perf_counter() - t0
        out = []
        pos = len(prompt_ids)
        t0 = time.perf_counter()
        for _ in range(max_new_tokens):
            nxt = self._sample_request(logits[0], req)
            out.append(nxt)
            if pos >= self.max_T - 1:
                break
            tok = torch.tensor([nxt], device=self.device)
            if self.decoder is not None:
                logits = self.decoder.decode(tok, pos)
            else:
                logits = self.model(
                    tok.view(1, 1), kv_caches=caches, pos0=pos
                )[:, -1]
            pos += 1
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        decode_s = time.perf_counter() - t0
        self.stats["requests"] += 1
        self.stats["tokens_generated"] += len(out)
        self.stats["decode_s"] += decode_s
        return {
            "token_ids": out,
            "prefill_s": prefill_s,
            "decode_s": decode_s,
            "decode_tok_s": len(out) / decode_s if decode_s > 0 else 0.0,
        }


class _ViewCache:
    """Adapter: lets the eager prefill path fill the GraphedDecoder's
    static cache buffers."""

    def __init__(self, k_buf, v_buf):
        self.k_buf = k_buf
        self.v_buf = v_buf
        self.len = 0

    def update(self, k, v, pos0):
        T = k.size(2)
        self.k_buf[:, :, pos0 : pos0 + T] = k.to(self.k_buf.dtype)
        self.v_buf[:, :, pos0 : pos0 + T] = v.to(self.v_buf.dtype)
        self.len = pos0 + T
        return self.k_buf[:, :, : self.len], self.v_buf[:, :, : self.len]


class ContinuousBatchingEngine(_Sampling):
    """Continuous batching (the vLLM-style loop the reference's serve
    LLM rides on): up to max_batch_size sequences decode together in a
    shared batched KV cache; finished sequences retire and queued
    requests are admitted mid-flight, so decode throughput does not
    drain between requests."""

    def __init__(self, config: LLMConfig):
        self.config = config
        self._init_sampling()
        cfg = CONFIGS[config.model_id]
        self.model_cfg = cfg
        self.device = (
            torch.device("cuda", 0)
            if torch.cuda.is_available()
            else torch.device("cpu")
        )
        dtype = (
            torch.bfloat16 if self.device.type == "cuda" else torch.float32
        )
        torch.manual_seed(0)
        self.model = LlamaModel(cfg, dtype=dtype).to(self.device).eval()
        self.model.cosT = self.model.cosT.to(self.device)
        self.model.sinT = self.model.sinT.to(self.device)
        self.max_T = min(config.max_seq_len, cfg.max_seq_len)
        self.B = max(1, config.max_batch_size)
        if config.kv_cache not in ("contiguous", "paged"):
            raise ValueError(
                f"kv_cache must be 'contiguous' or 'paged', got "
                f"{config.kv_cache!r}")
        self._paged = config.kv_cache == "paged"
        if not self._paged and (config.enable_prefix_caching
                                or config.prefill_chunk_tokens is not None):
            raise ValueError(
                "enable_prefix_caching and prefill_chunk_tokens need "
                "kv_cache='paged'")
        if config.kv_cache_dtype not in _KV_CACHE_DTYPES:
            raise ValueError(
                f"kv_cache_dtype must be one of {sorted(_KV_CACHE_DTYPES)}, "
                f"got {config.kv_cache_dtype!r}")
        kv_dtype = _KV_CACHE_DTYPES[config.kv_cache_dtype]
        if kv_dtype == torch.float8_e4m3fn and not self._paged:
            raise ValueError("kv_cache_dtype='fp8' needs kv_cache='paged'")
        wq = _quantized_weights(config)
        if cfg.num_experts and not self._paged:
            raise ValueError("a model with experts needs kv_cache='paged'")
        if wq:
            if not self._paged:
                raise ValueError(f"weight_dtype='{wq}' needs kv_cache='paged'")
            if cfg.num_experts and wq != "mxfp4":
                raise ValueError(f"weight_dtype='{wq}' together with a model "
                                 "with experts is not built yet")
            if wq == "fp8":
                quantize_linears_fp8(self.model)
            else:
                quantize_linears_mxfp4(self.model)
                quantize_experts_mxfp4(self.model)
        self._lora_rank = _lora_rank(config)
        # name -> {"slot": adapter slot, "root": its prefix-cache root}
        self._loras: dict = {}
        self._lora_roots = 0
        if self._lora_rank:
            if not self._paged:
                raise ValueError("max_loras needs kv_cache='paged'")
            add_lora_slots(self.model, config.max_loras, self._lora_rank)
        self._spec = int(config.num_speculative_tokens)
        if self._spec:
            if not self._paged:
                raise ValueError(
                    "num_speculative_tokens needs kv_cache='paged'")
            if config.device_sampling:
                raise ValueError("num_speculative_tokens together with "
                                 "device_sampling is not built yet")
            self._propose = config.speculative_proposer or (
                lambda toks, k: ngram_propose(toks, k,
                                              config.speculative_ngram))
        if self._paged:
            from ray_amd.llm.paged import PagedDecoder

            self.decoder = PagedDecoder(self.model, self.B, self.max_T,
                                        self.device,
                                        num_pages=config.kv_num_pages,
                                        prefix_caching=(
                                            config.enable_prefix_caching),
                                        prefill_chunk=(
                                            config.prefill_chunk_tokens),
                                        kv_dtype=kv_dtype,
                                        k_scale=config.kv_k_scale,
                                        v_scale=config.kv_v_scale,
                                        spec_tokens=self._spec)
            if config.use_hip_graph and self.device.type == "cuda":
                self.decoder.capture()
        else:
            self.decoder = BatchedDecoder(self.model, self.B, self.max_T,
                                          self.device)
        self._queue: List[dict] = []          # pending requests
        self._slots: List[Optional[dict]] = [None] * self.B
        self._finished: List[dict] = []
        self._next_id = 0
        self._tok = torch.zeros(self.B, dtype=torch.long,
                                device=self.device)
        self._pos = torch.zeros(self.B, dtype=torch.long,
                                device=self.device)
        if config.device_sampling:
            # rows: temperature, top_k, top_p, u, position; the fp32 rows
            # are int32 words viewed as float. One pinned tensor, so a step
            # sends all of it in one copy.
            self._stage = torch.zeros(
                5, self.B, dtype=torch.int32,
                pin_memory=self.device.type == "cuda")
            self._stage_i = self._stage.numpy()
            self._stage_f = self._stage.view(torch.float32).numpy()
            self._params = torch.zeros(5, self.B, dtype=torch.int32,
                                       device=self.device)
        self.stats = {"requests": 0, "tokens_generated": 0,
                      "decode_steps": 0}
        if self._lora_rank:
            self.stats["loras_loaded"] = 0
        if self._spec:
            self.stats["spec_draft_tokens"] = 0
            self.stats["spec_accepted_tokens"] = 0
        self.stats["weight_bytes"] = sum(
            t.numel() * t.element_size()
            for t in (*self.model.parameters(), *self.model.buffers()))
        self._sync_page_stats()

    def _sync_page_stats(self):
        if self._paged:
            pool = self.decoder.pool
            self.stats["kv_pages_total"] = pool.num_usable
            self.stats["kv_cache_bytes"] = pool.kv_bytes
            self.stats["kv_pages_free"] = pool.num_free
            self.stats["kv_pages_cached"] = pool.num_cached
            self.stats["prefix_hit_tokens"] = self.decoder.prefix_hit_tokens
            self.stats["prefill_tokens_computed"] = (
                self.decoder.prefill_tokens_computed)

    def _reserve_tokens(self, prompt_len: int, max_new_tokens: int) -> int:
        """KV rows a request can ever occupy (prompt + decode budget)."""
        return min(prompt_len + max_new_tokens, self.max_T)

    def _lora_modules(self) -> dict:
        return {name: mod for name, mod in self.model.named_modules()
                if isinstance(mod, ops.LoraLinear)}

    def add_lora(self, name: str, tensors: dict,
                 alpha: Optional[float] = None):
        """Load an adapter into a free slot. `tensors` maps the path of a
        decoder-layer projection ("layers.3.attn.o_proj") to (A [r, K],
        B [N, r]); projections that are not named keep a zero adapter. The
        adapter's part of a projection is scale * (x A^T) B^T with scale =
        alpha / r, or 1 when alpha is None. The slot's buffers are written
        in place, so a captured decode graph stays valid."""
        if not self._lora_rank:
            raise ValueError("add_lora needs LLMConfig.max_loras > 0")
        if name in self._loras:
            raise ValueError(f"adapter {name!r} is already loaded")
        used = {v["slot"] for v in self._loras.values()}
        free = [s for s in range(self.config.max_loras) if s not in used]
        if not free:
            raise ValueError(
                f"all {self.config.max_loras} adapter slots are in use")
        mods = self._lora_modules()
        for path, (A, B) in tensors.items():
            mod = mods.get(path)
            if mod is None:
                raise ValueError(f"{path!r} is not an adapted projection")
            r = A.shape[0] if A.dim() == 2 else -1
            if not 1 <= r <= self._lora_rank:
                raise ValueError(
                    f"{path}: rank {r} is not in 1..{self._lora_rank}")
            if (tuple(A.shape) != (r, mod.in_features)
                    or tuple(B.shape) != (mod.out_features, r)):
                raise ValueError(
                    f"{path}: A must be [r, {mod.in_features}] and B "
                    f"[{mod.out_features}, r], got {tuple(A.shape)} and "
                    f"{tuple(B.shape)}")
        slot = free[0]
        with torch.no_grad():
            for path, mod in mods.items():
                mod.lora_A[slot].zero_()
                mod.lora_B[slot].zero_()
                mod.lora_scale[slot] = 0.0
                if path in tensors:
                    A, B = tensors[path]
                    r = A.shape[0]
                    mod.lora_A[slot, :r].copy_(A)
                    mod.lora_B[slot, :, :r].copy_(B)
                    mod.lora_scale[slot] = (1.0 if alpha is None
                                            else float(alpha) / r)
        # a root of its own per call: neither the base model nor an earlier
        # adapter of the same name can hit this one's cached pages
        self._lora_roots -= 1
        self._loras[name] = {"slot": slot, "root": self._lora_roots}
        self.stats["loras_loaded"] = len(self._loras)

    def remove_lora(self, name: str):
        """Free the adapter's slot; not while a request uses it."""
        if name not in self._loras:
            raise ValueError(f"unknown adapter {name!r}")
        for r in (*self._queue, *self._slots):
            if r is not None and r["lora"] == name:
                raise ValueError(
                    f"adapter {name!r} is used by request {r['id']}")
        del self._loras[name]
        self.stats["loras_loaded"] = len(self._loras)

    def submit(self, prompt_ids: List[int], max_new_tokens: int = 32,
               temperature: Optional[float] = None,
               top_k: Optional[int] = None, top_p: Optional[float] = None,
               seed: Optional[int] = None,
               lora: Optional[str] = None) -> int:
        sampling = self._request_sampling(temperature, top_k, top_p, seed)
        if lora is not None and lora not in self._loras:
            raise ValueError(f"unknown adapter {lora!r}")
        rid = self._next_id
        self._next_id += 1
        cfg = self.model_cfg
        prompt = [t % cfg.vocab_size for t in prompt_ids][
            : self.max_T - max_new_tokens - 1
        ]
        if self._paged:
            from ray_amd.llm.paged import pages_for

            need = pages_for(self._reserve_tokens(len(prompt),
                                                  max_new_tokens))
            if need > self.decoder.pool.num_usable:
                raise ValueError(
                    f"request needs {need} KV pages but the pool holds "
                    f"{self.decoder.pool.num_usable}; raise kv_num_pages")
        self._queue.append({
            "id": rid, "prompt": prompt,
            "max_new_tokens": max_new_tokens, "lora": lora,
            **sampling,
        })
        self.stats["requests"] += 1
        return rid

    def _sample(self, logits: torch.Tensor, temperature: float) -> int:
        if temperature <= 0:
            return int(logits.argmax(-1).item())
        probs = torch.softmax(logits.float() / temperature, dim=-1)
        return int(torch.multinomial(probs, 1).item())

    def _admit(self):
        for slot in range(self.B):
            if self._slots[slot] is not None or not self._queue:
                continue
            if self._paged:
                # admit only when the head request's pages fit; requests
                # behind it may not overtake it
                head = self._queue[0]
                reserve = self._reserve_tokens(len(head["prompt"]),
                                               head["max_new_tokens"])
                if not self.decoder.can_reserve(reserve):
                    break
            req = self._queue.pop(0)
            toks = torch.tensor(req["prompt"], device=self.device)
            with torch.no_grad():
                if self._paged and req["lora"] is not None:
                    ad = self._loras[req["lora"]]
                    logits = self.decoder.prefill_slot(
                        slot, toks, reserve, lora_slot=ad["slot"],
                        prefix_root=ad["root"])
                elif self._paged:
                    logits = self.decoder.prefill_slot(slot, toks, reserve)
                else:
                    logits = self.decoder.prefill_slot(slot, toks)
            if self.config.device_sampling:
                tok = ops.sample(logits.view(1, -1), req["temperature"],
                                 req["top_k"], req["top_p"],
                                 self._next_u(req))
                self._tok[slot : slot + 1].copy_(tok)
                first = int(tok.item())
            else:
                first = self._sample_request(logits, req)
            req.update({
                "out": [first],
                "pos": len(req["prompt"]),  # next decode position
                "slot": slot,
            })
            self._slots[slot] = req
        self._sync_page_stats()

    def _retire(self, slot: int):
        req = self._slots[slot]
        self._slots[slot] = None
        if self._paged:
            self.decoder.release_slot(slot)
            self._sync_page_stats()
        self._finished.append({
            "id": req["id"], "token_ids": req["out"],
        })
        self.stats["tokens_generated"] += len(req["out"])

    @torch.no_grad()
    def step(self) -> List[dict]:
        """Admit + one batched decode iteration; returns newly finished
        requests."""
        self._admit()
        # retire sequences that are already complete post-prefill
        for slot in range(self.B):
            r = self._slots[slot]
            if r is not None and (
                len(r["out"]) >= r["max_new_tokens"]
                or r["pos"] >= self.max_T - 1
            ):
                self._retire(slot)
        self._admit()
        active = [s for s in range(self.B) if self._slots[s] is not None]
        if not active:
            out, self._finished = self._finished, []
            return out
        if self._spec:
            self._spec_step(active)
            self.stats["decode_steps"] += 1
            out, self._finished = self._finished, []
            return out
        if self.config.device_sampling:
            sampled = self._decode_and_sample(active)
        else:
            for s in active:
                r = self._slots[s]
                self._tok[s] = r["out"][-1]
                self._pos[s] = r["pos"]
                self.decoder.set_slot_len(s, r["pos"] + 1)  # attend new tok
            logits = self.decoder.decode(self._tok, self._pos)
        for s in active:
            r = self._slots[s]
            if self.config.device_sampling:
                nxt = sampled[s]
            else:
                nxt = self._sample_request(logits[s], r)
            r["out"].append(nxt)
            r["pos"] += 1
            if (len(r["out"]) >= r["max_new_tokens"]
                    or r["pos"] >= self.max_T - 1):
                self._retire(s)
        self.stats["decode_steps"] += 1
        out, self._finished = self._finished, []
        return out

    def _draft(self, r: dict) -> List[int]:
        """Draft tokens for one request this step: none unless it is greedy
        (argmax of the raw logits), and so few that the step neither emits
        more than the request's remaining tokens nor writes a row at or
        past max_T - 1."""
        if r["temperature"] > 0 or r["filtered"]:
            return []
        room = min(self._spec, r["max_new_tokens"] - len(r["out"]) - 1,
                   self.max_T - 2 - r["pos"])
        if room <= 0:
            return []
        draft = []
        for t in list(self._propose(r["prompt"] + r["out"], room))[:room]:
            if not 0 <= int(t) < self.model_cfg.vocab_size:
                break
            draft.append(int(t))
        return draft

    def _spec_step(self, active: List[int]):
        """One verify step: row 0 of a slot is the request's last token, the
        rows after it its drafts. A greedy request keeps the drafts that
        equal the argmax of the row before them and then takes the argmax
        of the first row that disagrees (of the last row when all agree),
        which are the tokens single steps would have produced. The others
        have one row, sampled as in a plain step."""
        T = self._spec + 1
        ps = self.decoder.pool.page_size
        toks = [[0] * T for _ in range(self.B)]
        ctx = [0] * self.B
        q_lens = [0] * self.B
        drafts = {}
        for s in active:
            r = self._slots[s]
            d = drafts[s] = self._draft(r)
            # every row the step writes lies inside the slot's pages
            if r["pos"] + len(d) >= ps * len(self.decoder._slot_pages[s]):
                raise RuntimeError(
                    f"request {r['id']}: rows up to {r['pos'] + len(d)} "
                    f"exceed the slot's reserved pages")
            toks[s][: len(d) + 1] = [r["out"][-1], *d]
            ctx[s] = r["pos"]
            q_lens[s] = len(d) + 1
        logits = self.decoder.verify(
            torch.tensor(toks, device=self.device),
            torch.tensor(ctx, dtype=torch.int32, device=self.device),
            torch.tensor(q_lens, dtype=torch.int32, device=self.device))
        top = logits.argmax(-1).tolist()  # [B][T], the step's one read
        for s in active:
            r = self._slots[s]
            d = drafts[s]
            if r["temperature"] > 0 or r["filtered"]:
                new = [self._sample_request(logits[s, 0], r)]
            else:
                n = 0
                while n < len(d) and d[n] == top[s][n]:
                    n += 1
                new = d[:n] + [top[s][n]]
                self.stats["spec_draft_tokens"] += len(d)
                self.stats["spec_accepted_tokens"] += n
            r["out"].extend(new)
            r["pos"] += len(new)
            self.decoder.set_slot_len(s, r["pos"])
            if (len(r["out"]) >= r["max_new_tokens"]
                    or r["pos"] >= self.max_T - 1):
                self._retire(s)

    def _decode_and_sample(self, active: List[int]) -> List[int]:
        """device_sampling: one decode step and one ops.sample call for the
        whole batch. self._tok already holds every active slot's last token
        on the device (written by the previous call, or by _admit), so the
        host sends only the parameters and reads back only the tokens.
        Inactive slots have temperature 0 and their tokens are ignored."""
        si, sf = self._stage_i, self._stage_f
        sf[0, :] = 0.0
        for s in active:
            r = self._slots[s]
            sf[0, s] = r["temperature"]
            si[1, s] = r["top_k"]
            sf[2, s] = r["top_p"]
            sf[3, s] = self._next_u(r)
            si[4, s] = r["pos"]
            self.decoder.set_slot_len(s, r["pos"] + 1)  # attend new tok
        self._params.copy_(self._stage, non_blocking=True)
        self._pos.copy_(self._params[4])
        logits = self.decoder.decode(self._tok, self._pos)
        pf = self._params.view(torch.float32)
        toks = ops.sample(logits, pf[0], self._params[1], pf[2], pf[3])
        self._tok.copy_(toks)
        return toks.tolist()

    def has_work(self) -> bool:
        return bool(self._queue) or any(
            s is not None for s in self._slots
        )

    def run_until_complete(self) -> dict:
        """Drain everything; returns {request_id: token_ids}."""
        results = {}
        while self.has_work():
            for f in self.step():
                results[f["id"]] = f["token_ids"]
        return results
