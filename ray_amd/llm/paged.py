"""Paged KV cache for serving: a page pool plus a batched decoder whose
attention is the fused split-KV HIP kernel (csrc/hip/paged_attn.hip).

The contiguous decoders (models/llama.py) reserve batch x max_T rows
per layer and read all of them for every token. Here K/V live in
16-token pages handed out per request, so a sequence costs what it
uses, and the decode kernel reads only the rows below each sequence's
length.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from ray_amd import ops

PAGE_SIZE = ops.PAGE_SIZE


def pages_for(tokens: int, page_size: int = PAGE_SIZE) -> int:
    return -(-max(0, tokens) // page_size)


class PagedKVPool:
    """Per-layer K/V page tensors [num_pages, Hkv, page_size, D] and a
    host free list. Page 0 is the reserved null page: block tables are
    zero-filled, so an unused entry points at memory that is inside the
    allocation and never part of any sequence. It is never handed out."""

    def __init__(self, num_layers: int, num_pages: int, Hkv: int, D: int,
                 device, dtype=torch.bfloat16, page_size: int = PAGE_SIZE):
        if num_pages < 2:
            raise ValueError("PagedKVPool needs at least 2 pages "
                             "(page 0 is reserved)")
        self.num_pages = num_pages
        self.page_size = page_size
        self.k = [
            torch.empty(num_pages, Hkv, page_size, D, device=device,
                        dtype=dtype)
            for _ in range(num_layers)
        ]
        self.v = [torch.empty_like(k) for k in self.k]
        # pop() hands out low page numbers first
        self._free: List[int] = list(range(num_pages - 1, 0, -1))
        self._used = set()

    @property
    def num_free(self) -> int:
        return len(self._free)

    @property
    def num_usable(self) -> int:
        return self.num_pages - 1

    def alloc(self, n: int) -> Optional[List[int]]:
        """n pages, or None (and nothing taken) when the pool is short."""
        if n < 0:
            raise ValueError("alloc of a negative page count")
        if n > len(self._free):
            return None
        pages = [self._free.pop() for _ in range(n)]
        self._used.update(pages)
        return pages

    def free(self, pages: List[int]):
        pages = list(pages)
        if len(set(pages)) != len(pages):
            raise ValueError(f"free: page listed twice in {pages}")
        for p in pages:
            if p not in self._used:
                raise ValueError(f"free: page {p} is not allocated")
        for p in pages:
            self._used.remove(p)
            self._free.append(p)


class _PagedSlotCache:
    """KV-cache adapter for prefill into one slot's pages: scatters the
    prompt's K/V into the pages and hands the contiguous K/V back to
    the prefill attention."""

    def __init__(self, k_pages, v_pages, page_ids: torch.Tensor,
                 page_size: int):
        self.k_pages = k_pages
        self.v_pages = v_pages
        self.page_ids = page_ids  # [n_pages] long, on device
        self.page_size = page_size
        self.len = 0

    def update(self, k, v, pos0):
        assert pos0 == 0 and k.size(0) == 1, "paged prefill is whole-prompt"
        T = k.size(2)
        t = torch.arange(T, device=k.device)
        pg = self.page_ids[t // self.page_size]
        sl = t % self.page_size
        # [1,Hkv,T,D] -> [T,Hkv,D]
        self.k_pages[pg, :, sl] = k[0].transpose(0, 1).to(self.k_pages.dtype)
        self.v_pages[pg, :, sl] = v[0].transpose(0, 1).to(self.v_pages.dtype)
        self.len = T
        return k, v


class PagedDecoder:
    """Batched single-token decode over a paged KV cache; same surface
    as BatchedDecoder (prefill_slot / set_slot_len / decode) plus
    release_slot and capture. All per-step state (tokens, positions,
    lengths, block table, split workspace) is in static device buffers
    read by the kernels, so one captured graph replays for any mix of
    sequence lengths."""

    def __init__(self, model, batch_size: int, max_T: int, device,
                 num_pages: Optional[int] = None):
        self.m = model
        cfg = model.cfg
        self.B = batch_size
        self.max_T = max_T
        self.device = device
        hd = cfg.hidden_size // cfg.num_heads
        self.max_pages = pages_for(max_T)
        if num_pages is None:
            num_pages = batch_size * self.max_pages + 1
        self.pool = PagedKVPool(cfg.num_layers, num_pages, cfg.num_kv_heads,
                                hd, device, model.dtype)
        self.block_table = torch.zeros(batch_size, self.max_pages,
                                       dtype=torch.int32, device=device)
        self.seq_lens = torch.zeros(batch_size, dtype=torch.int32,
                                    device=device)
        self.pos = torch.full((batch_size,), -1, dtype=torch.int32,
                              device=device)
        self.in_tok = torch.zeros(batch_size, 1, dtype=torch.long,
                                  device=device)
        self._slot_pages: List[List[int]] = [[] for _ in range(batch_size)]
        # fixed at construction: a captured graph bakes the grid in
        self.num_splits = ops.default_num_splits(
            batch_size, cfg.num_kv_heads, max_T, device)
        self.workspace = None
        if device.type == "cuda" and self.num_splits > 1:
            self.workspace = torch.empty(
                batch_size * cfg.num_heads * self.num_splits * (hd + 2),
                dtype=torch.float32, device=device)
        self.out_logits = None
        self.graph = None

    # ---- slot bookkeeping -------------------------------------------

    def can_reserve(self, tokens: int) -> bool:
        return pages_for(min(tokens, self.max_T)) <= self.pool.num_free

    def release_slot(self, slot: int):
        """Return the slot's pages to the pool; the slot goes inactive."""
        if self._slot_pages[slot]:
            self.pool.free(self._slot_pages[slot])
            self._slot_pages[slot] = []
        self.block_table[slot].zero_()
        self.seq_lens[slot] = 0
        self.pos[slot] = -1

    def set_slot_len(self, slot: int, length: int):
        self.seq_lens[slot] = length

    def reserve_slot(self, slot: int, reserve_tokens: int) -> List[int]:
        """Give the slot fresh pages for `reserve_tokens` rows (capped
        at max_T) and point its block-table row at them. The slot's
        length stays 0 until set_slot_len / prefill_slot."""
        self.release_slot(slot)
        need = pages_for(min(reserve_tokens, self.max_T))
        pages = self.pool.alloc(need)
        if pages is None:
            raise RuntimeError(
                f"paged KV pool exhausted: need {need} pages, "
                f"{self.pool.num_free} free")
        self._slot_pages[slot] = pages
        row = torch.zeros(self.max_pages, dtype=torch.int32)
        row[: len(pages)] = torch.tensor(pages, dtype=torch.int32)
        self.block_table[slot].copy_(row)
        return pages

    def prefill_slot(self, slot: int, toks: torch.Tensor,
                     reserve_tokens: Optional[int] = None):
        """Run the prompt through the model's normal prefill, scattering
        its K/V into freshly allocated pages. Pages for `reserve_tokens`
        (prompt + decode budget; default max_T) are taken up front.
        Returns last-position logits [V]."""
        n = toks.numel()
        if reserve_tokens is None:
            reserve_tokens = self.max_T
        if n > self.max_T:
            raise ValueError(f"prompt of {n} tokens exceeds max_T "
                             f"{self.max_T}")
        pages = self.reserve_slot(slot, max(reserve_tokens, n))
        page_ids = torch.tensor(pages, dtype=torch.long, device=self.device)
        caches = [
            _PagedSlotCache(self.pool.k[li], self.pool.v[li], page_ids,
                            self.pool.page_size)
            for li in range(self.m.cfg.num_layers)
        ]
        logits = self.m(toks.view(1, -1), kv_caches=caches, pos0=0)[0, -1]
        self.set_slot_len(slot, n)
        return logits

    # ---- decode -----------------------------------------------------

    def _step(self):
        m = self.m
        B = self.B
        x = m.embed(self.in_tok)  # [B,1,H]
        lin = ops.linear_sb
        for li, layer in enumerate(m.layers):
            h = layer.attn_norm(x)
            at = layer.attn
            q, k, v = at.qkv(h, lin=lin)  # strided views of the fused row
            kp, vp = self.pool.k[li], self.pool.v[li]
            q = ops.rope_append_paged(q[:, 0], k[:, 0], v[:, 0], m.cosT,
                                      m.sinT, self.pos, self.block_table,
                                      kp, vp)
            attn = ops.paged_attention_decode(
                q, kp, vp, self.block_table, self.seq_lens,
                num_splits=self.num_splits, workspace=self.workspace)
            x = x + lin(attn.reshape(B, 1, -1), at.o_proj.weight)
            hm = layer.mlp_norm(x)
            mp = layer.mlp
            x = x + lin(ops.swiglu(lin(hm, mp.gate_proj.weight),
                                   lin(hm, mp.up_proj.weight)),
                        mp.down_proj.weight)
        x = m.final_norm(x)
        return lin(x, m.lm_head.weight)[:, 0]

    @torch.no_grad()  # grad mode gates the GEMV fast path (linear_sb)
    def capture(self):
        """Record the batched step into a graph the way
        GraphedDecoder.capture does: side-stream warm-up, then a
        single-stream capture."""
        assert self.device.type == "cuda"
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):  # warmup allocations
                self.out_logits = self._step()
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out_logits = self._step()

    @torch.no_grad()
    def decode(self, toks: torch.Tensor, pos: torch.Tensor):
        """toks [B] last tokens, pos [B] their positions; returns logits
        [B, V]. Slots whose length is 0 are inactive: they write no K/V
        and their logits rows are meaningless."""
        self.in_tok.copy_(toks.view(self.B, 1))
        p32 = pos.to(device=self.device, dtype=torch.int32)
        self.pos.copy_(torch.where(self.seq_lens > 0, p32,
                                   torch.full_like(p32, -1)))
        if self.graph is not None:
            self.graph.replay()
            return self.out_logits
        return self._step()
