"""Paged KV cache for serving: a page pool plus a batched decoder whose
attention is the fused split-KV HIP kernel (csrc/hip/paged_attn.hip).

The contiguous decoders (models/llama.py) reserve batch x max_T rows
per layer and read all of them for every token. Here K/V live in
16-token pages handed out per request, so a sequence costs what it
uses, and the decode kernel reads only the rows below each sequence's
length.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional

import torch

from ray_amd import ops

PAGE_SIZE = ops.PAGE_SIZE


def pages_for(tokens: int, page_size: int = PAGE_SIZE) -> int:
    return -(-max(0, tokens) // page_size)


class PagedKVPool:
    """Per-layer K/V page tensors [num_pages, Hkv, page_size, D], a host
    free list with reference counts, and a prefix index. Page 0 is the
    reserved null page: block tables are zero-filled, so an unused entry
    points at memory that is inside the allocation and never part of any
    sequence. It is never handed out.

    Prefix index: a full prompt page is keyed by (parent, its page_size
    token ids), where parent is the node id of the page before it (0 at
    the root). Node ids are never reused, so an entry whose ancestor was
    evicted can no longer be reached. One page id addresses every
    layer's tensors, so the index is per pool. An indexed page whose
    count drops to 0 keeps its contents and waits in an LRU; alloc takes
    from the free list first and evicts from the LRU only when that is
    empty. While nothing is registered the pool is a plain free list.

    dtype float8_e4m3fn makes an fp8 pool: a page element is one byte
    holding value / scale (ops.quantize_kv_fp8), with one static
    (k_scale, v_scale) pair for the whole pool. Other dtypes store
    values as they are and take no scale."""

    def __init__(self, num_layers: int, num_pages: int, Hkv: int, D: int,
                 device, dtype=torch.bfloat16, page_size: int = PAGE_SIZE,
                 k_scale: float = 1.0, v_scale: float = 1.0):
        if num_pages < 2:
            raise ValueError("PagedKVPool needs at least 2 pages "
                             "(page 0 is reserved)")
        if dtype in (torch.float8_e4m3fnuz, torch.float8_e5m2,
                     torch.float8_e5m2fnuz):
            raise ValueError(f"fp8 KV pages are float8_e4m3fn, not {dtype}")
        self.is_fp8 = dtype == torch.float8_e4m3fn
        self.k_scale = ops._check_kv_scale(k_scale)
        self.v_scale = ops._check_kv_scale(v_scale)
        if not self.is_fp8 and (self.k_scale != 1.0 or self.v_scale != 1.0):
            raise ValueError("KV scales other than 1 need an fp8 pool")
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
        self._ref: Dict[int, int] = {}       # allocated page -> count >= 1
        self._index: Dict[tuple, int] = {}   # (parent node, tokens) -> page
        self._page_key: Dict[int, tuple] = {}  # indexed page -> its key
        self._node: Dict[int, int] = {}      # indexed page -> its node id
        self._next_node = 1
        # indexed pages with count 0, oldest (first to be evicted) first
        self._lru: "OrderedDict[int, None]" = OrderedDict()

    @property
    def kv_bytes(self) -> int:
        """Bytes of K and V pages over all layers."""
        return sum(t.numel() * t.element_size() for t in self.k + self.v)

    @property
    def num_free(self) -> int:
        """Pages alloc can hand out: free ones plus evictable cached
        ones."""
        return len(self._free) + len(self._lru)

    @property
    def num_cached(self) -> int:
        """Pages held in the prefix index, in use or evictable."""
        return len(self._page_key)

    @property
    def num_usable(self) -> int:
        return self.num_pages - 1

    def _drop_index(self, p: int):
        del self._index[self._page_key.pop(p)]
        del self._node[p]

    def alloc(self, n: int) -> Optional[List[int]]:
        """n pages with count 1, or None (and nothing taken) when the
        pool is short."""
        if n < 0:
            raise ValueError("alloc of a negative page count")
        if n > self.num_free:
            return None
        pages = []
        for _ in range(n):
            if self._free:
                p = self._free.pop()
            else:
                p, _ = self._lru.popitem(last=False)
                self._drop_index(p)
            self._ref[p] = 1
            pages.append(p)
        return pages

    def share(self, pages: List[int]):
        """Take one more reference on each allocated page."""
        pages = list(pages)
        for p in pages:
            if p not in self._ref:
                raise ValueError(f"share: page {p} is not allocated")
        for p in pages:
            self._ref[p] += 1

    def free(self, pages: List[int]):
        """Drop one reference per page. A page at count 0 returns to the
        free list, or, if it is indexed, to the back of the LRU: pass a
        sequence's pages deepest-first so chains are evicted from the
        tail."""
        pages = list(pages)
        if len(set(pages)) != len(pages):
            raise ValueError(f"free: page listed twice in {pages}")
        for p in pages:
            if p not in self._ref:
                raise ValueError(f"free: page {p} is not allocated")
        for p in pages:
            self._ref[p] -= 1
            if self._ref[p] == 0:
                del self._ref[p]
                if p in self._page_key:
                    self._lru[p] = None
                else:
                    self._free.append(p)

    def _page_tokens(self, tokens, i: int) -> tuple:
        ps = self.page_size
        return tuple(int(t) for t in tokens[i * ps:(i + 1) * ps])

    def match_prefix(self, tokens, max_pages: int) -> List[int]:
        """Longest run of indexed full pages that spell the start of
        `tokens`, at most max_pages long, with a reference taken on
        each."""
        pages: List[int] = []
        parent = 0
        for i in range(min(max_pages, len(tokens) // self.page_size)):
            p = self._index.get((parent, self._page_tokens(tokens, i)))
            if p is None:
                break
            if p in self._ref:
                self._ref[p] += 1
            else:
                del self._lru[p]
                self._ref[p] = 1
            pages.append(p)
            parent = self._node[p]
        return pages

    def register_prefix(self, tokens, pages: List[int]):
        """Index every full page of the prompt `tokens`, held in
        `pages` (allocated, in order), that is not indexed yet. A key
        that is already present keeps its first page."""
        parent = 0
        for i in range(min(len(pages), len(tokens) // self.page_size)):
            key = (parent, self._page_tokens(tokens, i))
            p = self._index.get(key)
            if p is None:
                p = pages[i]
                if p not in self._ref:
                    raise ValueError(
                        f"register_prefix: page {p} is not allocated")
                if p in self._page_key:
                    # already spells another chain: leave it there
                    return
                self._index[key] = p
                self._page_key[p] = key
                self._node[p] = self._next_node
                self._next_node += 1
            parent = self._node[p]


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
                 num_pages: Optional[int] = None,
                 prefix_caching: bool = False,
                 prefill_chunk: Optional[int] = None,
                 kv_dtype: Optional[torch.dtype] = None,
                 k_scale: float = 1.0, v_scale: float = 1.0):
        if prefill_chunk is not None and prefill_chunk < 1:
            raise ValueError("prefill_chunk must be at least 1")
        self.prefix_caching = prefix_caching
        self.prefill_chunk = prefill_chunk
        self.prefix_hit_tokens = 0        # prompt tokens served from pages
        self.prefill_tokens_computed = 0  # prompt tokens run through the model
        self.m = model
        cfg = model.cfg
        self.B = batch_size
        self.max_T = max_T
        self.device = device
        hd = cfg.hidden_size // cfg.num_heads
        self.max_pages = pages_for(max_T)
        if num_pages is None:
            num_pages = batch_size * self.max_pages + 1
        # kv_dtype None: pages in the model dtype
        self.pool = PagedKVPool(cfg.num_layers, num_pages, cfg.num_kv_heads,
                                hd, device,
                                model.dtype if kv_dtype is None else kv_dtype,
                                k_scale=k_scale, v_scale=v_scale)
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
            # a decrement: shared pages live on under their other
            # owners. With prefix caching the deepest page goes first,
            # so that cached chains are evicted from their tail.
            pages = self._slot_pages[slot]
            self.pool.free(pages[::-1] if self.prefix_caching else pages)
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
        # An fp8 pool always prefills through the pages, so the prompt
        # attends to the quantised rows that decode will read; the path
        # below attends to the raw K/V and would give the first token
        # other keys than every later one.
        if (self.prefix_caching or self.prefill_chunk is not None
                or self.pool.is_fp8):
            return self._prefill_slot_paged(slot, toks,
                                            max(reserve_tokens, n))
        self.prefill_tokens_computed += n
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

    @torch.no_grad()
    def _prefill_slot_paged(self, slot: int, toks: torch.Tensor,
                            reserve_tokens: int):
        """Prefill through the paged prefill kernel: reuse the cached
        pages that spell the start of the prompt, then run the rest in
        chunks that attend to the pages directly.

        Invariant: shared pages are read-only. Only full prompt pages
        are ever shared; chunk writes start at row 16 * (shared pages)
        and decode appends at rows >= n, both past every shared page."""
        n = toks.numel()
        if n < 1:
            raise ValueError("prefill of an empty prompt")
        ps = self.pool.page_size
        self.release_slot(slot)
        need = pages_for(min(reserve_tokens, self.max_T))
        tok_list = toks.tolist()
        shared: List[int] = []
        if self.prefix_caching:
            # at most (n-1)//ps pages: at least one token is computed,
            # so there are last-position logits
            shared = self.pool.match_prefix(tok_list, (n - 1) // ps)
        fresh = self.pool.alloc(need - len(shared))
        if fresh is None:
            self.pool.free(shared[::-1])
            raise RuntimeError(
                f"paged KV pool exhausted: need {need - len(shared)} pages, "
                f"{self.pool.num_free} free")
        pages = shared + fresh
        self._slot_pages[slot] = pages
        row = torch.zeros(self.max_pages, dtype=torch.int32)
        row[: len(pages)] = torch.tensor(pages, dtype=torch.int32)
        self.block_table[slot].copy_(row)

        ctx = len(shared) * ps
        chunk = self.prefill_chunk or (n - ctx)
        logits = None
        for pos0 in range(ctx, n, chunk):
            end = min(pos0 + chunk, n)
            logits = self._prefill_chunk(slot, toks[pos0:end], pos0,
                                         last=end == n)
        self.prefix_hit_tokens += ctx
        self.prefill_tokens_computed += n - ctx
        if self.prefix_caching:
            self.pool.register_prefix(tok_list, pages[: n // ps])
        self.set_slot_len(slot, n)
        return logits

    def _prefill_chunk(self, slot: int, toks: torch.Tensor, pos0: int,
                       last: bool = True):
        """Run prompt tokens pos0 .. pos0+T-1 of one slot: per layer,
        append their rotated K and raw V to the slot's pages, then
        attend to the pages (append-then-attend, as the decode step).
        Returns last-position logits [V] when `last`, else None."""
        m = self.m
        T = toks.numel()
        ps = self.pool.page_size
        dev = self.device
        x = m.embed(toks.view(1, T))
        cos, sin = m.cosT[pos0 : pos0 + T], m.sinT[pos0 : pos0 + T]
        pool = self.pool
        if not pool.is_fp8:
            t = torch.arange(pos0, pos0 + T, device=dev)
            pg = self.block_table[slot, t // ps].long()
            sl = t % ps
        bt = self.block_table[slot : slot + 1]
        ctx_lens = torch.tensor([pos0], dtype=torch.int32, device=dev)
        q_lens = torch.tensor([T], dtype=torch.int32, device=dev)
        for li, layer in enumerate(m.layers):
            at = layer.attn
            q, k, v = at.qkv(layer.attn_norm(x))
            q = ops.rope(q, cos, sin)
            k = ops.rope(k, cos, sin)
            kp, vp = self.pool.k[li], self.pool.v[li]
            # [1,T,Hkv,D] -> rows pos0.. of the slot's pages. fp8 pages
            # are written by the append op, so prefill and decode
            # quantise in one place and shared prefix pages hold the
            # bytes any request would have produced.
            if pool.is_fp8:
                ops.kv_append_paged(k[0], v[0], pos0, bt[0], kp, vp,
                                    pool.k_scale, pool.v_scale)
            else:
                kp[pg, :, sl] = k[0].to(kp.dtype)
                vp[pg, :, sl] = v[0].to(vp.dtype)
            attn = ops.paged_attention_prefill(q.contiguous(), kp, vp, bt,
                                               ctx_lens, q_lens,
                                               pool.k_scale, pool.v_scale)
            x = x + at.o_proj(attn.reshape(1, T, -1))
            x = x + layer.mlp(layer.mlp_norm(x))
        if not last:
            return None
        return m.lm_head(m.final_norm(x[:, -1:]))[0, -1]

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
                                      kp, vp, self.pool.k_scale,
                                      self.pool.v_scale)
            attn = ops.paged_attention_decode(
                q, kp, vp, self.block_table, self.seq_lens,
                num_splits=self.num_splits, workspace=self.workspace,
                k_scale=self.pool.k_scale, v_scale=self.pool.v_scale)
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
