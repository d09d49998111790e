"""Paged KV cache: per-layer page pools, one block table for all layers, and the host-side page allocator.

    cache = PagedKVCache(n_layers, num_pages, nkv, page_size, hd, B, max_pages, dtype=torch.float16, device=dev)
    cache.reserve(slot, n_positions)       # positions < n_positions of `slot` are backed by pages (grows only, idempotent)
    step = DecodeStep(layers, embed, norm, lm_head, cache.kpool, cache.vpool, inv_freq, tok, pos, out_tok, block_table=cache.table)
    cache.release(slot)                    # the slot's pages go back to the free list
    cache.fork(src, dst, n_positions)      # dst shares src's first n_positions (a shared prompt prefix)

A pool is ``[num_pages, nkv, page_size, hd]`` (k and v of every layer have one each); entry j of the table's row b is the page that
holds positions ``j * page_size .. (j + 1) * page_size - 1`` of slot b in EVERY layer's pools, -1 where nothing is reserved (the
kernels' guard reads page 0 through such an entry and drops stores through it).  The allocator is plain host code: a free list and
a reference count per page; the only device work is one small copy of a table row per reserve / release / fork (and fork's copy of
a partial page), none of it inside a captured graph.  The caller reserves the positions a call or a run of graph replays will
reach before it starts."""
import torch

from ._native import QpalError
from .attention import PAGE_SIZES, kv_cache_bytes


class PagedKVCache:
    def __init__(self, n_layers, num_pages, nkv, page_size, hd, B, max_pages, dtype=torch.float16, device="cpu"):
        if page_size not in PAGE_SIZES:
            raise QpalError(f"PagedKVCache: page_size must be one of {PAGE_SIZES}, got {page_size}")
        if min(n_layers, num_pages, nkv, hd, B, max_pages) < 1:
            raise QpalError("PagedKVCache: n_layers, num_pages, nkv, hd, B and max_pages must be at least 1")
        kv_cache_bytes(1, 1, 1, 1, dtype)  # (the dtype check)
        self.n_layers, self.num_pages, self.nkv, self.page_size, self.hd = int(n_layers), int(num_pages), int(nkv), int(page_size), int(hd)
        self.B, self.max_pages, self.dtype = int(B), int(max_pages), dtype
        shape = (self.num_pages, self.nkv, self.page_size, self.hd)
        mk = lambda: [torch.zeros(shape, dtype=torch.uint8 if dtype != torch.float16 else dtype, device=device).view(dtype)  # noqa: E731
                      for _ in range(self.n_layers)]
        self.kpool, self.vpool = mk(), mk()
        self.table = torch.full((self.B, self.max_pages), -1, dtype=torch.int32, device=device)
        self._rows = [[] for _ in range(self.B)]             # the pages of every slot, in position order
        self._shared = [0] * self.B                          # the prefix a forked slot took from its source
        self._refs = [0] * self.num_pages
        self._free = list(range(self.num_pages - 1, -1, -1))  # a stack: pop() hands out page 0 first

    # ------------------------------------------------------------------------------------------------------ figures
    @property
    def max_len(self):
        """the logical length of a slot: what takes max_len's place in every rule of the attention launches"""
        return self.max_pages * self.page_size

    @property
    def pages_free(self):
        return len(self._free)

    def pages_of(self, slot):
        """the pages of `slot` in position order (a copy)"""
        return list(self._rows[self._slot(slot)])

    def refcount(self, page):
        return self._refs[page]

    def shared_upto(self, slot):
        """the shared positions of a forked slot: its first shared_upto positions are the source's prefix (whole pages shared, the
        partial page copied) and are never written again; 0 for a slot that was not forked"""
        return self._shared[self._slot(slot)]

    def bytes(self):
        """bytes of ONE pool (k or v of one layer): kv_cache_bytes of a contiguous cache that holds as many positions"""
        return kv_cache_bytes(self.num_pages, self.nkv, self.page_size, self.hd, self.dtype)

    # ---------------------------------------------------------------------------------------------------- allocator
    def _slot(self, slot):
        if not 0 <= int(slot) < self.B:
            raise QpalError(f"PagedKVCache: slot {slot} outside the table's {self.B} rows")
        return int(slot)

    def _push_row(self, slot):
        row = self._rows[slot] + [-1] * (self.max_pages - len(self._rows[slot]))
        self.table[slot].copy_(torch.tensor(row, dtype=torch.int32))

    def reserve(self, slot, n_positions):
        """backs positions < n_positions of `slot` with pages; a slot only grows, a second call with the same figure does nothing.
        QpalError, with everything as it was, if the pool has too few free pages or n_positions > max_pages * page_size."""
        slot = self._slot(slot)
        if n_positions > self.max_len:
            raise QpalError(f"PagedKVCache.reserve: {n_positions} positions, a slot holds at most {self.max_len}")
        need = (max(int(n_positions), 0) + self.page_size - 1) // self.page_size - len(self._rows[slot])
        if need <= 0:
            return
        if need > len(self._free):
            raise QpalError(f"PagedKVCache.reserve: {need} pages needed, {len(self._free)} free")
        for _ in range(need):
            page = self._free.pop()
            self._refs[page] = 1
            self._rows[slot].append(page)
        self._push_row(slot)

    def release(self, slot):
        """drops the slot's references; a page nobody else holds goes back to the free list; the row goes back to -1"""
        slot = self._slot(slot)
        for page in reversed(self._rows[slot]):
            self._refs[page] -= 1
            if self._refs[page] == 0:
                self._free.append(page)
        had = bool(self._rows[slot])
        self._rows[slot], self._shared[slot] = [], 0
        if had:
            self._push_row(slot)

    def fork(self, src, dst, n_positions):
        """`dst` (released) takes the first n_positions of `src`: references on src's pages that lie wholly below n_positions, and a
        fresh page with a copy of the partial page, if any, in every layer.  No copy-on-write: both slots append at positions >=
        n_positions only (`src` into its own partial page, `dst` into its copy), so a shared page is never written."""
        src, dst = self._slot(src), self._slot(dst)
        if src == dst or self._rows[dst]:
            raise QpalError("PagedKVCache.fork: dst must be another, released slot")
        n = int(n_positions)
        if not 0 <= n <= len(self._rows[src]) * self.page_size:
            raise QpalError(f"PagedKVCache.fork: slot {src} has no {n} reserved positions")
        full, part = divmod(n, self.page_size)
        if part and not self._free:
            raise QpalError("PagedKVCache.fork: no free page for the copy of the partial page")
        pages = self._rows[src][:full]
        for page in pages:
            self._refs[page] += 1
        if part:
            page, old = self._free.pop(), self._rows[src][full]
            self._refs[page] = 1
            for pool in self.kpool + self.vpool:
                pool[page].view(torch.uint8).copy_(pool[old].view(torch.uint8))
            pages = pages + [page]
        self._rows[dst], self._shared[dst] = pages, n
        self._push_row(dst)
