"""Paged KV cache: per-layer page pools, one block table for all layers, and the host-side page allocator.

    cache = PagedKVCache(n_layers, num_pages, nkv, page_size, hd, B, max_pages, dtype=torch.float16, device=dev)
    cache.reserve(slot, n_positions)       # positions < n_positions of `slot` are backed by pages (grows only, idempotent)
    step = DecodeStep(layers, embed, norm, lm_head, cache.kpool, cache.vpool, inv_freq, tok, pos, out_tok, block_table=cache.table)
    cache.release(slot)                    # the slot's pages go back to the free list
    cache.fork(src, dst, n_positions)      # dst shares src's first n_positions (a shared prompt prefix)
    step = DecodeStep(..., block_table=cache.table, shared_prefix=cache.prefix)   # the shared pages are read once per group
    cache.trim(slot, window_floor(pos, W)) # sliding window: pages wholly below the floor go back to the pool

A pool is ``[num_pages, nkv, page_size, hd]`` (k and v of every layer have one each); entry j of the table's row b is the page that
holds positions ``j * page_size .. (j + 1) * page_size - 1`` of slot b in EVERY layer's pools, -1 where nothing is reserved (the
kernels' guard reads page 0 through such an entry and drops stores through it).  The allocator is plain host code: a free list and
a reference count per page; the only device work is one small copy of a table row per reserve / release / fork (and fork's copy of
a partial page), none of it inside a captured graph.  The caller reserves the positions a call or a run of graph replays will
reach before it starts."""
import torch

from ._native import QpalError
from .attention import MAX_GROUPS, PAGE_SIZES, kv_cache_bytes

# The smallest prefix fork() makes a group of, in positions, and the fewest members a group needs before it is published to the
# device.  DESIGN.md §26.5: the shared launch pair beats the plain paged launch by more than the plain launch's spread at (members,
# length) = (32, 2048), (64, 2048), (32, 4096), (64, 4096) and loses or ties at 8 or 16 members and at 1024 positions; groups the
# measurement does not favour stay with the plain arithmetic (the launch serves an unpublished slot exactly as the plain one does).
MIN_SHARED_LEN = 2048
MIN_SHARED_MEMBERS = 32


class SharedPrefix:
    """What the shared-prefix decode launch reads: row_group int32 [B] (the group of a slot, or -1), grp_slot int32
    [G] (a live member whose table row addresses the group's shared pages), grp_len int32 [G] (the shared positions, a multiple of
    page_size; 0: no such group).  The tensors keep their addresses: a captured step sees every later push()."""

    def __init__(self, row_group, grp_slot, grp_len, flat=None):
        self.row_group, self.grp_slot, self.grp_len = row_group, grp_slot, grp_len
        self._flat = flat  # empty(): the three are views of one vector, so that push() is ONE copy

    @property
    def G(self):
        return self.grp_slot.shape[0]

    @classmethod
    def empty(cls, B, G=MAX_GROUPS, device="cpu"):
        flat = torch.tensor([-1] * (B + G) + [0] * G, dtype=torch.int32).to(device)
        return cls(flat[:B], flat[B:B + G], flat[B + G:], flat)

    def push(self, row_group, grp_slot, grp_len):
        """the three host lists into the device tensors: one small copy"""
        B, G = self.row_group.shape[0], self.G
        new = torch.tensor(list(row_group) + list(grp_slot) + list(grp_len), dtype=torch.int32)
        if self._flat is not None:
            self._flat.copy_(new)
        else:
            for t, part in ((self.row_group, new[:B]), (self.grp_slot, new[B:B + G]), (self.grp_len, new[B + G:])):
                t.copy_(part)


class PagedKVCache:
    def __init__(self, n_layers, num_pages, nkv, page_size, hd, B, max_pages, dtype=torch.float16, device="cpu", groups=MAX_GROUPS,
                 min_len=MIN_SHARED_LEN, min_members=MIN_SHARED_MEMBERS):
        if not 1 <= int(groups) <= MAX_GROUPS:
            raise QpalError(f"PagedKVCache: groups must lie in [1, {MAX_GROUPS}], got {groups}")
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
        self._rows = [[] for _ in range(self.B)]             # the pages of every slot, in position order (-1: trimmed)
        self._trimmed = [0] * self.B                         # positions below this have lost their pages (a multiple of page_size)
        self._shared = [0] * self.B                          # the prefix a forked slot took from its source
        self._refs = [0] * self.num_pages
        self._free = list(range(self.num_pages - 1, -1, -1))  # a stack: pop() hands out page 0 first
        # shared prefixes: the groups fork() publishes for the shared-prefix decode launch
        self.min_len = int(min_len)                          # the smallest prefix worth a group
        self.min_members = max(int(min_members), 2)          # the fewest members of a group the device is told of
        self.prefix = SharedPrefix.empty(self.B, int(groups), device)
        self._group = [-1] * self.B                          # the group of every slot
        self._members = [[] for _ in range(int(groups))]     # the members of every group, in joining order
        self._glen = [0] * int(groups)

    # ------------------------------------------------------------------------------------------------------ figures
    @property
    def max_len(self):
        """the logical length of a slot: what takes max_len's place in every rule of the attention launches"""
        return self.max_pages * self.page_size

    @property
    def pages_free(self):
        return len(self._free)

    def pages_of(self, slot):
        """the pages of `slot` in position order (a copy; -1 where trim() has taken the page)"""
        return list(self._rows[self._slot(slot)])

    def refcount(self, page):
        return self._refs[page]

    def trimmed_upto(self, slot):
        """positions of `slot` below this have no page any more (trim); 0 for a slot that was never trimmed"""
        return self._trimmed[self._slot(slot)]

    def pages_held(self, slot):
        """the pages `slot` holds a reference on: its reserved pages without the trimmed ones"""
        return sum(1 for page in self._rows[self._slot(slot)] if page >= 0)

    def shared_upto(self, slot):
        """the shared positions of a forked slot: its first shared_upto positions are the source's prefix (whole pages shared, the
        partial page copied) and are never written again; 0 for a slot that was not forked"""
        return self._shared[self._slot(slot)]

    def bytes(self):
        """bytes of ONE pool (k or v of one layer): kv_cache_bytes of a contiguous cache that holds as many positions"""
        return kv_cache_bytes(self.num_pages, self.nkv, self.page_size, self.hd, self.dtype)

    def group_of(self, slot):
        """the group whose shared pages `slot` reads once per group in the shared-prefix launch, or -1"""
        return self._group[self._slot(slot)]

    def members_of(self, group):
        """the slots of `group` (a copy; empty: no such group)"""
        return list(self._members[group])

    def published(self, group):
        """whether `prefix` names the group: it has at least min_members members"""
        return len(self._members[group]) >= self.min_members

    def _push_prefix(self):
        pub = [self.published(g) for g in range(len(self._members))]
        self.prefix.push([g if g >= 0 and pub[g] else -1 for g in self._group],
                         [m[0] if ok else -1 for m, ok in zip(self._members, pub)], [n if ok else 0 for n, ok in zip(self._glen, pub)])

    def _join(self, src, dst, n):
        """fork's bookkeeping of groups: dst joins src's group where the fork shares at least that group's length, or the two
        found a group of the whole pages below n; returns whether anything changed"""
        shared = n // self.page_size * self.page_size
        g = self._group[src]
        if g >= 0:
            if shared < self._glen[g]:
                return False  # a shorter fork from a grouped slot: correct, just not deduplicated
        else:
            if shared < max(self.min_len, self.page_size):
                return False
            g = next((i for i, m in enumerate(self._members) if not m), -1)
            if g < 0:
                return False  # every group is taken: the fork stays ungrouped
            self._members[g], self._glen[g], self._group[src] = [src], shared, g
        self._members[g].append(dst)
        self._group[dst] = g
        return True

    def _leave(self, slot):
        """release's: the slot leaves its group; a group of fewer than two members dissolves; returns whether anything changed"""
        g = self._group[slot]
        if g < 0:
            return False
        self._members[g].remove(slot)  # (grp_slot is the first member left: a survivor)
        self._group[slot] = -1
        if len(self._members[g]) < 2:
            for m in self._members[g]:
                self._group[m] = -1
            self._members[g], self._glen[g] = [], 0
        return True

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
            if page < 0:
                continue  # (trimmed: the reference went with trim())
            self._refs[page] -= 1
            if self._refs[page] == 0:
                self._free.append(page)
        had = bool(self._rows[slot])
        self._rows[slot], self._shared[slot], self._trimmed[slot] = [], 0, 0
        if had:
            self._push_row(slot)
        if self._leave(slot):
            self._push_prefix()

    def trim(self, slot, below):
        """`slot` will never again read a position < below (a sliding window has passed them: below = window_floor(pos, W) of the
        LARGEST window of any layer; a model with one unwindowed layer never trims).  Pages that lie wholly below `below` lose this
        slot's reference — a page nobody else holds goes back to the free list — and their table entries become -1, which the
        windowed launches never dereference.  The slot keeps its length: reserve() still counts positions from 0 and never backs
        a trimmed position again.  A trimmed slot leaves its shared-prefix group (the group's launch would read the pages), and
        fork() from it raises.  A call with a smaller `below` than an earlier one does nothing.  Host code and one small copy of
        the table row, as reserve(): between replays of a captured step, never inside one."""
        slot = self._slot(slot)
        rows = self._rows[slot]
        first, n = self._trimmed[slot] // self.page_size, min(max(int(below), 0) // self.page_size, len(rows))
        if n <= first:
            return
        for j in range(first, n):
            page = rows[j]
            self._refs[page] -= 1
            if self._refs[page] == 0:
                self._free.append(page)
            rows[j] = -1
        self._trimmed[slot] = n * self.page_size
        self._push_row(slot)
        if self._leave(slot):
            self._push_prefix()

    def fork(self, src, dst, n_positions):
        """`dst` (released) takes the first n_positions of `src`: references on src's pages that lie wholly below n_positions, and a
        fresh page with a copy of the partial page, if any, in every layer.  Whole shared pages of at least min_len positions make
        the two a group (or dst joins src's group where the fork covers that group's length), which `prefix` names once it has
        min_members members.  No copy-on-write: both slots append at positions >=
        n_positions only (`src` into its own partial page, `dst` into its copy), so a shared page is never written."""
        src, dst = self._slot(src), self._slot(dst)
        if src == dst or self._rows[dst]:
            raise QpalError("PagedKVCache.fork: dst must be another, released slot")
        n = int(n_positions)
        if not 0 <= n <= len(self._rows[src]) * self.page_size:
            raise QpalError(f"PagedKVCache.fork: slot {src} has no {n} reserved positions")
        if n > 0 and self._trimmed[src] > 0:
            raise QpalError(f"PagedKVCache.fork: slot {src} has been trimmed below position {self._trimmed[src]}: its prefix is gone")
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
        if self._join(src, dst, n):
            self._push_prefix()
