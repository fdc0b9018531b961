"""Row filters of a filtered search (``vqa_index_search_filtered``): one bit per row position of a shard.  A
:class:`RowFilterBatch` gives each query of a batch its own filter (``vqa_index_search_filtered_multi``).

Layout (include/vqa_retrieval.h): ``ceil(n / 32)`` 32-bit words, row position ``p`` allowed iff
``(bits[p >> 5] >> (p & 31)) & 1``; bits at positions >= n are ignored by the library.  A :class:`RowFilter` holds the words
as an int32 tensor (on the shard's device for a search; on the host it is only built, sliced and inspected) together with the
number of allowed rows and of 256-row tiles they touch -- what a filtered search reads is ``tiles x 256 x d x element size``
bytes.  Nothing here needs a GPU; :meth:`DeviceIndex.row_filter` builds one on the device.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import numpy as np
import torch

TILE_ROWS = 256


def mask_to_bits(mask: torch.Tensor) -> torch.Tensor:
    """bool ``[n]`` -> int32 ``[ceil(n / 32)]`` words (bit p & 31 of word p >> 5), on the mask's device."""
    n = int(mask.numel())
    nw = (n + 31) // 32
    m = torch.zeros(nw * 32, dtype=torch.int64, device=mask.device)
    m[:n] = mask.reshape(-1).to(torch.int64)
    w = (m.view(nw, 32) << torch.arange(32, dtype=torch.int64, device=mask.device)).sum(1)
    return torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)


def bits_to_mask(bits: torch.Tensor, n: int) -> torch.Tensor:
    """int32 words -> bool ``[n]`` (the inverse of :func:`mask_to_bits`; bits past n are dropped)."""
    w = bits.to(torch.int64) & 0xFFFFFFFF
    m = (w[:, None] >> torch.arange(32, dtype=torch.int64, device=bits.device)) & 1
    return m.reshape(-1)[:n].to(torch.bool)


def _as_tensor(a, dtype=None) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    return t.to(dtype) if dtype is not None else t


def _device(device) -> torch.device:
    return torch.device("cuda", device) if isinstance(device, int) else torch.device(device)


class RowFilter:
    """The allowed rows of one shard of ``n`` rows.  ``bits``: int32 words (see the module doc); ``allowed``: rows allowed;
    ``tiles``: 256-row tiles holding at least one of them.  Reusable across searches: the words are uploaded once."""

    def __init__(self, bits: torch.Tensor, n: int):
        n = int(n)
        if bits.dtype != torch.int32 or bits.dim() != 1 or int(bits.numel()) != (n + 31) // 32:
            raise ValueError(f"bits must be an int32 [{(n + 31) // 32}] tensor for {n} rows")
        self.bits = bits.contiguous()
        self.n = n
        self.generation = None  # DeviceIndex.row_filter(): the shard's generation it was built at (a later append / remove makes it stale)
        mask = bits_to_mask(self.bits, n)
        self.allowed = int(mask.sum().item())
        pad = torch.zeros((-n) % TILE_ROWS, dtype=torch.bool, device=mask.device)
        self.tiles = int(torch.cat([mask, pad]).view(-1, TILE_ROWS).any(1).sum().item()) if n else 0

    @classmethod
    def from_mask(cls, mask, device=None) -> "RowFilter":
        """bool / uint8 ``[n]`` mask (numpy array or tensor, host or device; nonzero = allowed)."""
        m = _as_tensor(mask)
        if m.dim() != 1:
            raise ValueError("a row mask must be 1-D [n]")
        if m.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"a row mask must be bool or uint8, got {m.dtype}")
        if device is not None:
            m = m.to(_device(device))
        return cls(mask_to_bits(m != 0), int(m.numel()))

    @classmethod
    def from_positions(cls, n: int, positions, device=None) -> "RowFilter":
        """Row positions in ``[0, n)`` (any order, repeats allowed; numpy array, list or tensor, host or device)."""
        p = _as_tensor(positions, torch.int64).reshape(-1)
        if device is not None:
            p = p.to(_device(device))
        if p.numel() and (int(p.min().item()) < 0 or int(p.max().item()) >= n):
            raise ValueError(f"row positions outside [0, {n})")
        m = torch.zeros(int(n), dtype=torch.bool, device=p.device)
        m[p] = True
        return cls(mask_to_bits(m), int(n))

    def mask(self) -> torch.Tensor:
        """bool ``[n]`` on the words' device."""
        return bits_to_mask(self.bits, self.n)

    def slice(self, lo: int, hi: int) -> "RowFilter":
        """The filter of rows ``[lo, hi)`` as a shard of its own (row lo becomes position 0; lo need not be a multiple of 32):
        what one rank of a sharded index searches with."""
        if not 0 <= lo <= hi <= self.n:
            raise ValueError(f"rows [{lo}, {hi}) outside [0, {self.n})")
        return RowFilter(mask_to_bits(self.mask()[lo:hi]), hi - lo)

    def to(self, device) -> "RowFilter":
        dev = _device(device)
        if self.bits.device == dev:
            return self
        out = RowFilter.__new__(RowFilter)
        out.bits, out.n, out.allowed, out.tiles = self.bits.to(dev), self.n, self.allowed, self.tiles
        out.generation = self.generation
        return out

    def __repr__(self) -> str:
        return f"RowFilter(n={self.n}, allowed={self.allowed}, tiles={self.tiles}, device={self.bits.device})"


class RowFilterBatch:
    """One filter per query of a batch of B (``vqa_index_search_filtered_multi``): the distinct filters stacked as int32
    ``bits [F, ceil(n / 32)]`` and ``query_filter`` int32 ``[B]``, the filter of each query (``-1``: all rows).  Built from a
    list of B ``RowFilter | None``; a filter object that appears several times is stored once (by identity).  Reusable across
    searches and graph captures, like a :class:`RowFilter`; ``generation`` is the shard generation every filter was built at."""

    def __init__(self, filters: Sequence[Optional[RowFilter]]):
        filters = list(filters)
        if not filters:
            raise ValueError("a RowFilterBatch needs one entry per query (got none)")
        distinct: List[RowFilter] = []
        index = {}
        assign = []
        for f in filters:
            if f is None:
                assign.append(-1)
                continue
            if not isinstance(f, RowFilter):
                raise ValueError(f"RowFilterBatch entries must be RowFilter or None, got {type(f).__name__}")
            if id(f) not in index:
                index[id(f)] = len(distinct)
                distinct.append(f)
            assign.append(index[id(f)])
        ns = {f.n for f in distinct}
        devs = {f.bits.device for f in distinct}
        gens = {f.generation for f in distinct if f.generation is not None}  # (a filter built from a mask has none)
        if len(ns) > 1 or len(devs) > 1:
            raise ValueError("the filters of a RowFilterBatch must all be of one shard (same n, same device)")
        if len(gens) > 1:
            raise ValueError(f"the filters of a RowFilterBatch were built at different shard generations {sorted(map(str, gens))}")
        self.filters = distinct
        self.n = distinct[0].n if distinct else None  # None: every query searches all rows (fits any shard)
        self.generation = gens.pop() if gens else None
        dev = distinct[0].bits.device if distinct else torch.device("cpu")
        nw = (self.n + 31) // 32 if distinct else 0
        # F >= 1 always (the library requires it): an all -1 batch carries one empty bitmap nobody uses
        self.bits = (torch.stack([f.bits for f in distinct]) if distinct
                     else torch.zeros((1, nw), dtype=torch.int32, device=dev)).contiguous()
        self.query_filter = torch.tensor(assign, dtype=torch.int32).to(dev)
        self.assign = assign

    def __len__(self) -> int:
        return len(self.assign)

    @property
    def F(self) -> int:
        return int(self.bits.shape[0])

    def _with(self, filters: List[RowFilter]) -> "RowFilterBatch":
        return RowFilterBatch([None if a < 0 else filters[a] for a in self.assign])

    def slice(self, lo: int, hi: int) -> "RowFilterBatch":
        """Every filter restricted to rows ``[lo, hi)`` (:meth:`RowFilter.slice`), same query assignment: what one rank of a
        sharded index searches with."""
        out = self._with([f.slice(lo, hi) for f in self.filters])
        if not self.filters:
            out.n = None
        for f in out.filters:
            f.generation = self.generation
        out.generation = self.generation
        return out

    def to(self, device) -> "RowFilterBatch":
        out = self._with([f.to(device) for f in self.filters])
        if not self.filters:
            out.query_filter = out.query_filter.to(_device(device))
            out.bits = out.bits.to(_device(device))
        return out

    def __repr__(self) -> str:
        return f"RowFilterBatch(B={len(self)}, F={len(self.filters)}, n={self.n}, device={self.bits.device})"
