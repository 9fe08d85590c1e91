"""Bin packing of tiles into batches (reference ``data/partition/sampler.py``)."""
from __future__ import annotations

import math
import random
from typing import Dict, Iterator, List, Optional, Sequence

from .partition import TilePartition


def _indexed(items: Sequence[float], cap: float, skip_too_big: bool):
    if skip_too_big:
        return [(v, i) for i, v in enumerate(items) if 0 < v <= cap]
    if not all(0 < v <= cap for v in items):
        raise ValueError("All items must be > 0 and <= bin_capacity.")
    return [(v, i) for i, v in enumerate(items)]


def best_fit_decreasing(items: Sequence[float], bin_capacity: float, skip_too_big: bool = False) -> List[List[int]]:
    """Largest first; each item into the open bin it fills most tightly (sampler.py:11-84)."""
    todo = sorted(_indexed(items, bin_capacity, skip_too_big), key=lambda x: x[0], reverse=True)
    bins: List[List[int]] = []
    room: List[float] = []
    for v, i in todo:
        best, slack = -1, float("inf")
        for b, r in enumerate(room):
            if r >= v and r - v < slack:
                best, slack = b, r - v
        if best < 0:
            bins.append([i]); room.append(bin_capacity - v)
        else:
            bins[best].append(i); room[best] -= v
    return bins


def harmonic_k(items: Sequence[float], bin_capacity: float, k: int = 6, skip_too_big: bool = False) -> List[List[int]]:
    """Online Harmonic-k: an item of scaled size in (1/(j+1), 1/j] shares a bin with j-1 peers of its
    class; items <= 1/k are packed first-fit (sampler.py:87-178)."""
    if k < 2:
        raise ValueError("Parameter k must be an integer >= 2.")
    todo = _indexed(items, bin_capacity, skip_too_big)
    done: List[List[int]] = []
    open_class: Dict[int, List[int]] = {}
    small: List[List[int]] = []
    small_room: List[float] = []
    for v, i in todo:
        scaled = v / bin_capacity
        if scaled > 1 / k:
            j = math.floor(1 / scaled)
            open_class.setdefault(j, []).append(i)
            if len(open_class[j]) == j:
                done.append(open_class[j]); open_class[j] = []
        else:
            for b, r in enumerate(small_room):
                if v <= r:
                    small[b].append(i); small_room[b] -= v
                    break
            else:
                small.append([i]); small_room.append(bin_capacity - v)
    done.extend(b for b in open_class.values() if b)
    done.extend(small)
    return done


def first_fit_decreasing_bucketed(items: Sequence[float], bin_capacity: float, skip_too_big: bool = False,
                                  n_buckets: Optional[int] = 1, rng: Optional[random.Random] = None) -> List[List[int]]:
    """First-fit over the descending order (``n_buckets`` None / >= n / >= 2: plain FFD -- see the note on the
    bucket shuffle below; 1: fully random first-fit, what ``PartitionSampler`` uses), sampler.py:186-289."""
    rng = rng or random
    todo = sorted(_indexed(items, bin_capacity, skip_too_big), key=lambda x: x[0], reverse=True)
    n = len(todo)
    if n == 0:
        return []
    if n_buckets is not None and 1 <= n_buckets < n:
        if n_buckets == 1:
            rng.shuffle(todo)
        else:
            gaps = sorted(((todo[i - 1][0] - todo[i][0], i) for i in range(1, n)), reverse=True)
            cuts = sorted({pos for _, pos in gaps[:n_buckets - 1]} | {n})
            start = 0
            for c in cuts:
                # the reference shuffles a temporary slice here (sampler.py:268: ``rng.shuffle(indexed_items[start:i])``):
                # the packing order stays the plain descending one and only the RNG advances.  Reproduced as is, so
                # that the same seed yields the same bins (and the same later draws) as the reference
                rng.shuffle(todo[start:c])
                start = c
    bins: List[List[int]] = []
    room: List[float] = []
    for v, i in todo:
        for b, r in enumerate(room):
            if r >= v:
                bins[b].append(i); room[b] -= v
                break
        else:
            bins.append([i]); room.append(bin_capacity - v)
    return bins


class TileBatchSampler:
    """Batches of tile ids whose summed weight stays within ``max_num`` (PartitionSampler, sampler.py:292-405):
    shuffle -> random order + bucketed first-fit, re-packed every epoch; otherwise best-fit-decreasing once."""

    def __init__(self, partition: TilePartition, max_num: int, mode: str = "edge", shuffle: bool = False,
                 skip_too_big: bool = False, seed: Optional[int] = None):
        if mode not in ("node", "edge"):
            raise ValueError("mode must be 'node' or 'edge'")
        self.weights = partition.weights(mode)
        self.max_num, self.shuffle, self.skip_too_big = max_num, shuffle, skip_too_big
        self._rng = random.Random(seed)
        self._batches: List[List[int]] = []
        self._generate()

    def _generate(self) -> None:
        idx = list(range(len(self.weights)))
        if self.shuffle:
            self._rng.shuffle(idx)
        w = [self.weights[i] for i in idx]
        if self.shuffle:
            bins = first_fit_decreasing_bucketed(w, self.max_num, self.skip_too_big, rng=self._rng)
        else:
            bins = best_fit_decreasing(w, self.max_num, self.skip_too_big)
        self._batches = [[idx[j] for j in b] for b in bins]

    def __iter__(self) -> Iterator[List[int]]:
        yield from self._batches
        if self.shuffle:
            self._generate()

    def __len__(self) -> int:
        return len(self._batches)
