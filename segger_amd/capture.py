"""What the two captured steps share (``train_step_graph``: one training step per replay; ``inference``: one scored
batch per replay): the geometric ladder of bucket sizes, the test of a batch against a bucket, the policy of a pool of
buckets, the static buffers a capture reads, and the warm-up that precedes it."""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch
from torch import Tensor

from .graph import EdgeCSR


# ------------------------------------------------------------------------------------------------ the ladder
def ladder(n: int, granularity: float, floor: int, extra: int = 0) -> int:
    """``n`` rounded up the ladder ``floor, int(floor * g) + 1, ...`` to a rung strictly above it (a dummy of every kind
    exists), then ``extra`` rungs further."""
    b = floor
    while b <= n:
        b = int(b * granularity) + 1
    for _ in range(extra):
        b = int(b * granularity) + 1
    return b


# ------------------------------------------------------------------------------------------------ batch against bucket
def counts(batch, edges: dict) -> Dict[str, int]:
    """What a bucket's sizes are made from and compared with: node counts, ``num_graphs``, and the edge count of every
    edge type in ``edges`` (size key -> edge type; the training step and the predictor name their edge sizes differently)."""
    c = {"tx": batch["tx"].num_nodes, "bd": batch["bd"].num_nodes, "graphs": int(getattr(batch, "num_graphs", 1))}
    for key, et in edges.items():
        c[key] = int(batch[et].edge_index.shape[1])
    return c


def fits(sizes: Dict[str, int], batch, edges: dict) -> bool:
    """``counts(batch, edges)`` against a bucket's sizes: node counts strictly below their size (a dummy of every kind
    exists), edge and graph counts at most their size.  Read one at a time, most telling first: a pool asks every bucket
    about every batch, and most answers are an early no."""
    if batch["tx"].num_nodes >= sizes["tx"] or batch["bd"].num_nodes >= sizes["bd"]:
        return False
    for key, et in edges.items():
        if int(batch[et].edge_index.shape[1]) > sizes[key]:
            return False
    return int(getattr(batch, "num_graphs", 1)) <= sizes["graphs"]


def waste(sizes: Dict[str, int], batch, edges: dict, e_tt: str) -> float:
    """Padded / real size of the transcript side (what a step costs): the larger of the node ratio and the ratio of the
    transcript-to-transcript edges (size key ``e_tt``)."""
    return max(sizes[e_tt] / max(int(batch[edges[e_tt]].edge_index.shape[1]), 1), sizes["tx"] / max(batch["tx"].num_nodes, 1))


# ------------------------------------------------------------------------------------------------ the pool of buckets
def tightest(buckets: list, batch):
    """The bucket that holds ``batch`` with the least waste, or None."""
    fit = [b for b in buckets if b.fits(batch)]
    return min(fit, key=lambda b: b.waste(batch)) if fit else None


def pick(buckets: list, batch, make_bucket: Callable, granularity: float, max_buckets: int, when_full: str):
    """The tightest bucket ``batch`` fits.  ``make_bucket()`` is appended and returned instead when none fits or the
    tightest would pad the transcript side by more than two granules; with ``max_buckets`` in the pool the tightest fit
    is used whatever it wastes, and a batch no bucket holds raises ``RuntimeError(when_full)``."""
    best = tightest(buckets, batch)
    full = len(buckets) >= max_buckets
    if best is None or (best.waste(batch) > granularity ** 2 and not full):
        if full:
            raise RuntimeError(when_full)
        best = make_bucket()
        buckets.append(best)
    return best


# ------------------------------------------------------------------------------------------------ static buffers
def zeros_on(dev) -> Callable[..., Tensor]:
    return lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)


def static_csr(n_rows: int, n_cols: int, n_edges: int, dev) -> EdgeCSR:
    z = zeros_on(dev)
    return EdgeCSR(z(n_rows + 1, dtype=torch.int64), z(n_edges, dtype=torch.int32), z(n_edges, dtype=torch.int32),
                   n_rows, n_cols)


def node_segments(dst: dict, tx, bd, tx_x_pad: int, bd_x: Optional[Tensor] = None) -> list:
    """``ops.stage`` segments of ``x`` / ``pos`` / ``batch`` of both node types into ``dst[type][attr]``.  Dummies are
    copies of node 0, except a dummy transcript's gene id, which is ``tx_x_pad``; ``bd_x``: the boundary features to
    copy when they are not ``bd["x"]`` itself (a compute-dtype copy)."""
    bd_x = bd["x"] if bd_x is None else bd_x
    T, B = dst["tx"], dst["bd"]
    return [(T["x"], tx["x"], "const", tx_x_pad, 0, 0),
            (T["pos"], tx["pos"], "tile", 2, 0, 0), (T["batch"], tx["batch"], "tile", 1, 0, 0),
            (B["x"], bd_x, "tile", max(int(bd_x[0].numel()), 1), 0, 0),
            (B["pos"], bd["pos"], "tile", 2, 0, 0), (B["batch"], bd["batch"], "tile", 1, 0, 0)]


# ------------------------------------------------------------------------------------------------ warm-up
def on_side_stream(fn: Callable[[], None]) -> None:
    """Run ``fn`` on a fresh stream, ordered behind the current stream's work and ahead of what it is given next: the
    eager run before a capture (lazy inits, allocator, optimizer state) stays off the stream that will be captured."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)


# ------------------------------------------------------------------------------------------------ gradient exchange
class Exchange:
    """How a data-parallel step's gradients are exchanged between its backward and its Adam: not at all, by a callable
    that averages the tensors ``.grad`` points at IN PLACE, or through a ``dp.FlatGradBucket``.  Every ``step`` call
    runs ``zero`` or ``adopt``, then exactly one ``reduce``, on every rank."""

    def __init__(self, sync: Optional[Callable] = None, bucket=None):
        self.sync, self.bucket = sync, bucket
        self.split = sync is not None or bucket is not None

    def pack(self) -> None:
        """(inside the backward's capture) gradients -> the bucket's flat buffer; ``.grad`` = its slices."""
        if self.bucket is not None:
            self.bucket.pack()

    def zero(self, params: list, grads: Optional[list] = None) -> None:
        """This rank has no batch: zeros into the exchange.  ``grads``: the tensors a captured Adam reads (None before
        any capture: fresh ones)."""
        if self.bucket is not None:
            self.bucket.zero()
        elif self.sync is not None:
            if grads is None:
                grads = [torch.zeros_like(p) for p in params]
            else:
                torch._foreach_zero_([g for g in grads if g is not None])
            self.adopt(params, grads)

    def adopt(self, params: list, grads: list) -> None:
        """After the backward graph's replay: ``.grad`` = the tensors it wrote (the bucket's slices / ``grads``)."""
        if self.bucket is not None:
            params, grads = self.bucket.params, self.bucket.views
        for p, g in zip(params, grads):
            p.grad = g

    def reduce(self) -> None:
        if self.bucket is not None:
            self.bucket.all_reduce_mean(packed=True)
        elif self.sync is not None:
            self.sync()       # must average IN PLACE: the captured optimizer reads the tensors .grad points at now


def exchange_of(grad_sync=None, grad_bucket=None) -> Exchange:
    if grad_bucket is None and hasattr(getattr(grad_sync, "__self__", None), "pack"):
        grad_bucket, grad_sync = grad_sync.__self__, None     # bucket.all_reduce_mean given as the callable
    return Exchange(grad_sync, grad_bucket)
