from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from .. import _lib
from ..graph import EdgeCSR


@torch.no_grad()
def dropout_bits(csr: EdgeCSR, heads: int, dropout_p: float, seeds, seed_dev: Optional[Tensor] = None) -> Tensor:
    """uint8 [len(seeds), n_edges]: the attention-dropout keep bits (bit h = head h) of ``len(seeds)`` layers over the
    slots of one CSR view (``segger_dropout_bits``) -- generated once per training step per view, then every forward /
    backward pass of every layer tests a bit instead of hashing per (edge, head)."""
    _lib.require_cuda(csr.col)
    lib = _lib.load()
    seeds = [int(v) & 0xFFFFFFFFFFFFFFFF for v in seeds]
    stride = (csr.n_edges + 15) // 16 * 16                 # planes start 16-byte aligned: four slots are stored as one word
    out = torch.empty((len(seeds), stride), dtype=torch.uint8, device=csr.col.device)
    arr = (C.c_uint64 * len(seeds))(*seeds)
    with _lib.on_device(out.device):
        rc = lib.segger_dropout_bits(csr.eid.data_ptr() if csr.n_edges else None, csr.n_edges, heads, dropout_p, arr,
                                     len(seeds), _lib.ptr(seed_dev), out.data_ptr(), stride, _lib.stream_ptr(out.device))
    _lib.check(rc, "segger_dropout_bits")
    return out[:, :csr.n_edges]


def dropout_bits_many(views, heads: int, dropout_p: float, seed_dev: Optional[Tensor] = None) -> list:
    """:func:`dropout_bits` for up to four ``(csr, seeds)`` views in ONE launch (``segger_dropout_bits_many``)."""
    views = [(c, [int(v) & 0xFFFFFFFFFFFFFFFF for v in sd]) for c, sd in views]
    if not views:
        return []
    if len(views) > 4:
        return dropout_bits_many(views[:4], heads, dropout_p, seed_dev) + dropout_bits_many(views[4:], heads, dropout_p, seed_dev)
    dev = views[0][0].col.device
    _lib.require_cuda(views[0][0].col)
    lib = _lib.load()
    jobs = (_lib.BitsJob * len(views))()
    outs, keep = [], []
    for i, (csr, seeds) in enumerate(views):
        stride = (csr.n_edges + 15) // 16 * 16
        out = torch.empty((len(seeds), stride), dtype=torch.uint8, device=dev)
        arr = (C.c_uint64 * len(seeds))(*seeds)
        keep.append(arr)
        jobs[i].eid = csr.eid.data_ptr() if csr.n_edges else None
        jobs[i].n_edges, jobs[i].n_seeds = csr.n_edges, len(seeds)
        jobs[i].seeds = C.cast(arr, C.c_void_p)
        jobs[i].bits, jobs[i].plane_stride = out.data_ptr(), stride
        outs.append(out[:, :csr.n_edges])
    with _lib.on_device(dev):
        rc = lib.segger_dropout_bits_many(jobs, len(views), heads, dropout_p, _lib.ptr(seed_dev), _lib.stream_ptr(dev))
    _lib.check(rc, "segger_dropout_bits_many")
    return outs


@torch.no_grad()
def step_advance(step: Tensor, inc: int) -> Tensor:
    """``step += inc`` in place and a snapshot of the new value, one launch (``segger_step_advance``); int64[1] on the GPU."""
    _lib.require_cuda(step)
    if step.dtype != torch.int64 or step.numel() != 1:
        raise ValueError("step_advance: int64[1]")
    snap = torch.empty_like(step)
    with _lib.on_device(step.device):
        rc = _lib.load().segger_step_advance(step.data_ptr(), int(inc), snap.data_ptr(), _lib.stream_ptr(step.device))
    _lib.check(rc, "segger_step_advance")
    return snap


@torch.no_grad()
def step_draws(views, heads: int, dropout_p: float, samplers, negatives, seed_dev: Tensor, advance=None):
    """Every random draw of one training step in ONE launch (``segger_step_draws``): ``views`` = up to four ``(csr, seeds)``
    of :func:`dropout_bits_many` (or []), ``samplers`` = up to two ``(index, seed)`` of :func:`triplet_sample`, ``negatives``
    = ``(pos, n_b, n_b_dev, seed)`` of :func:`sample_negatives` or None; all streams read the device word ``seed_dev``;
    ``advance``: up to 64 fp32 device scalars incremented by one on the way (:func:`adam_step_counters`).
    -> (planes, [(pos, neg, d_pos, d_neg), ...], negatives | None): what the separate calls return for the same seeds."""
    if len(views) > 4 or len(samplers) > 2:
        raise ValueError("step_draws: at most four views and two samplers")
    _lib.require_cuda(seed_dev)
    lib = _lib.load()
    dev = seed_dev.device
    a = _lib.StepDrawsArgs()
    keep, planes, draws = [], [], []
    if views:
        jobs = (_lib.BitsJob * len(views))()
        for i, (csr, seeds) in enumerate(views):
            seeds = [int(v) & 0xFFFFFFFFFFFFFFFF for v in seeds]
            stride = (csr.n_edges + 15) // 16 * 16
            out = torch.empty((len(seeds), stride), dtype=torch.uint8, device=dev)
            arr = (C.c_uint64 * len(seeds))(*seeds)
            keep.append(arr)
            jobs[i].eid = csr.eid.data_ptr() if csr.n_edges else None
            jobs[i].n_edges, jobs[i].n_seeds = csr.n_edges, len(seeds)
            jobs[i].seeds = C.cast(arr, C.c_void_p)
            jobs[i].bits, jobs[i].plane_stride = out.data_ptr(), stride
            planes.append(out[:, :csr.n_edges])
        keep.append(jobs)
        a.bits, a.n_bits, a.heads, a.dropout_p = C.cast(jobs, C.c_void_p), len(views), int(heads), float(dropout_p)
    a.n_samplers = len(samplers)
    for i, (index, seed) in enumerate(samplers):
        lab = index["lab"]
        n = int(lab.numel())
        pos = torch.empty(n, dtype=torch.int64, device=dev)
        neg = torch.empty(n, dtype=torch.int64, device=dev)
        dd = torch.empty((2, n), dtype=torch.float32, device=dev)
        j = a.samplers[i]
        j.lab, j.n, j.n_clusters = lab.data_ptr(), n, int(index["n_clusters"])
        j.cdf_pos, j.cdf_neg = index["cdf_pos_t"].data_ptr(), index["cdf_neg_t"].data_ptr()
        j.counts, j.offsets, j.members = index["counts"].data_ptr(), index["offsets"].data_ptr(), index["members"].data_ptr()
        j.seed, j.dists = int(seed) & 0xFFFFFFFFFFFFFFFF, index["dists"].data_ptr()
        j.pos, j.neg, j.d_pos, j.d_neg = pos.data_ptr(), neg.data_ptr(), dd[0].data_ptr(), dd[1].data_ptr()
        draws.append((pos, neg, dd[0], dd[1]))
    out_neg = None
    if negatives is not None:
        npos, n_b, n_b_dev, nseed = negatives
        npos = npos.to(torch.int64).contiguous()
        out_neg = torch.empty_like(npos)
        keep.append(npos)
        a.neg_pos, a.neg_n, a.neg_n_b, a.neg_n_b_dev = npos.data_ptr(), int(npos.numel()), int(n_b), _lib.ptr(n_b_dev)
        a.neg_seed, a.neg_out = int(nseed) & 0xFFFFFFFFFFFFFFFF, out_neg.data_ptr()
    a.seed_dev = seed_dev.data_ptr()
    if advance:
        ptrs = (C.c_void_p * len(advance))(*[t.data_ptr() for t in advance])
        keep.append(ptrs)
        a.advance, a.n_advance = C.cast(ptrs, C.c_void_p), len(advance)
    with _lib.on_device(dev):
        rc = lib.segger_step_draws(C.byref(a), _lib.stream_ptr(dev))
    _lib.check(rc, "segger_step_draws")
    return planes, draws, out_neg


@torch.no_grad()
def triplet_sample(index: dict, uniforms=None, seed_dev: Optional[Tensor] = None, seed: Optional[int] = None):
    """``FastTripletSelector.sample_triplets`` in one launch (``segger_triplet_sample``) from the selector's index
    (``triplet_loss.FastTripletSelector.build_index``).  ``uniforms``: four [n] tensors, or None for the kernel's own
    counter-based U[0,1) stream, seeded from torch's CPU generator (so ``torch.manual_seed`` still fixes a run) or from
    ``seed`` + the device word ``seed_dev`` (read at run time: a captured hipGraph draws afresh on every replay)."""
    lab = index["lab"]
    _lib.require_cuda(lab)
    lib = _lib.load()
    dev = lab.device
    n = int(lab.numel())
    u = None
    if uniforms is not None:
        u = torch.stack([t.to(device=dev, dtype=torch.float32) for t in uniforms]).contiguous()
        seed = 0
    elif seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())          # CPU generator: no kernel, no sync
    pos = torch.empty(n, dtype=torch.int64, device=dev)
    neg = torch.empty(n, dtype=torch.int64, device=dev)
    dd = torch.empty((2, n), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        rc = lib.segger_triplet_sample(lab.data_ptr(), n, int(index["n_clusters"]), index["cdf_pos_t"].data_ptr(),
                                       index["cdf_neg_t"].data_ptr(), index["counts"].data_ptr(),
                                       index["offsets"].data_ptr(), index["members"].data_ptr(), _lib.ptr(u),
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(seed_dev),
                                       index["dists"].data_ptr(), pos.data_ptr(), neg.data_ptr(), dd[0].data_ptr(),
                                       dd[1].data_ptr(), _lib.stream_ptr(dev))
    _lib.check(rc, "segger_triplet_sample")
    return pos, neg, dd[0], dd[1]


@torch.no_grad()
def sample_negatives(pos: Tensor, n_b: int, n_b_dev: Optional[Tensor] = None, seed: Optional[int] = None,
                     seed_dev: Optional[Tensor] = None) -> Tensor:
    """``(pos + randint(1, n_b)) % n_b`` (the segmentation loss's negatives, lightning_model.py:178-180) in one launch
    (``segger_sample_negatives``); entries with ``pos < 0`` stay ``-1``.  The stream is seeded like
    :func:`triplet_sample`; ``n_b_dev`` (int64[1] on the device) overrides ``n_b`` at run time."""
    _lib.require_cuda(pos)
    lib = _lib.load()
    dev = pos.device
    pos = pos.to(torch.int64).contiguous()
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    neg = torch.empty_like(pos)
    with _lib.on_device(dev):
        rc = lib.segger_sample_negatives(pos.data_ptr(), int(pos.numel()), int(n_b), _lib.ptr(n_b_dev),
                                         int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(seed_dev), neg.data_ptr(),
                                         _lib.stream_ptr(dev))
    _lib.check(rc, "segger_sample_negatives")
    return neg
