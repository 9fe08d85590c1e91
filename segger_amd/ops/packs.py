from __future__ import annotations

import torch
from torch import Tensor

from .. import _lib
from .._lib import DTYPE_CODE


def f32_split_planes(w: Tensor, transposed: bool = False) -> Tensor:
    """bf16 [3, M, K]: hi = bf16(w), mid = bf16(w - hi), lo = bf16(w - hi - mid) of an fp32 matrix (the weight operand of
    :func:`linear_f32_split_launch`); ``transposed``: the planes of w^T, [3, K, M].  One launch (``segger_f32_split_planes``)."""
    w = w.detach()
    if not w.is_cuda:                     # (host tensors: plain torch, for tests of the split's algebra)
        w = w.float().t().contiguous() if transposed else w.float()
        hi = w.bfloat16()
        r = w - hi.float()
        mid = r.bfloat16()
        return torch.stack((hi, mid, (r - mid.float()).bfloat16())).contiguous()
    if w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous():
        w = w.float().contiguous()
    m, k = int(w.shape[0]), int(w.shape[1])
    out = torch.empty((3, k, m) if transposed else (3, m, k), dtype=torch.bfloat16, device=w.device)
    with _lib.on_device(w.device):
        rc = _lib.load().segger_f32_split_planes(w.data_ptr(), m, k, int(transposed), out.data_ptr(), _lib.stream_ptr(w.device))
    _lib.check(rc, "segger_f32_split_planes")
    return out


# Parameters change between forwards in ways their version counters do not always show: torch's FUSED optimizers
# update them in place without bumping ``_version`` (measured: fused Adam 0 -> 0, foreach Adam 0 -> 1).  Every
# optimizer step therefore advances a generation counter ON THE PARAMETERS IT STEPPED (torch's optimizer post-step
# hook); anything else that writes parameters behind autograd's back (``p.data`` arithmetic, a hipGraph replay) must
# call :func:`invalidate_weights` on them, or :func:`invalidate_weight_cache` (everything).  The generation is per
# parameter so that one model's optimizer step does not re-key another model's packs: a pending backward of the other
# model must not see "weights changed" (and its packs are not re-copied for nothing).
_GLOBAL_GENERATION = [0]
_GEN_ATTR = "_segger_weight_gen"
_BASE_ATTR = "_segger_weight_base"      # an alias (detached view) of a parameter names it here: it ages with its base


def alias_of(p: Tensor) -> Tensor:
    """A distinct autograd leaf over the storage of parameter ``p`` whose cached copies follow ``p``'s generation."""
    a = p.detach().requires_grad_(p.requires_grad)
    setattr(a, _BASE_ATTR, p)
    return a


def _gen_of(p) -> tuple:
    base = getattr(p, _BASE_ATTR, None)
    return (getattr(p, _GEN_ATTR, 0), 0 if base is None else getattr(base, _GEN_ATTR, 0))


def invalidate_weights(params) -> None:
    """The given parameters were written in place: their cached compute-dtype copies are rebuilt on next use."""
    for p in params:
        if p is not None:
            setattr(p, _GEN_ATTR, getattr(p, _GEN_ATTR, 0) + 1)


def invalidate_weight_cache(*_args, **_kwargs) -> None:
    """Forget every cached compute-dtype copy of the projection weights (they are rebuilt on next use)."""
    _GLOBAL_GENERATION[0] += 1


def _optimizer_stepped(optimizer, *_args, **_kwargs) -> None:
    for group in optimizer.param_groups:
        invalidate_weights(group["params"])


from torch.optim.optimizer import register_optimizer_step_post_hook as _register_step_hook  # noqa: E402

_register_step_hook(_optimizer_stepped)

# While a hipGraph is being captured, a refresh must only touch buffers the captured step owns: a multi-tensor copy
# over every pack of the process would bake pointers to OTHER models' packs (and their source parameters) into the
# graph, and replays would write through them after those models are gone.  ``pack_scope(params)`` names the
# parameters of the step being captured; outside a scope a capturing refresh is limited to the requesting pack.
_PACK_SCOPE: list = []


class pack_scope:
    def __init__(self, params):
        self.ids = frozenset(id(p) for p in params)

    def __enter__(self):
        _PACK_SCOPE.append(self.ids)
        return self

    def __exit__(self, *exc):
        _PACK_SCOPE.pop()
        return False


class _Pack:
    """Compute-dtype copy of one or several row-stacked fp32 master weights (+ the fp32 stacked bias, + the transposed
    copy the data gradient streams), refreshed only when a parameter changed (optimizer step, load_state_dict, .to()):
    the three projections that read x_tx (lin_l / lin_r of tx-neighbors-tx, lin_l of tx-belongs-bd) are ONE GEMM
    without a per-forward cat + cast + transpose (and without autograd's slice-copies on the way back).  The copies
    live in persistent buffers; after an optimizer step ALL stale packs of the process are refreshed by one multi-tensor
    copy (``torch._foreach_copy_`` casts fp32 -> bf16 into row windows of the stacked buffers in a single launch)."""

    def __init__(self, weights, biases):
        import weakref
        self.params = [weakref.ref(p) for p in tuple(weights) + tuple(b for b in biases if b is not None)]
        self.param_ids = frozenset(id(p) for p in tuple(weights) + tuple(b for b in biases if b is not None))
        self.rows = [int(w.shape[0]) for w in weights]
        self.has_bias = [b is not None for b in biases]
        self.k = int(weights[0].shape[1])
        self.dtype = None
        self.w = self.b = self._wt = None
        self._wt_fresh = False
        self.key = None
        self.views: list = []

    def _alloc(self, dtype, device):
        m = sum(self.rows)
        self.w = torch.empty((m, self.k), dtype=dtype, device=device)
        self.b = torch.zeros(m, dtype=torch.float32, device=device) if any(self.has_bias) else None
        self._wt, self._wt_fresh, self.dtype = None, False, dtype
        self.views, r0 = [], 0
        for r in self.rows:
            self.views.append(self.w[r0:r0 + r]); r0 += r
        r0 = 0
        for r, hb in zip(self.rows, self.has_bias):
            if hb:
                self.views.append(self.b[r0:r0 + r])
            r0 += r

    def _current_key(self):
        ps = [r() for r in self.params]
        if any(p is None for p in ps):
            return None, ps
        return (_GLOBAL_GENERATION[0],) + tuple((p.data_ptr(), p._version) + _gen_of(p) for p in ps), ps

    def get(self, dtype, device):
        key, ps = self._current_key()
        if self.w is None or self.dtype != dtype or self.w.device != device:
            self._alloc(dtype, device)
            self.key = None
        if self.key != key:
            if self.key is not None:
                _refresh_stale_packs(self)                   # one launch for every stale pack (of the scope)
            if self.key != key:                              # (first use, or skipped by the scope)
                with torch.no_grad():
                    _copy_groups(self.views, [p.detach() for p in ps])
                self.key, self._wt_fresh = key, False
        return self

    def planes(self, transposed: bool = False) -> Tensor:
        """fp32 packs: the bf16 [3, M, K] split of the stacked weight (or [3, K, M] of its transpose) for the opt-in
        bf16x3 projections (F32_SPLIT), rebuilt when the pack was refreshed."""
        slot = "_planes_t" if transposed else "_planes"
        hit = self.__dict__.get(slot)
        if hit is None or hit[0] != self.key:
            with torch.no_grad():
                hit = (self.key, f32_split_planes(self.w, transposed=transposed))
            self.__dict__[slot] = hit
        return hit[1]

    @property
    def wt(self) -> Tensor:                              # [K, M]: dX = dY @ W
        if self._wt is None:
            self._wt = torch.empty((self.k, sum(self.rows)), dtype=self.dtype, device=self.w.device)
        if not self._wt_fresh:
            self._wt.copy_(self.w.t())
            self._wt_fresh = True
        return self._wt


_PACKS: dict = {}


def _copy_groups(dsts, srcs) -> None:
    """``torch._foreach_copy_`` per destination dtype: one multi-tensor launch casts all fp32 weights into their bf16 /
    f16 row windows, one copies the fp32 biases.  (A single call over destinations of mixed dtypes mis-copied the fp32
    -> fp32 part on torch 2.10 / ROCm: biases came out wrong while the weights were right.)"""
    by_dtype: dict = {}
    for d, s_ in zip(dsts, srcs):
        g = by_dtype.setdefault(d.dtype, ([], []))
        g[0].append(d); g[1].append(s_)
    for d_list, s_list in by_dtype.values():
        torch._foreach_copy_(d_list, s_list)


@torch.no_grad()
def _refresh_stale_packs(requester: "_Pack") -> None:
    """Refresh every pack whose parameters changed since it was filled: ONE launch for all 16-bit packs on the GPU
    (``segger_pack_refresh``: casts into the stacked buffers, their transposed copies, the bias copies); anything else
    by one multi-tensor copy per dtype + one launch for the transposed copies.  During a hipGraph capture only the
    packs of the active :class:`pack_scope` (or, without one, only ``requester``) are touched: see ``_PACK_SCOPE``."""
    scope = _PACK_SCOPE[-1] if _PACK_SCOPE else None
    capturing = requester.w.is_cuda and torch.cuda.is_current_stream_capturing()
    dsts, srcs, live, one_launch = [], [], [], []
    for pk in _PACKS.values():
        if pk.w is None or pk.w.device != requester.w.device:
            continue
        if scope is not None:
            if not pk.param_ids <= scope:
                continue
        elif capturing and pk is not requester:
            continue
        key, ps = pk._current_key()
        if key is None or key == pk.key:
            continue
        fast = (pk.w.is_cuda and pk.w.element_size() == 2
                and all(p.dtype == torch.float32 and p.is_contiguous() and p.device == pk.w.device for p in ps))
        if fast:
            one_launch.append((pk, ps))
        else:
            dsts += pk.views
            srcs += [p.detach() for p in ps]
        live.append((pk, key))
    if dsts:
        _copy_groups(dsts, srcs)
    # fp32 packs that serve the bf16x3 split kernels: the plane sets they already hold (normal and / or transposed) are
    # rebuilt for ALL of them by ONE launch (segger_f32_split_planes_many) into the same buffers -- lazily, one launch per
    # pack and orientation, they were 16-18 launches of 5 us in a captured 1M-edge step at fp32 storage
    jobs = []
    for pk, key in live:
        if pk.w.is_cuda and pk.w.dtype == torch.float32:
            for slot, tr in (("_planes", 0), ("_planes_t", 1)):
                hit = pk.__dict__.get(slot)
                if hit is not None and hit[1].is_cuda and hit[1].device == pk.w.device:
                    jobs.append((pk, slot, tr, key, hit[1]))
    for j0 in range(0, len(jobs), _lib.PLANES_MAX_JOBS):
        chunk = jobs[j0:j0 + _lib.PLANES_MAX_JOBS]
        arr = (_lib.PlanesJob * len(chunk))()
        for a, (pk, slot, tr, key, buf) in zip(arr, chunk):
            a.w, a.rows, a.cols, a.transpose, a.planes = pk.w.data_ptr(), int(pk.w.shape[0]), int(pk.w.shape[1]), tr, buf.data_ptr()
        dev = chunk[0][0].w.device
        with _lib.on_device(dev):
            rc = _lib.load().segger_f32_split_planes_many(arr, len(chunk), _lib.stream_ptr(dev))
        _lib.check(rc, "segger_f32_split_planes_many")
        for pk, slot, tr, key, buf in chunk:
            pk.__dict__[slot] = (key, buf)
    done_t = set()
    for dt in {pk.w.dtype for pk, _ in one_launch}:
        # casts into the stacked buffers, transposed copies and bias copies of every stale pack: ONE launch
        # (segger_pack_refresh) instead of two multi-tensor copies + the transposing launch below
        group = [(pk, ps) for pk, ps in one_launch if pk.w.dtype == dt]
        n_seg = sum(len(pk.views) for pk, _ in group)
        arr = (_lib.PackSeg * n_seg)()
        i = 0
        for pk, ps in group:
            m_total, r0 = sum(pk.rows), 0
            n_w = len(pk.rows)
            for j, r in enumerate(pk.rows):
                g = arr[i]; i += 1
                g.src, g.dst, g.rows, g.cols = ps[j].data_ptr(), pk.views[j].data_ptr(), r, pk.k
                if pk._wt is not None:
                    g.dst_t, g.ld_t = pk._wt.data_ptr() + r0 * pk._wt.element_size(), m_total
                r0 += r
            for j in range(n_w, len(pk.views)):              # biases, in the order of pk.views
                g = arr[i]; i += 1
                g.src, g.dst, g.rows, g.cols, g.dst_f32 = ps[j].data_ptr(), pk.views[j].data_ptr(), int(pk.views[j].numel()), 1, 1
            if pk._wt is not None:
                done_t.add(id(pk))
        dev = group[0][0].w.device
        with _lib.on_device(dev):
            rc = _lib.load().segger_pack_refresh(arr, n_seg, DTYPE_CODE[dt], _lib.stream_ptr(dev))
        _lib.check(rc, "segger_pack_refresh")
    for pk, key in live:
        pk.key, pk._wt_fresh = key, id(pk) in done_t
    # the transposed copies the data gradients stream (every pack that has been through a backward): one launch
    tr = [pk for pk, _ in live if pk._wt is not None and pk.w.element_size() == 2 and pk.w.is_cuda and not pk._wt_fresh]
    if tr:
        arr = (_lib.TransposeSeg * len(tr))()
        for i, pk in enumerate(tr):
            arr[i].dst, arr[i].src = pk._wt.data_ptr(), pk.w.data_ptr()
            arr[i].rows, arr[i].cols = int(pk.w.shape[0]), int(pk.w.shape[1])
        dev = tr[0].w.device
        with _lib.on_device(dev):
            rc = _lib.load().segger_transpose_many(arr, len(tr), _lib.stream_ptr(dev))
        _lib.check(rc, "segger_transpose_many")
        for pk in tr:
            pk._wt_fresh = True


def packs_of(params) -> list:
    """The live packs built over (a subset of) ``params``: a captured step keeps them -- and so their buffers -- alive
    for as long as its graph may replay."""
    ids = frozenset(id(p) for p in params)
    return [pk for pk in _PACKS.values() if pk.param_ids <= ids]


def _pack_for(weights, biases) -> _Pack:
    """The cache entry of a parameter group, keyed by the tensors' identities (dropped when the first one dies)."""
    import weakref
    ids = tuple(id(w) for w in weights) + tuple(id(b) for b in biases)
    pk = _PACKS.get(ids)
    if pk is None:
        pk = _PACKS[ids] = _Pack(weights, biases)
        weakref.finalize(weights[0], _PACKS.pop, ids, None)
    return pk
