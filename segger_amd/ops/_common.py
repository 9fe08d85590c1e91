from __future__ import annotations

import functools
from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _lib


# --------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------
def _rows(t: Tensor, width: int, name: str) -> Tuple[int, int]:
    """(data_ptr, row stride in elements) of a [n, width] tensor whose last dim is dense."""
    sh = t.shape
    if len(sh) != 2 or sh[1] != width:
        raise ValueError(f"{name}: expected [n, {width}], got {tuple(sh)}")
    st = t.stride()
    if sh[0] > 1:
        if st[1] != 1:
            raise ValueError(f"{name}: last dimension must be contiguous")
        return t.data_ptr(), st[0]
    return t.data_ptr(), max(width, st[0])


def _grad_rows(g: Tensor, dt) -> Tensor:
    """An incoming gradient in the compute dtype with dense rows (what :func:`_rows` takes); the common case costs no torch call."""
    if g.dtype != dt:
        g = g.to(dt)
    if g.dim() != 2 or (g.shape[0] > 1 and g.stride(1) != 1):
        g = g.contiguous()
    return g


def _seq(v) -> tuple:
    """A parameter argument that may be one tensor (or None) or a sequence of them, as a tuple."""
    return tuple(v) if isinstance(v, (list, tuple)) else (v,)


def _tag_prenorm(z: Tensor, y: Tensor, eps: float) -> Tensor:
    """Leaves on ``z = l2_normalize(y, eps)`` what it was normalised from (ops.loss_head may differentiate through y directly)."""
    if torch.is_grad_enabled() and y.requires_grad:
        z._segger_prenorm = (y, float(eps))
    return z


def _prenorm_of(z: Tensor):
    """``(y, eps)`` as :func:`_tag_prenorm` left it on ``z``, or None."""
    return getattr(z, "_segger_prenorm", None)


@functools.lru_cache(maxsize=None)
def _has_specialised(heads: int, channels: int) -> bool:
    return bool(_lib.load().segger_gatv2_has_specialised(heads, channels))


@functools.lru_cache(maxsize=4096)
def _gat_bwd_ws_bytes(n_dst: int, n_src: int, n_edges: int, heads: int, channels: int) -> int:
    """``n_src`` / ``n_edges``: of the by-source view the source pass walks; 0 for the one-pass form."""
    return int(_lib.load().segger_gatv2_bwd_workspace_bytes_two_pass(n_dst, n_src, n_edges, heads, channels))


@functools.lru_cache(maxsize=4096)
def _wgrad_ws_bytes(n: int, m: int, k: int) -> int:
    return int(_lib.load().segger_linear_wgrad_workspace_bytes(n, m, k))


def _seed_parts(seed):
    """``seed`` is an int, or ``(int, device int64 tensor)``: the kernels then use ``int + *tensor`` read at
    run time, so a captured hipGraph draws a new dropout mask on every replay."""
    if isinstance(seed, tuple):
        value, dev = seed
        return int(value) & 0xFFFFFFFFFFFFFFFF, (None if dev is None else dev.data_ptr())
    return int(seed) & 0xFFFFFFFFFFFFFFFF, None


def _bits_ptr(bits: Tensor, n_edges: int) -> int:
    if bits.dtype != torch.uint8 or bits.numel() != n_edges or not bits.is_contiguous():
        raise ValueError("keep_bits must be a contiguous uint8 tensor with one entry per edge slot")
    return bits.data_ptr()


# ---- deferred partial sums (csrc/reduce.hip) ----------------------------------------------------------------
_DEFER_KEEP: Optional[list] = None


class deferred_reductions:
    """Inside this context the final sums of per-workgroup partials (weight / bias gradients of every projection,
    grad_att / grad_bias of every conv) are queued instead of launched; leaving it runs them all as ONE kernel
    (``segger_reductions_flush``).  The gradient TENSORS handed out meanwhile are placeholders: nothing may read them
    before the context exits, so this is for callers that hold the gradients themselves (``torch.autograd.grad`` in
    ``train_step_graph``), not for ``loss.backward()`` into ``.grad`` accumulators.  Workspaces are kept alive here."""

    def __init__(self, device):
        self.device = device

    def __enter__(self):
        global _DEFER_KEEP
        if _DEFER_KEEP is not None:
            raise RuntimeError("deferred_reductions does not nest")
        with _lib.on_device(self.device):        # the table is pinned to the device current HERE and to the stream of the
            rc = _lib.load().segger_reductions_defer_begin()     # first producer: a backward elsewhere sums for itself
        _lib.check(rc, "segger_reductions_defer_begin")
        _DEFER_KEEP = []
        return self

    def __exit__(self, *exc):
        global _DEFER_KEEP
        try:
            with _lib.on_device(self.device):
                rc = _lib.load().segger_reductions_flush(_lib.stream_ptr(self.device))
            _lib.check(rc, "segger_reductions_flush")
        finally:
            _DEFER_KEEP = None
        return False


def _defer_keep(*tensors) -> None:
    if _DEFER_KEEP is not None:
        _DEFER_KEEP.append(tensors)


def _f32_vec(t: Optional[Tensor], n: int, name: str) -> Optional[Tensor]:
    if t is None:
        return None
    if t.dtype == torch.float32 and t.numel() == n and t.is_contiguous():
        return t                                         # (only its data_ptr is used: the common case costs no torch call)
    t = t.detach().reshape(-1)
    if t.numel() != n:
        raise ValueError(f"{name}: expected {n} elements, got {t.numel()}")
    return t.to(torch.float32).contiguous()


# ---- "the hand-written path is off": vendor-GEMM use is counted and announced once per (site, K, M, dtype) ------------------
# The MFMA projection kernels cover segger's CLI widths (hidden 64 / 128, heads x channels = 128, 16-bit and fp32).  Another
# width (say hidden_channels=96) still WORKS -- through torch's library GEMM -- but not on this project's kernels.
# ``ops.vendor_gemm_calls`` counts those calls per (site, K, M, dtype); the first one of each kind warns.
vendor_gemm_calls: dict = {}


def _vendor_gemm(site: str, k_in: int, m_out: int, dtype) -> None:
    key = (site, int(k_in), int(m_out), str(dtype).replace("torch.", ""))
    seen = vendor_gemm_calls.get(key, 0)
    vendor_gemm_calls[key] = seen + 1
    if not seen:
        import warnings
        warnings.warn(f"segger_amd: {site} for K={k_in} -> M={m_out} ({key[3]}) is not covered by the hand-written MFMA "
                      f"kernels (segger_linear_supported / segger_linear_wgrad_supported) and runs on the vendor GEMM; "
                      f"covered widths: include/segger_amd.h. Counted in segger_amd.ops.vendor_gemm_calls.",
                      RuntimeWarning, stacklevel=3)
