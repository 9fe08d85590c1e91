"""Index parity of the prediction head (no GPU, torch CPU and numpy only): the proof that every assignment which differs
from a float64 reference is a tie, and the designed inputs of ``test_edge_cos_argmax_every_route`` with the certificate
that they have no near-tie at all.

The proof (:func:`explain_mismatches`).  ``score_ref`` is a float64 score per edge (``oracle.edge_scores``), known to be
within ``tol`` of the scores the assignment under test was made from -- the tolerance the calling test already asserts on
the scores, never a constant of its own.  Write ``M_r`` for the reference maximum over the edges of row ``r``:

* a row without edges is exactly ``-1`` (and ``max_eid == E``, ``max_sim == 0`` where the caller has them);
* where both sides assign, the result is one of the row's own candidates (after ``dst_index``), and the best reference
  score among the row's edges that map to it is ``>= M_r - 2 tol``: each of the two candidates' scores may be off by ``tol``;
* ``-1`` against an assignment, either way round, needs ``min_similarity`` and ``|M_r - min_similarity| <= tol``.

The designed inputs (:func:`designed_case`, :func:`planted_case`).  Every row's winner is built, not drawn: the best of the
37 destination columns sits in exactly one slot of the row (first, last, middle in turn), every other slot holds another
column, and a row whose float64 top-two gap on the storage-rounded inputs is under ``2 * MIN_GAP`` is redrawn here.
:func:`certify` then demands of the float64 oracle alone that every row's maximum exceeds every other distinct score of
the row by ``MIN_GAP`` (100 times the loosest head tolerance) and lies ``MIN_GAP`` away from every similarity threshold the
case is run with -- a condition on the inputs, never a tolerance on the kernel.  Only the planted rows whose scores are
exactly -1, 0 or 1 in every storage format (zero rows, one-hot rows; ``exact_rows``) may sit on a threshold or one float32
from it: there the certificate demands those exact values instead."""
import functools

import numpy as np
import torch

HEAD_TOL = {torch.float32: 2e-6, torch.bfloat16: 1e-5, torch.float16: 1e-5}     # tests/test_gpu_heads.py::test_edge_cos_argmax
MIN_GAP = 1e-3
N_COLS = 37
DEGREES = (1, 2, 7, 64, 65, 300, 0)          # 0: empty row; 64 / 65: on and past one wave of candidates; 300: a long walk
ROWS_PER_BLOCK = {8: 256, 16: 128, 32: 64, 64: 32, 128: 16}
GENERIC_CHANNELS = (3, 20, 63, 65, 72, 200)
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
ONE_UP = float(np.nextafter(np.float32(1), np.float32(2)))
# the planted case's special destination columns and its rows
COL_E0, COL_E1, COL_NEG_E0, COL_ZERO_A, COL_ZERO_B = 30, 31, 32, 35, 36
ROW_DUP, ROW_NEG, ROW_ZERO_SRC, ROW_ZERO_DST, ROW_HOT_1, ROW_HOT_0, ROW_HOT_M1, ROW_EMPTY = range(8)


def routes():
    """-> [(kind, channels, n_rows)]: every launch route of the head.  "contiguous": the five vectorised widths at one row
    and at one row more than a block holds, the generic kernel's widths at one row and one more than a block's four; "ld": a
    16-byte aligned column slice of a wider tensor; "unaligned": a slice that starts one element in."""
    out = [("contiguous", c, n) for c, r in ROWS_PER_BLOCK.items() for n in (1, r + 1)]
    out += [("contiguous", c, n) for c in GENERIC_CHANNELS for n in (1, 5)]
    out += [("ld", 64, ROWS_PER_BLOCK[64] + 1), ("ld", 16, ROWS_PER_BLOCK[16] + 1), ("unaligned", 64, ROWS_PER_BLOCK[64] + 1)]
    return out


def route_id(route):
    return "%s-C%d-n%d" % route


def _np(t, dtype=None):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a if dtype is None else a.astype(dtype)


# ------------------------------------------------------------------------------------------------ the proof
def reference_assign(src, dst, score_ref, n_rows, dst_index=None, min_similarity=None):
    """``oracle.predict_assign`` from given scores, in numpy: -> (seg [-1 = none], row maximum [-inf = no edge], arg-max
    edge id [E = no edge]); ties go to the lowest edge id."""
    src, dst, score = _np(src, np.int64), _np(dst, np.int64), _np(score_ref, np.float64)
    E = src.size
    mapped = dst if dst_index is None else _np(dst_index, np.int64)[dst]
    top = np.full(n_rows, -np.inf)
    np.maximum.at(top, src, score)
    arg = np.full(n_rows, E, dtype=np.int64)
    is_top = score == top[src]
    np.minimum.at(arg, src[is_top], np.flatnonzero(is_top))
    valid = arg < E
    if min_similarity is not None:
        valid &= top >= min_similarity
    seg = np.full(n_rows, -1, dtype=np.int64)
    seg[valid] = mapped[arg[valid]]
    return seg, top, arg


def explain_mismatches(seg_got, src, dst, score_ref, n_rows, *, dst_index=None, min_similarity=None, tol, max_eid=None,
                       max_sim=None, label=""):
    """Assert that ``seg_got`` is the reference assignment except where the reference itself cannot tell (module docstring);
    -> (n_mismatch, worst_gap), printed before anything is asserted.  ``worst_gap``: the largest ``M_r`` minus the best
    reference score of the candidate taken instead, over the rows where both sides assign different candidates."""
    got = _np(seg_got, np.int64)
    src, dst, score = _np(src, np.int64), _np(dst, np.int64), _np(score_ref, np.float64)
    E = src.size
    assert got.shape == (n_rows,) and src.shape == dst.shape == score.shape == (E,)
    mapped = dst if dst_index is None else _np(dst_index, np.int64)[dst]
    ref, top, _ = reference_assign(src, dst, score, n_rows, dst_index, min_similarity)
    empty = np.bincount(src, minlength=n_rows) == 0
    # the best reference score among each row's edges that map to what the row was given
    taken = np.full(n_rows, -np.inf)
    hit = mapped == got[src]
    np.maximum.at(taken, src[hit], score[hit])
    differ = (got != ref) & ~empty
    swapped = differ & (got != -1) & (ref != -1)
    flipped = differ & ~swapped                                          # -1 on one side only
    stranger = (got != -1) & ~empty & np.isinf(taken)                    # assigned to what is not a candidate of the row
    with np.errstate(invalid="ignore"):                                  # (-inf) - (-inf) on rows that fail anyway
        gap = np.where(got != -1, top - taken, 0.0)
        far = np.abs(top - (np.nan if min_similarity is None else min_similarity))
    worst_gap = float(gap[swapped & ~stranger].max(initial=0.0))
    n_mismatch = int(differ.sum())
    print(f"index parity {label}: n_mismatch {n_mismatch} of {int((~empty).sum())} rows with edges, worst_gap {worst_gap:.3e}, "
          f"threshold flips {int(flipped.sum())} (farthest {float(far[flipped].max(initial=0.0)) if min_similarity is not None else 0.0:.3e}), "
          f"tol {tol:.1e}")
    bad = {
        "an empty row is not -1": empty & (got != -1),
        "assigned to a non-candidate": stranger,
        "a swap across more than 2 tol": differ & (got != -1) & ~stranger & (gap > 2 * tol),
        "-1 on one side without a similarity threshold": flipped if min_similarity is None else np.zeros(n_rows, dtype=bool),
        "a threshold flip farther than tol from the threshold": (flipped & ~(far <= tol)) if min_similarity is not None
        else np.zeros(n_rows, dtype=bool),
    }
    if max_eid is not None:
        bad["an empty row's max_eid is not E"] = empty & (_np(max_eid, np.int64) != E)
    if max_sim is not None:
        bad["an empty row's max_sim is not 0"] = empty & (_np(max_sim, np.float64) != 0)
    for what, rows in bad.items():
        for r in np.flatnonzero(rows)[:10]:
            e = np.flatnonzero(src == r)
            print(f"  row {r}: {what}; got {got[r]}, reference {ref[r]}, M_r {top[r]!r}, taken {taken[r]!r}, "
                  f"candidates {mapped[e].tolist()[:12]}, scores {score[e].tolist()[:12]}")
    failed = [f"{what} ({int(rows.sum())} rows)" for what, rows in bad.items() if rows.any()]
    assert not failed, f"index parity {label}: " + "; ".join(failed)
    return n_mismatch, worst_gap


def restrict_rows(keep, src, dst, score_ref):
    """The edges of the rows ``keep`` (bool [n_rows]) selects, those rows renumbered 0.. in order: what ``predict_step``
    returns is filtered by ``predict_mask`` the same way.  -> (src, dst, score_ref, n_rows)."""
    keep, src = _np(keep, bool), _np(src, np.int64)
    new_id = np.cumsum(keep) - 1
    e = keep[src]
    return new_id[src[e]], _np(dst, np.int64)[e], _np(score_ref, np.float64)[e], int(keep.sum())


# ------------------------------------------------------------------------------------------------ designed inputs
def _cosines(v, cols):
    v, cols = v.double(), cols.double()
    return (cols @ v) / (v.norm().clamp_min(1e-8) * cols.norm(dim=1).clamp_min(1e-8))


def _draw_row(g, z_dst, dtype, cols, accept):
    """A storage-rounded source row whose float64 cosines against ``z_dst[cols]`` pass ``accept``; -> (row, cosines)."""
    for _ in range(1000):
        v = torch.randn(z_dst.shape[1], generator=g).to(dtype)
        s = _cosines(v, z_dst[cols])
        if accept(s):
            return v, s
    raise AssertionError("no well-separated row in 1000 draws")


def _clear_top(s):
    top = s.topk(2).values
    return bool(top[0] - top[1] >= 2 * MIN_GAP and abs(top[0]) >= 2 * MIN_GAP and 1.0 - top[0] >= 2 * MIN_GAP)


def _assemble(g, rows):
    """``rows``: per row, the destination columns of its slots in order.  -> (src, dst) as a shuffled COO list whose stable
    sort by row puts each row's slots back in their order: edge ids differ from slots."""
    deg = torch.tensor([len(r) for r in rows])
    by_slot = torch.repeat_interleave(torch.arange(len(rows)), deg)
    src = by_slot[torch.randperm(int(deg.sum()), generator=g)]
    dst = torch.empty_like(src)
    dst[torch.argsort(src, stable=True)] = torch.tensor([c for r in rows for c in r], dtype=torch.int64)
    return src, dst


def _seed(channels, n_rows, dtype, salt):
    return ((channels * 1000 + n_rows) * 4 + DTYPES.index(dtype)) * 2 + salt


@functools.lru_cache(maxsize=None)
def designed_case(channels, n_rows, dtype):
    """Random rows with built winners.  Degrees cycle through ``DEGREES`` from a start that moves with the width (so the few
    rows of the generic routes cover every degree between them); the last row, alone in its block, is never the empty one."""
    g = torch.Generator().manual_seed(_seed(channels, n_rows, dtype, 0))
    z_dst = torch.randn(N_COLS, channels, generator=g).to(dtype)
    start = (list(ROWS_PER_BLOCK) + list(GENERIC_CHANNELS)).index(channels) % 6
    deg = [DEGREES[(r + start) % 7] for r in range(n_rows)]
    if deg[-1] == 0:
        deg[-1] = DEGREES[(n_rows + start) % 7]
    z_src = torch.zeros(n_rows, channels, dtype=dtype)
    rows, winner_slot, top = [], [], []
    everything = torch.arange(N_COLS)
    for r, d in enumerate(deg):
        z_src[r], s = _draw_row(g, z_dst, dtype, everything, _clear_top)
        if d == 0:
            rows.append([]); winner_slot.append(-1)
            continue
        best = int(s.argmax())
        w = (0, d - 1, d // 2)[len(top) % 3]
        others = torch.randint(0, N_COLS - 1, (d,), generator=g)
        slots = (others + (others >= best)).tolist()                     # any column but the best
        slots[w] = best
        rows.append(slots); winner_slot.append(w); top.append(float(s[best]))
    src, dst = _assemble(g, rows)
    # a similarity threshold that splits the rows: between the two middle maxima that are far enough apart
    top = sorted(top)
    mids = [(abs(i - len(top) // 2), (top[i] + top[i + 1]) / 2) for i in range(len(top) - 1) if top[i + 1] - top[i] >= 4 * MIN_GAP]
    threshold = min(mids)[1] if mids else top[0] - 0.01
    return {"z_src": z_src, "z_dst": z_dst, "src": src, "dst": dst, "n_rows": n_rows, "n_cols": N_COLS,
            "dst_index": torch.randperm(N_COLS, generator=g) + 1000, "thresholds": (None, threshold),
            "degrees": deg, "winner_slot": winner_slot}


@functools.lru_cache(maxsize=None)
def planted_case(channels, dtype):
    """Eight rows with known answers (``ROW_*``): duplicated edges, an all-negative row, a zero source row, a row whose
    candidates are zero destination rows, three rows of axis-aligned one-hot embeddings (best score exactly 1, 0, -1), an
    empty row; run with no threshold, 0, 1 and the float32 after 1."""
    g = torch.Generator().manual_seed(_seed(channels, 0, dtype, 1))
    z_dst = torch.randn(N_COLS, channels, generator=g).to(dtype)
    z_dst[COL_E0:] = 0
    z_dst[COL_E0, 0], z_dst[COL_E1, 1], z_dst[COL_NEG_E0, 0] = 1, 1, -1
    plain = torch.arange(COL_E0)
    z_src = torch.zeros(8, channels, dtype=dtype)
    rows = [[] for _ in range(8)]
    z_src[ROW_DUP], s = _draw_row(g, z_dst, dtype, plain, _clear_top)
    order = s.argsort(descending=True).tolist()
    rows[ROW_DUP] = [order[3], order[0], order[5], order[0], order[3], order[0]]      # the best column three times: slot 1 wins

    def clear_negatives(s):
        neg = s[s <= -2 * MIN_GAP].sort(descending=True).values
        return bool(neg.numel() >= 3 and neg[0] - neg[1] >= 2 * MIN_GAP)
    z_src[ROW_NEG], s = _draw_row(g, z_dst, dtype, plain, clear_negatives)
    neg = [c for c in s.argsort(descending=True).tolist() if s[c] <= -2 * MIN_GAP]
    rows[ROW_NEG] = [neg[1], neg[2], neg[0], neg[1]]                                  # the least negative in the middle
    rows[ROW_ZERO_SRC] = [5, 3, 5, 9]                                                 # (z_src row stays zero) all 0: slot 0 wins
    z_src[ROW_ZERO_DST], _ = _draw_row(g, z_dst, dtype, plain, _clear_top)
    rows[ROW_ZERO_DST] = [COL_ZERO_B, COL_ZERO_A, COL_ZERO_B]
    z_src[ROW_HOT_1, 0] = z_src[ROW_HOT_0, 0] = z_src[ROW_HOT_M1, 0] = 1
    rows[ROW_HOT_1] = [COL_E1, COL_E0, COL_NEG_E0]                                    # 0, 1, -1
    rows[ROW_HOT_0] = [COL_NEG_E0, COL_E1]                                            # -1, 0
    rows[ROW_HOT_M1] = [COL_NEG_E0]                                                   # -1
    src, dst = _assemble(g, rows)
    return {"z_src": z_src, "z_dst": z_dst, "src": src, "dst": dst, "n_rows": 8, "n_cols": N_COLS,
            "dst_index": torch.randperm(N_COLS, generator=g) + 1000, "thresholds": (None, 0.0, 1.0, ONE_UP),
            "degrees": [len(r) for r in rows], "winner_slot": [1, 2, 0, 0, 1, 1, 0, -1],
            "exact_rows": (ROW_ZERO_SRC, ROW_ZERO_DST, ROW_HOT_1, ROW_HOT_0, ROW_HOT_M1)}


def reference(case, min_similarity):
    """The float64 oracle on the storage-rounded inputs: -> (per-edge scores, max_sim, max_eid, seg)."""
    import segger_oracle as oracle
    zs, zd = case["z_src"].double(), case["z_dst"].double()
    ei = torch.stack([case["src"], case["dst"]])
    score = oracle.edge_scores(zs, zd, ei)
    seg, max_sim = oracle.predict_assign(zs, zd, ei, case["dst_index"], min_similarity)
    _, max_eid = oracle.scatter_max(score, case["src"], case["n_rows"])
    return score, max_sim, max_eid, seg


def certify(case):
    """Assert the gap condition of the module docstring from the oracle alone; -> the smallest gap met (inf if none)."""
    score = _np(reference(case, None)[0])
    src = _np(case["src"])
    assert np.isfinite(score).all()
    worst = np.inf
    for r in range(case["n_rows"]):
        s = score[src == r]
        if not s.size:
            continue
        rest = s[s != s.max()]                                           # bit-equal scores are exact ties, not near ones
        if rest.size:
            assert s.max() - rest.max() >= MIN_GAP, (r, s.max(), rest.max())
            worst = min(worst, s.max() - rest.max())
        if r in case.get("exact_rows", ()):                              # scores exact in every format: any threshold is clear
            assert np.isin(s, (-1.0, 0.0, 1.0)).all(), (r, s)
            continue
        for t in case["thresholds"]:
            if t is not None:
                assert abs(s.max() - t) >= MIN_GAP, (r, s.max(), t)
                worst = min(worst, abs(s.max() - t))
    return worst
