"""TEST INFRASTRUCTURE: the contract of nafp_search_topk_l2_excl (include/nafp.h) restated in numpy on top of tests/_search_ref.py.

Query r gets what `topk_exact` gives on the index with the rows [lo_r, hi_r) REMOVED, the ids mapped back to the rows of the
whole index.  lo and hi are clipped to [0, n] first; lo >= hi after that removes nothing.  Deleting rows keeps the order of the
ids that remain, so the (distance, id) order of the reduced index is the (distance, id) order of the survivors: the restatement
needs nothing but the unmasked reference.  Queries that share a range share one reduced index.

`topk_excl_exact` is for the integer-valued sets (`_search_ref.exact_set`): equality of ids and of the bytes of the distances.
`lane_rows` and `split_boundaries` restate the two pieces of geometry the range placements of the GPU test are chosen against."""
import numpy as np

import _search_ref as sr

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def clip_ranges(excl, n):
    """(nq, 2) any int32 pairs -> (lo, hi) int64 arrays clipped to [0, n]; lo >= hi means nothing is excluded."""
    e = np.asarray(excl, np.int64).reshape(-1, 2)
    return np.clip(e[:, 0], 0, n), np.clip(e[:, 1], 0, n)


def excluded_mask(excl, n):
    """(nq, n) bool: row c is excluded for query r."""
    lo, hi = clip_ranges(excl, n)
    c = np.arange(n)[None, :]
    return (c >= lo[:, None]) & (c < hi[:, None])


def topk_excl_exact(q, x, k, excl):
    """(D float32, I int32), (nq, k): per query the excluded rows removed, `topk_exact` on the rest, the ids mapped back."""
    q, x = np.asarray(q), np.asarray(x)
    nq, n = len(q), len(x)
    lo, hi = clip_ranges(excl, n)
    assert len(lo) == nq
    empty = hi <= lo
    lo, hi = np.where(empty, 0, lo), np.where(empty, 0, hi)         # every empty range is the same range
    D = np.full((nq, k), np.inf, np.float32)
    I = np.full((nq, k), -1, np.int32)
    for a, b in sorted({(int(a), int(b)) for a, b in zip(lo, hi)}):
        rows = np.nonzero((lo == a) & (hi == b))[0]
        keep = np.concatenate([np.arange(0, a), np.arange(b, n)])
        if not len(keep):
            continue
        d, i = sr.topk_exact(np.ascontiguousarray(q[rows]), np.ascontiguousarray(x[keep]), k)
        D[rows] = d
        I[rows] = np.where(i >= 0, keep[np.maximum(i, 0)], -1)
    return D, I


def lane_rows(hh):
    """The 16 rows of a 32-row block that the lanes of half hh hold: (r & 3) + 8 (r >> 2) + 4 hh."""
    return [(r & 3) + 8 * (r >> 2) + 4 * hh for r in range(16)]


def split_boundaries(nq, n, k):
    """The first row of every index split but the first."""
    splits, tps = sr.plan_splits(nq, n, sr.template_k(k))
    return [s * tps * sr.TILE_ROWS for s in range(1, splits)]
