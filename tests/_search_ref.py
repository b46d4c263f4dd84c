"""Exact and float64 references, a-priori error bound, input sets and mutants for the exact top-k search (csrc/search.hip:
search_topk_body + search_merge_kernel, and the same body under nafp_ivf_flat_search).  Plain numpy, no GPU code: imported by
tests/test_search_ref_host.py (CPU) and tests/test_gpu_search_edges.py (GPU), so both see the same arrays.

EXACT ARITHMETIC.  On vectors with small integer entries stored as float32 every product, every partial sum in any order, the
half norm |x|^2/2 (a multiple of 0.5), the key q.x - |x|^2/2 and the distance |q|^2 - 2 key are integers or half-integers far
below 2^24: float32 computes them without rounding, whatever the accumulation order of the matrix instructions.  The result of
the search is then determined bit for bit: `topk_exact` computes the distances in int64 and orders by (distance, id); the
distances written are those integers as float32.  A comparison on these sets is np.array_equal on the ids and on the BYTES of
the distances, with no tie tolerance.  `exactness_margin` returns the magnitudes the premise rests on.

FLOAT INPUTS.  `topk_f64` orders by the float64 distance sum_i (q_i - x_i)^2 and `dist_bound` bounds the error of the float32
distance the library writes for one (query, row) pair, term by term; u = 2^-24, gamma_n = n u / (1 - n u) (valid for a sum of n
rounded terms in ANY order), d the dimension, xx = |x|^2, qq = |q|^2, S = sum_i |q_i x_i|, all in float64:
  half norm   h = fl(0.5 fl(sum x_i^2)): d rounded products, d - 1 additions in some order, the halving exact:
              e_h = gamma_d xx / 2
  key         the accumulator starts at -h and takes the d products q_i x_i (matrix instructions, order and internal rounding
              unspecified): a sum of d + 1 terms of which d are rounded products; gamma_{d+2} leaves one rounding to spare:
              e_key = e_h + gamma_{d+2} (xx / 2 + e_h + S)
  qq          d rounded squares summed by lane and then across the wave: e_qq = gamma_d qq
  distance    fl(qq - 2 key): the doubling is exact, the subtraction rounds once, relative to the computed difference; the
              clamp at 0 moves a negative value TOWARDS the true one (which is >= 0), so it adds nothing:
              bound = e + u (dist + e),  e = e_qq + 2 e_key
Nothing here was fitted to GPU output; for unit vectors at d = 128 the bound is about 650 u = 3.9e-5.  Inputs are assumed far
from under- and overflow (the tests scale by at most 2^+-10).

`check` is the comparison of the float GPU tests (its docstring states the rules).

MUTANTS.  `mutate=NAME` makes one deliberate error of the kind the kernel could make; tests/test_search_ref_host.py asserts that
every mutant fails the GPU tests' own comparison on every input set it applies to (`applies` states when, from the geometry and the
unmutated reference alone):
  tie_larger_id            ties go to the larger id (a flipped tie-break)
  kth_keeps_later          of the rows tied with the k-th place the later ones are kept (>= for > in the insertion)
  halves_swapped           the two 4-row halves of each 8-row group swapped (the 4 * hh term of the row mapping)
  split_last_tile_dropped  the last 64-row tile of every index split is skipped (tiles per split one short)
  ragged_last_row_dropped  the last row of a partial last tile is lost (a bound one short)
  clamp_missing            float sets only: the distance is qq - 2 key in float32 without the clamp at 0
  k20_truncated            k > 20 served by the 20-entry lists: columns 20.. are padding
"""
import collections
import functools

import numpy as np

U = 2.0 ** -24
TILE_ROWS = 64
MUTANTS = ('tie_larger_id', 'kth_keeps_later', 'halves_swapped', 'split_last_tile_dropped', 'ragged_last_row_dropped',
           'clamp_missing', 'k20_truncated')


def template_k(k):
    """The compiled list length that serves k results."""
    return 20 if k <= 20 else 32


def plan_splits(nq, n, K):
    """(splits, tiles per split) of a launch: the restatement of plan_splits in csrc/search.hip the split mutants need.  The GPU
    test reads the split count from nafp_search_workspace_bytes and holds this restatement to it."""
    n_tiles = (n + TILE_ROWS - 1) // TILE_ROWS
    q_tiles = (nq + 127) // 128
    s = max(1, 2048 // max(q_tiles, 1))
    s = min(s, max(1, n_tiles // 8))
    s = min(s, 4096 // (2 * K))
    tps = (n_tiles + s - 1) // s
    return (n_tiles + tps - 1) // tps, tps


def split_cap(K):
    return 4096 // (2 * K)


def _mutate_dist(dist, k, mutate, nq_launch):
    """The distance matrix as a mutant of the row handling sees it: +inf = the row is never a candidate."""
    nq, n = dist.shape
    if mutate == 'halves_swapped':
        n8 = (n + 7) // 8 * 8
        src = np.arange(n8) ^ 4
        out = np.full((nq, n8), np.inf)
        out[:, src < n] = dist[:, src[src < n]]
        return out
    if mutate == 'split_last_tile_dropped':
        splits, tps = plan_splits(nq_launch, n, template_k(k))
        n_tiles = (n + TILE_ROWS - 1) // TILE_ROWS
        out = dist.copy()
        for s in range(splits):
            t = min(n_tiles, (s + 1) * tps) - 1
            out[:, t * TILE_ROWS:(t + 1) * TILE_ROWS] = np.inf
        return out
    if mutate == 'ragged_last_row_dropped' and n % TILE_ROWS:
        out = dist.copy()
        out[:, n - 1] = np.inf
        return out
    return dist


def _select(dist, k, mutate=None, nq_launch=None):
    """(D float64, I int64) of shape (nq, k): the k smallest of each row of `dist` (float64, +inf = absent) by (distance, id),
    padded with +inf / -1."""
    assert mutate is None or mutate in MUTANTS, mutate
    nq = dist.shape[0]
    dist = _mutate_dist(dist, k, mutate, nq if nq_launch is None else nq_launch)
    n = dist.shape[1]
    kk = 20 if (mutate == 'k20_truncated' and k > 20) else k
    cols = np.arange(n)
    if n > 8 * kk:                                                # sort only the columns that reach some row's k-th distance
        kth = np.partition(dist, kk - 1, axis=1)[:, kk - 1]
        cols = np.nonzero((dist <= kth[:, None]).any(0))[0]
    sub = dist[:, cols]
    ids = np.broadcast_to(cols, sub.shape)
    order = cols[np.lexsort((-ids if mutate == 'tie_larger_id' else ids, sub), axis=1)[:, :kk]]
    if mutate == 'kth_keeps_later' and n > kk:
        order = order.copy()
        for r in range(nq):
            dk = dist[r, order[r, kk - 1]]
            if not np.isfinite(dk):
                continue
            group = np.nonzero(dist[r] == dk)[0]
            m = int((dist[r, order[r]] == dk).sum())
            order[r, kk - m:] = group[len(group) - m:]
    D = np.take_along_axis(dist, order, 1)
    I = np.where(np.isfinite(D), order, -1).astype(np.int64)
    D = np.where(I >= 0, D, np.inf)
    if D.shape[1] < k:
        pad = k - D.shape[1]
        D = np.concatenate([D, np.full((nq, pad), np.inf)], 1)
        I = np.concatenate([I, np.full((nq, pad), -1, np.int64)], 1)
    return D, I


_MEMO = collections.OrderedDict()


def _memo(fn):
    """The last few results of fn(q, x) for the very same array objects (which nobody modifies in place; neither are the results):
    a set's mutants and checks share one distance matrix."""
    @functools.wraps(fn)
    def wrapped(q, x):
        key = (fn.__name__, id(q), id(x))
        hit = _MEMO.get(key)
        if hit is not None and hit[0] is q and hit[1] is x:
            return hit[2]
        out = fn(q, x)
        _MEMO[key] = (q, x, out)
        while len(_MEMO) > 6:
            _MEMO.popitem(last=False)
        return out
    return wrapped


@_memo
def exact_distances(q, x):
    """(nq, n) int64 |q - x|^2 of integer-valued arrays."""
    qi, xi = np.asarray(q).astype(np.int64), np.asarray(x).astype(np.int64)
    assert np.array_equal(qi, np.asarray(q)) and np.array_equal(xi, np.asarray(x)), 'the exact reference takes integer entries'
    return (qi * qi).sum(1)[:, None] + (xi * xi).sum(1)[None, :] - 2 * (qi @ xi.T)


def topk_exact(q, x, k, mutate=None, nq_launch=None):
    """(D float32, I int32), (nq, k): the (distance, id) lexicographic order in int64; fewer than k rows: id -1, +inf.
    nq_launch: the number of queries of the launch q is a sample of (it decides the split plan a split mutant follows)."""
    D, I = _select(exact_distances(q, x).astype(np.float64), k, mutate, nq_launch)
    return D.astype(np.float32), I.astype(np.int32)


def exactness_margin(q, x):
    """{'products', 'xx', 'dist'}: the largest sum_i |q_i x_i|, |x|^2 and distance: all must stay below 2^24."""
    qi, xi = np.asarray(q).astype(np.int64), np.asarray(x).astype(np.int64)
    return {'products': int((np.abs(qi) @ np.abs(xi).T).max()), 'xx': int(max((xi * xi).sum(1).max(), (qi * qi).sum(1).max())),
            'dist': int(exact_distances(q, x).max())}


def tie_shares(q, x, k):
    """(share of queries with a tie straddling the k-th place, share with a tie inside their top-k) of an exact set."""
    dist = np.sort(exact_distances(q, x), axis=1)
    if dist.shape[1] <= k:
        return 0.0, float((np.diff(dist, axis=1) == 0).any(1).mean()) if dist.shape[1] > 1 else 0.0
    straddle = dist[:, k - 1] == dist[:, k]
    inside = (np.diff(dist[:, :k], axis=1) == 0).any(1) if k > 1 else np.zeros(len(dist), bool)
    return float(straddle.mean()), float(inside.mean())


# ---- float inputs ------------------------------------------------------------------------------------------------

def _gamma(n):
    return n * U / (1.0 - n * U)


def f64_distances(q, x):
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    out = np.empty((len(q), len(x)))
    for r in range(len(q)):                                      # sum (q - x)^2: exactly 0 for a row queried with itself
        out[r] = ((x - q[r]) ** 2).sum(1)
    return out


def dist_bound(q, x, dist=None):
    """(nq, n): the a-priori bound of |float32 distance written - float64 distance| (module docstring)."""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    d = q.shape[1]
    dist = f64_distances(q, x) if dist is None else dist
    xx, qq = (x * x).sum(1), (q * q).sum(1)
    S = np.abs(q) @ np.abs(x).T
    e_h = _gamma(d) * xx / 2
    e_key = e_h[None, :] + _gamma(d + 2) * ((xx / 2 + e_h)[None, :] + S)
    e = _gamma(d) * qq[:, None] + 2 * e_key
    return e + U * (dist + e)


def _finite_rows(x):
    return np.isfinite(np.asarray(x, np.float64)).all(1)


@_memo
def _f64_tables(q, x):
    """Distances and bounds with the non-finite index rows absent (+inf distance, never expected)."""
    ok = _finite_rows(x)
    xs = np.where(ok[:, None], np.asarray(x, np.float64), 0.0)
    dist = f64_distances(q, xs)
    bound = dist_bound(q, xs, dist)
    dist[:, ~ok] = np.inf
    return dist, bound


def topk_f64(q, x, k, mutate=None, nq_launch=None):
    """(D float64, I int64, bound float64), (nq, k): the float64 order (distance, id) over the finite index rows and the bound of
    each returned pair (+inf in the padding).  `clamp_missing` returns float32 distances formed as the kernel forms them, less
    the clamp."""
    dist, bound = _f64_tables(q, x)
    D, I = _select(dist, k, None if mutate == 'clamp_missing' else mutate, nq_launch)
    if mutate == 'halves_swapped':
        return D, I, None
    B = np.where(I >= 0, np.take_along_axis(bound, np.maximum(I, 0), 1), np.inf)
    if mutate == 'clamp_missing':
        q32, x32 = np.asarray(q, np.float32), np.asarray(x, np.float32)
        key = (q32 @ x32.T - np.float32(0.5) * (x32 * x32).sum(1, dtype=np.float32)[None, :]).astype(np.float32)
        d32 = ((q32 * q32).sum(1, dtype=np.float32)[:, None] - np.float32(2) * key).astype(np.float32)
        D = np.where(I >= 0, np.take_along_axis(d32, np.maximum(I, 0), 1), np.inf)
    return D, I, B


def check(D, I, q, x, k):
    """The comparison of the float GPU tests; raises AssertionError, returns the worst observed / bound ratios
    {'dist', 'column', 'missing'} (all must be below 1).  Non-finite index rows are absent from the reference.
      - shape; ids in [0, n) and distinct within a row, or -1 with +inf, the padding only after min(k, rows present) results;
      - dist:    |D[r, c] - d64(r, I[r, c])| <= bound(r, I[r, c]);
      - D is non-decreasing along a row and never negative;
      - column:  |d64(r, I[r, c]) - Dref[r, c]| <= bound(r, I[r, c]): the returned row's float64 distance against the reference's
                 distance in the same column (an order by keys that are each off by at most e can move a column's distance by
                 2 e, so one bound is stricter than what the arithmetic guarantees in the worst case; it is what is asked);
      - missing: an id the reference has and the result lacks is legitimate only if its float64 distance is within
                 bound(missing) + bound(k-th) of the float64 distance of the result's k-th row."""
    D, I = np.asarray(D), np.asarray(I).astype(np.int64)
    nq, n = len(q), len(x)
    assert D.shape == (nq, k) and I.shape == (nq, k), (D.shape, I.shape)
    dist, bound = _f64_tables(q, x)
    Dref, Iref = _select(dist, k)
    present = I >= 0
    assert np.array_equal(present, Iref >= 0), 'padding differs from the reference'
    assert (I[present] < n).all(), 'an id beyond the index'
    assert np.isposinf(D[~present]).all(), 'padding distance is not +inf'
    worst = {'dist': 0.0, 'column': 0.0, 'missing': 0.0}
    if not present.any():
        return worst
    Dm = np.where(present, D.astype(np.float64), 0.0)
    assert not np.isnan(D).any() and (Dm >= 0).all(), 'a negative or NaN distance'
    assert (np.diff(Dm, axis=1)[present[:, 1:]] >= 0).all(), 'distances decrease along a row'
    Ic = np.maximum(I, 0)
    srt = np.sort(np.where(present, I, -np.arange(1, k + 1)[None, :]), axis=1)
    assert (np.diff(srt, axis=1) != 0).all(), 'an id returned twice'
    d_own = np.take_along_axis(dist, Ic, 1)
    b_own = np.take_along_axis(bound, Ic, 1)
    assert np.isfinite(d_own[present]).all(), 'a non-finite index row was returned'
    with np.errstate(invalid='ignore'):
        worst['dist'] = float((np.abs(Dm - d_own) / b_own)[present].max())
        worst['column'] = float((np.abs(d_own - Dref) / b_own)[present].max())
    for r in range(nq):
        if not present[r].all():
            continue                                             # fewer rows than k: nothing can be missing
        miss = np.setdiff1d(Iref[r], I[r])
        if len(miss):
            kth = I[r, k - 1]
            ratio = np.abs(dist[r, miss] - dist[r, kth]) / (bound[r, miss] + bound[r, kth])
            worst['missing'] = max(worst['missing'], float(ratio.max()))
    for what, v in worst.items():
        assert v < 1.0, (what, v)
    return worst


# ---- input sets --------------------------------------------------------------------------------------------------

def exact_set(n, nq, d, amax, seed):
    """(q, x) float32 with integer entries: x uniform in {-amax..amax}; for n >= 16 a quarter of the rows 1 .. n-2 are copies of
    other such rows (ties at every place, also the first); query j is index row r_j (r_0 = n - 1, r_1 = 0, the rest drawn), the
    odd j perturbed by {-1, 0, 1} per entry.  Rows 0 and n - 1 are never part of a copy, so query 0 has one nearest row, the
    last."""
    rng = np.random.default_rng([seed, n, nq, d, amax])
    x = rng.integers(-amax, amax + 1, size=(n, d))
    if n >= 16:
        m = n // 4
        dst = 1 + rng.permutation(n - 2)[:m]
        pool = np.setdiff1d(np.arange(1, n - 1), dst)
        x[dst] = x[rng.choice(pool, size=m)]
    rows = rng.integers(0, n, size=nq)
    rows[0] = n - 1
    if nq > 1:
        rows[1] = 0
    q = x[rows].copy()
    q[1::2] += rng.integers(-1, 2, size=q[1::2].shape)
    return q.astype(np.float32), x.astype(np.float32)


Case = collections.namedtuple('Case', 'name n nq d k amax seed')

N_INDEX = (1, 2, 63, 64, 65, 127, 128, 129, 959, 960, 961, 1024, 1025, 1089, 1537)
N_QUERY = (1, 127, 128, 129, 257)
DIMS = (64, 128, 256)
KS = (1, 19, 20, 21, 32)


def _geometry():
    """A pruned cross product: every n_index, n_query and k at every d, both alphabets at every d."""
    out = []
    for di, d in enumerate(DIMS):
        for i, n in enumerate(N_INDEX):
            nq = N_QUERY[(i + di) % 5]
            k = KS[(i + i // 5 + 2 * di) % 5]
            amax = 1 + (i + di) % 2
            out.append(Case(f'n{n}-q{nq}-d{d}-k{k}-a{amax}', n, nq, d, k, amax, 100 + i))
    return out


GEOMETRY = _geometry()


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    return exact_set(case.n, case.nq, case.d, case.amax, case.seed)


@functools.lru_cache(maxsize=None)
def case_ref(case):
    q, x = case_inputs(case)
    return topk_exact(q, x, case.k)


PREFIX = Case('prefix', 1089, 129, 128, 32, 1, 5)                   # k = 1 .. 32 against the first columns of k = 32
BEHIND = tuple(Case(f'behind-n{n}-d{d}', n, 129, d, k, 1, 6) for n, d, k in ((1, 64, 20), (65, 128, 21), (961, 256, 20)))
SHORT = tuple(Case(f'short-n{n}-k{k}', n, 5, 128, k, 1, 4) for n, k in ((1, 20), (2, 32), (19, 20), (20, 21), (31, 32)))
IVF = (Case('ivf-d64-k20', 1089, 129, 64, 20, 1, 3), Case('ivf-d128-k21', 1089, 129, 128, 21, 1, 3),
       Case('ivf-d256-k32', 961, 127, 256, 32, 1, 3))
IVF_NLIST = (1, 8, 50)

# large indexes: the split count at its cap (816 tiles / 8 = 102 splits of 8 for K = 20; 512 tiles -> 64 splits for K = 32), a
# ragged last tile, and a launch whose 22 query blocks lower the split count
LARGE = (Case('large-k20', 52187, 40, 64, 20, 1, 7), Case('large-k32', 32747, 40, 64, 32, 1, 8))
LARGE_NQ_MANY = 2700


@functools.lru_cache(maxsize=None)
def large_many_queries():
    """(q (2700, 64), sample rows): the many-query launch on LARGE[0]'s index; the reference is computed for the sample, which
    holds the first and last row of several 128-query blocks."""
    _, x = case_inputs(LARGE[0])
    rng = np.random.default_rng(77)
    rows = rng.integers(0, len(x), size=LARGE_NQ_MANY)
    q = x[rows].copy()
    q[1::2] += rng.integers(-1, 2, size=q[1::2].shape).astype(np.float32)
    edges = [0, 127, 128, 255, 1279, 1280, 2559, 2560, 2687, 2688, 2699]
    sample = np.unique(np.concatenate([edges, rng.integers(0, LARGE_NQ_MANY, size=53)]))
    return q, sample


# placed duplicates: one row copied to chosen positions of a 1561-row index (25 tiles, the last of 25 rows; 3 splits of 9 tiles)
PLACED_N = 1561
_LANE_ROWS = [t * 64 + mi * 32 + 8 * (r >> 2) + (r & 3) for t in range(2) for mi in range(2) for r in range(16)]   # hh = 0


def placed_positions(k):
    """{scenario: sorted positions}, each with k + 4 copies (more than k), for the ways equal keys can meet."""
    m = k + 4
    return {
        'same_lane': _LANE_ROWS[:m],                             # rows r, r + 1 of the 4-row groups one lane owns
        'lane_halves': list(range(2, 2 + m)),                    # rows r and r + 4: the two lane halves, one tile
        'blocks': list(range(32 - m // 2, 32 - m // 2 + m)),     # across the two 32-row blocks of tile 0
        'tiles': list(range(64 - m // 2, 64 - m // 2 + m)),      # tile 0 and tile 1 of split 0
        'splits': list(range(576 - m // 2, 576 - m // 2 + m)),   # the last tile of split 0 and the first of split 1
        'ragged_tile': list(range(PLACED_N - m, PLACED_N)),      # the 25-row last tile (and, for k = 32, the tile before it)
        'scattered': list(range(3, PLACED_N, 37))[:m],           # one copy in many tiles and all splits
    }


@functools.lru_cache(maxsize=None)
def placed_set(d, k, scenario):
    """(q (5, d), x (1561, d), positions): random {-1, 0, 1} rows, the row v at `positions`; queries 0 and 4 are v itself."""
    rng = np.random.default_rng([9, d])
    x = rng.integers(-1, 2, size=(PLACED_N, d)).astype(np.float32)
    v = rng.integers(-1, 2, size=d).astype(np.float32)
    pos = placed_positions(k)[scenario]
    x[pos] = v
    q = np.stack([v, x[5], x[700], x[PLACED_N - 1], v])
    return q, x, np.asarray(pos)


PLACED_SCENARIOS = ('same_lane', 'lane_halves', 'blocks', 'tiles', 'splits', 'ragged_tile', 'scattered')


# float sets
def unit_rows(n, d, seed, scale=None):
    x = np.random.default_rng([seed, n, d]).normal(size=(n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    if scale is not None:
        x *= scale
    return x.astype(np.float32)


FloatCase = collections.namedtuple('FloatCase', 'name n nq d k kind')
FLOAT_CASES = (
    FloatCase('unit-n65-q128-d64-k19', 65, 128, 64, 19, 'unit'),
    FloatCase('unit-n961-q127-d64-k21', 961, 127, 64, 21, 'unit'),
    FloatCase('unit-n1089-q129-d128-k20', 1089, 129, 128, 20, 'unit'),
    FloatCase('unit-n1537-q257-d256-k32', 1537, 257, 256, 32, 'unit'),
    FloatCase('self-n1089-q129-d128-k20', 1089, 129, 128, 20, 'self'),
    FloatCase('self-n1025-q257-d256-k1', 1025, 257, 256, 1, 'self'),
    FloatCase('norms-n1089-q129-d128-k20', 1089, 129, 128, 20, 'norms'),
    FloatCase('norms-n961-q127-d64-k32', 961, 127, 64, 32, 'norms'),
)


@functools.lru_cache(maxsize=None)
def float_inputs(case):
    """(q, x) float32.  unit: unit vectors; self: the queries are index rows (the last and the first among them) of unit
    vectors; norms: index rows with norms spread over 0.25 .. 4, so the L2 order is not the inner-product order."""
    if case.kind == 'norms':
        scale = 2.0 ** np.random.default_rng(case.n).uniform(-2, 2, size=(case.n, 1))
        return unit_rows(case.nq, case.d, 2), unit_rows(case.n, case.d, 1, scale)
    x = unit_rows(case.n, case.d, 1)
    if case.kind == 'self':
        rows = np.random.default_rng(case.nq).integers(0, case.n, size=case.nq)
        rows[0], rows[1] = case.n - 1, 0
        return x[rows].copy(), x
    return unit_rows(case.nq, case.d, 2), x


def applies(mutant, n, nq_launch, k, I_ref, straddle, inside, self_queries=False):
    """Whether `mutant` must change the result of a set: from the geometry and the unmutated reference alone.  I_ref: the
    reference ids; straddle / inside: whether some query has a tie across the k-th place / inside its top-k; self_queries: a float
    set whose queries are index rows (only there can qq - 2 key come out negative)."""
    if mutant == 'tie_larger_id':
        return inside or straddle
    if mutant == 'kth_keeps_later':
        return straddle
    if mutant == 'halves_swapped':
        return True
    if mutant == 'split_last_tile_dropped':
        splits, tps = plan_splits(nq_launch, n, template_k(k))
        n_tiles = (n + TILE_ROWS - 1) // TILE_ROWS
        last = {min(n_tiles, (s + 1) * tps) - 1 for s in range(splits)}
        return bool(np.isin(I_ref[I_ref >= 0] // TILE_ROWS, list(last)).any())
    if mutant == 'ragged_last_row_dropped':
        return n % TILE_ROWS != 0 and bool((I_ref == n - 1).any())
    if mutant == 'clamp_missing':
        return self_queries
    if mutant == 'k20_truncated':
        return k > 20 and n > 20
    raise ValueError(mutant)
