"""GPU: nafp_search_topk_l2_excl (csrc/search.hip: search_topk_excl_kernel + search_merge_kernel), the exact top-k search with one
excluded row range per query, against its numpy restatement (tests/_search_excl_ref.py).

EXACT CASES.  Integer-valued sets (tests/_search_ref.py): every key and distance is exact in float32, the order is fully
determined, and ids and the BYTES of the distances are compared for equality.  The ranges are placed against the geometry of the
kernel -- a lane holds rows (r & 3) + 8 (r >> 2) + 4 hh of a 32-row block, a tile is 64 rows, 1561 rows at 5 or 129 queries are 3
splits of 9 tiles with a ragged last tile -- and every range sits inside a run of EQUAL rows that reaches two rows past either
end, queried with that very row: unmasked, the whole run is the head of the result; masked, the rows just outside the range must
come back and the rows just inside must not, so a bound that is one off, or a lane that uses its neighbour's range, changes ids.

FLOAT CASES.  No tolerance either: with every range empty the bytes are nafp_search_topk_l2's, and a masked search equals the
unmasked search over the index with the rows physically deleted (a key depends on its own row and query only, and deletion keeps
the id order)."""
import functools

import numpy as np
import pytest
import torch

import _search_excl_ref as xr
import _search_ref as sr

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
IMIN, IMAX = xr.INT32_MIN, xr.INT32_MAX


def _L():
    from neural_audio_fp_amd import _lib as L
    return L, L.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Index:
    def __init__(self, x):
        L, lib = _L()
        self.x = _dev(np.asarray(x, np.float32))
        self.n, self.d = int(self.x.shape[0]), int(self.x.shape[1])
        self.aux = torch.empty((int(lib.nafp_search_index_aux_floats(self.n)),), dtype=torch.float32, device='cuda')
        L.check(lib.nafp_search_index_prepare(L.ptr(self.x), self.n, self.d, L.ptr(self.aux), L.current_stream()), 'prepare')


def _search(q, ix, k, excl=None):
    """(D, I) numpy of the masked search (excl (nq, 2) of any ints) or, excl None, of nafp_search_topk_l2.  The workspace starts
    from NaN bytes, the outputs from sentinels."""
    L, lib = _L()
    q_t = q if torch.is_tensor(q) else _dev(np.asarray(q, np.float32))
    nq = int(q_t.shape[0])
    need = int(lib.nafp_search_workspace_bytes(nq, ix.n, k))
    assert need > 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device='cuda')
    D = torch.full((nq, k), 123.0, dtype=torch.float32, device='cuda')
    I = torch.full((nq, k), -7, dtype=torch.int32, device='cuda')
    if excl is None:
        L.check(lib.nafp_search_topk_l2(L.ptr(q_t), nq, L.ptr(ix.x), L.ptr(ix.aux), ix.n, ix.d, k, L.ptr(D), L.ptr(I), L.ptr(ws), need,
                                        L.current_stream()), 'search_topk_l2')
    else:
        e_t = _dev(np.asarray(excl, np.int64).reshape(nq, 2).astype(np.int32))
        L.check(lib.nafp_search_topk_l2_excl(L.ptr(q_t), nq, L.ptr(ix.x), L.ptr(ix.aux), ix.n, ix.d, k, L.ptr(e_t), L.ptr(D), L.ptr(I),
                                             L.ptr(ws), need, L.current_stream()), 'search_topk_l2_excl')
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy()


def _assert_same(got, want, what):
    bad = np.nonzero((got[1] != want[1]).any(1) | (got[0].view(np.uint32) != want[0].view(np.uint32)).any(1))[0]
    if len(bad):
        r = bad[0]
        raise AssertionError(f'{what}: {len(bad)} query rows differ; row {r}: ids {got[1][r].tolist()} / want {want[1][r].tolist()}, '
                             f'dist {got[0][r].tolist()} / want {want[0][r].tolist()}')


# ---- range placement against the lane layout, the tiles and the splits ------------------------------------------------------

def _ranges(n):
    """The ranges of the issue that fit an index of n rows (the last one reaches, or passes, the end of the index)."""
    out = [(3, 4), (4, 5), (3, 5), (0, 7), (30, 34), (62, 66)]
    if n >= 1561:
        out += [(574, 578), (1530, 1561)]
    else:
        out += [(n - 5, n + 3)]                                     # hi beyond n: clipped
    return out


EMPTY = [(0, 0), (5, 5), (7, 3), (-5, -1), (IMAX, IMIN), (IMIN, 0), (IMAX, IMAX), (IMIN, IMIN)]


@functools.lru_cache(maxsize=None)
def _placed(n, nq, d, k):
    """(q, x, excl): exact_set's index with a run of equal rows around every range (two rows past either end) and the queries
    that ask for those rows: even queries carry the ranges in turn, the odd query after each asks for the same row with an EMPTY
    range (one of the degenerate pairs in turn), so neighbouring lanes of a wave differ in their ranges and in nothing else."""
    _, x = sr.exact_set(n, 1, d, 1, 31)
    x = x.copy()
    rng = np.random.default_rng([n, d, 7])
    ranges = _ranges(n)
    vec = {}
    for lo, hi in ranges:
        a, b = max(0, lo - 2), min(n, hi + 2)
        v = None
        for (l2, h2), v2 in vec.items():                            # overlapping runs share their row
            if max(0, l2 - 2) < b and a < min(n, h2 + 2):
                v = v2
        vec[(lo, hi)] = rng.integers(-1, 2, size=d).astype(np.float32) if v is None else v
        x[a:b] = vec[(lo, hi)]
    q = np.empty((nq, d), np.float32)
    excl = np.empty((nq, 2), np.int64)
    for j in range(nq):
        r = ranges[(j // 2) % len(ranges)]
        q[j] = vec[r]
        excl[j] = r if j % 2 == 0 else EMPTY[(j // 2) % len(EMPTY)]
    if nq >= 129:                                                   # the last lane of a block, the first two of the ragged block
        excl[126], excl[127], excl[128] = ranges[4], ranges[5], ranges[-1]
        q[126], q[127], q[128] = vec[ranges[4]], vec[ranges[5]], vec[ranges[-1]]
    return q, x, excl


PLACED = [(65, 16, 64, 20), (65, 129, 128, 1), (129, 16, 256, 21), (129, 129, 64, 32), (1089, 16, 128, 32), (1089, 129, 256, 20),
          (1561, 5, 64, 21), (1561, 16, 128, 20), (1561, 16, 256, 32), (1561, 129, 128, 21), (1561, 129, 64, 1), (1561, 129, 256, 20),
          (1561, 5, 128, 32)]


@pytest.mark.parametrize('n,nq,d,k', PLACED, ids=lambda v: str(v))
def test_ranges_against_lanes_tiles_and_splits(nafp, n, nq, d, k):
    q, x, excl = _placed(n, nq, d, k)
    if n == 1561:                                                   # 3 splits of 9 tiles: a boundary at row 576, a ragged last tile
        assert sr.plan_splits(nq, n, sr.template_k(k)) == (3, 9) and xr.split_boundaries(nq, n, k) == [576, 1152]
        _, lib = _L()
        assert int(lib.nafp_search_workspace_bytes(nq, n, k)) == nq * 2 * 3 * sr.template_k(k) * 8 + 256
    ix = Index(x)
    got = _search(q, ix, k, excl)
    want = xr.topk_excl_exact(q, x, k, excl)
    _assert_same(got, want, f'n {n} nq {nq} d {d} k {k}')
    mask = xr.excluded_mask(excl, n)
    for r in range(nq):
        ids = got[1][r][got[1][r] >= 0]
        assert not mask[r, ids].any(), (r, excl[r].tolist(), ids.tolist())
    if k >= 20:                                                     # the rows just outside a range come back, at distance 0
        for r in range(0, nq, 2):
            lo, hi = int(excl[r, 0]), min(int(excl[r, 1]), n)
            if hi - lo > 8:
                continue
            near = [c for c in (lo - 2, lo - 1, hi, hi + 1) if 0 <= c < n]
            assert set(near) <= set(got[1][r].tolist()) and (got[0][r][np.isin(got[1][r], near)] == 0).all(), (r, lo, hi)
            # the neighbour with the empty range returns the very rows this query must not
            if r + 1 < nq and r + 1 not in (126, 127, 128):
                assert set(range(lo, hi)) <= set(got[1][r + 1].tolist()), (r + 1, lo, hi)
    _assert_same(_search(q, ix, k, excl), got, 'run to run')


# ---- the post-filter trap ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('d,k', [(64, 20), (128, 32), (256, 20), (128, 1), (64, 21)])
def test_more_than_k_excluded_rows_are_nearer_than_the_k_survivors(nafp, d, k):
    """k + 8 copies of the query inside its range, all at distance 0; the k true nearest lie outside it, one in every other
    tile and in all three splits.  A search that filtered a k-wide list afterwards would have nothing left."""
    n = sr.PLACED_N
    rng = np.random.default_rng([d, k, 3])
    x = rng.integers(-1, 2, size=(n, d)).astype(np.float32)
    v = rng.integers(-1, 2, size=d).astype(np.float32)
    lo, hi = 700, 700 + k + 8                                       # (crosses the tile boundary at 704)
    x[lo:hi] = v
    stride = ((n - 4) // (max(k, 8) + 2)) | 1                       # odd: the rows fall on every lane position in turn
    pos = [p for p in range(3, n, stride) if not lo <= p < hi]
    assert len(pos) >= k and len({p // 64 for p in pos}) >= min(k, 8) and {p // 576 for p in pos} == {0, 1, 2}
    for j, p in enumerate(pos):
        x[p] = v
        x[p, j % d] += 1 + j % 2                                   # distance 1 or 4: ties among them, far nearer than a random row
    q = np.stack([v, x[5], v, x[n - 1], v])
    excl = np.array([(lo, hi), (0, 0), (lo, hi), (5, 2), (lo - 3, hi + 3)], np.int64)
    got = _search(q, Index(x), k, excl)
    _assert_same(got, xr.topk_excl_exact(q, x, k, excl), 'post-filter trap')
    for r in (0, 2, 4):
        assert (got[1][r] >= 0).all() and set(got[1][r].tolist()) <= set(pos) and got[0][r].max() <= 4
    unmasked = _search(q, Index(x), k)
    assert ((unmasked[1][0] >= lo) & (unmasked[1][0] < hi)).all()    # without the range the list of k holds nothing else


# ---- too few survivors, degenerate pairs, ties -------------------------------------------------------------------------------

@pytest.mark.parametrize('d,k', [(128, 20), (64, 32), (256, 21)])
def test_too_few_survivors_and_degenerate_pairs(nafp, d, k):
    n = 65
    q, x = sr.exact_set(n, 12, d, 1, 41)
    excl = np.array([(3, 60), (0, n), (IMIN, IMAX), (IMAX, IMIN), (9, 4), (-7, 3), (60, 1000), (IMIN, 2), (63, IMAX), (-1, 0), (n, n + 1),
                     (0, n - 1)], np.int64)
    got = _search(q, Index(x), k, excl)
    _assert_same(got, xr.topk_excl_exact(q, x, k, excl), 'n = 65')
    present = (got[1] >= 0).sum(1)
    assert present[0] == min(k, 8) and (got[1][0, 8:] == -1).all() and np.isposinf(got[0][0, 8:]).all()
    for r in (1, 2):                                                # the whole index excluded
        assert (got[1][r] == -1).all() and np.isposinf(got[0][r]).all()
    _assert_same(tuple(a[[3, 4, 9, 10]] for a in got), tuple(a[[3, 4, 9, 10]] for a in _search(q, Index(x), k)), 'pairs that exclude nothing')
    assert present[11] == 1 and got[1][11, 0] == n - 1
    assert not np.isin(got[1][5], [0, 1, 2]).any() and not np.isin(got[1][6], range(60, 65)).any()
    assert not np.isin(got[1][7], [0, 1]).any() and not np.isin(got[1][8], [63, 64]).any()


@pytest.mark.parametrize('d,k', [(128, 20), (64, 1), (256, 32)])
def test_equal_rows_half_inside_a_range_come_in_id_order(nafp, d, k):
    n = 129
    q, x = sr.exact_set(n, 5, d, 1, 43)
    x, q = x.copy(), q.copy()
    x[40:56] = x[40]                                                # 16 equal rows; 44 .. 51 excluded
    x[100:104] = x[40]
    q[0] = q[3] = x[40]
    excl = np.array([(44, 52), (0, 0), (44, 52), (48, 101), (0, 0)], np.int64)
    got = _search(q, Index(x), k, excl)
    _assert_same(got, xr.topk_excl_exact(q, x, k, excl), 'ties')
    assert got[1][0, :min(k, 12)].tolist() == [40, 41, 42, 43, 52, 53, 54, 55, 100, 101, 102, 103][:k]
    assert got[1][3, :min(k, 11)].tolist() == [40, 41, 42, 43, 44, 45, 46, 47, 101, 102, 103][:k]


# ---- empty ranges: the bytes of the unmasked search ----------------------------------------------------------------------------

@pytest.mark.parametrize('kind,n,nq,d,k', [('exact', 1089, 129, 128, 20), ('unit', 1089, 129, 128, 20), ('exact', 1561, 5, 64, 32),
                                           ('unit', 129, 129, 256, 21)])
def test_empty_ranges_give_the_bytes_of_the_unmasked_search(nafp, kind, n, nq, d, k):
    if kind == 'exact':
        q, x = sr.exact_set(n, nq, d, 2, 47)
    else:
        q, x = sr.unit_rows(nq, d, 2), sr.unit_rows(n, d, 1)
    ix = Index(x)
    excl = np.array([EMPTY[j % len(EMPTY)] for j in range(nq)], np.int64)
    _assert_same(_search(q, ix, k, excl), _search(q, ix, k), f'{kind}: empty ranges')


# ---- deletion equivalence on float data ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('d,k,lo,hi', [(128, 20, 500, 540), (64, 32, 0, 7), (256, 20, 1060, 1089), (128, 21, 62, 66), (128, 32, 3, 4)])
def test_masked_search_equals_search_over_the_index_with_the_rows_deleted(nafp, d, k, lo, hi):
    n, nq = 1089, 129
    x = sr.unit_rows(n, d, 1)
    q = sr.unit_rows(nq, d, 2)
    q[::3] = x[np.arange(lo - 2, lo - 2 + len(q[::3])) % n]          # a third of the queries are index rows in and around the range
    keep = np.concatenate([np.arange(0, lo), np.arange(hi, n)])
    got = _search(q, Index(x), k, np.tile([(lo, hi)], (nq, 1)))
    Dd, Id = _search(q, Index(x[keep]), k)
    _assert_same(got, (Dd, np.where(Id >= 0, keep[np.maximum(Id, 0)], -1).astype(np.int32)), f'deletion of [{lo}, {hi})')
    assert (got[1] >= 0).all() and not ((got[1] >= lo) & (got[1] < hi)).any()


# ---- self-join -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('d,k', [(128, 20), (64, 32), (256, 20)])
def test_self_join_over_ragged_tracks(nafp, d, k):
    """Every index row is a query and its own track is excluded: the launch `duplicates` makes.  exact_set copies a quarter of
    the rows, so many a query has its equal in another track -- and several in its own."""
    n = 1089
    _, x = sr.exact_set(n, 1, d, 1, 53)
    lens = [1, 2, 63, 64, 65, 130, 7, 257, 31, 33, 128, 200]
    first = np.concatenate([[0], np.cumsum(lens + [n - sum(lens)])])
    assert first[-1] == n and (np.diff(first) > 0).all()
    tr = np.searchsorted(first, np.arange(n), side='right') - 1
    excl = np.stack([first[tr], first[tr + 1]], 1)
    got = _search(x, Index(x), k, excl)
    assert not ((got[1] >= excl[:, :1]) & (got[1] < excl[:, 1:])).any()
    _assert_same(got, xr.topk_excl_exact(x, x, k, excl), 'self-join')
    assert (got[0][:, 0] == 0).mean() > 0.1                          # copies in other tracks are found at distance 0


# ---- non-finite rows ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('d,k', [(128, 20), (64, 32), (256, 20)])
def test_non_finite_rows(nafp, d, k):
    n = 129
    q, x = sr.exact_set(n, 6, d, 1, 59)
    q, x = q.copy(), x.copy()
    clean = x.copy()
    x[10] = np.nan
    x[70, 3] = np.inf
    x[33, d - 1] = -np.inf                                           # inside query 0's range as well
    q[2, 5] = np.nan
    q[0] = clean[10]                                                 # the row that was at distance 0 before it became NaN
    excl = np.array([(20, 40), (0, 0), (20, 40), (60, 80), (5, 15), (IMIN, IMAX)], np.int64)
    got = _search(q, Index(x), k, excl)
    bad = [10, 33, 70]
    dist = sr.exact_distances(np.where(np.isnan(q), 0, q), clean).astype(np.float64)
    dist[:, bad] = np.inf
    dist[xr.excluded_mask(excl, n)] = np.inf
    Dw, Iw = sr._select(dist, k)
    Dw, Iw = Dw.astype(np.float32), Iw.astype(np.int32)
    Dw[2], Iw[2] = np.inf, -1                                        # a NaN query: k times -1, +inf
    _assert_same(got, (Dw, Iw), 'non-finite rows')
    assert not np.isin(got[1], bad).any() and (got[1][2] == -1).all() and (got[1][5] == -1).all()
    assert (got[1][[0, 1, 3, 4]] >= 0).all()


# ---- launch independence -----------------------------------------------------------------------------------------------------------

def test_a_query_does_not_depend_on_what_shares_the_launch(nafp):
    n, nq, d, k = 1561, 129, 128, 20
    q, x, excl = _placed(n, nq, d, k)
    ix = Index(x)
    full = _search(q, ix, k, excl)
    _assert_same(_search(q, ix, k, excl), full, 'run twice')
    for r in (0, 14, 63, 64, 126, 127, 128):
        one = _search(q[r:r + 1], ix, k, excl[r:r + 1])
        _assert_same(one, (full[0][r:r + 1], full[1][r:r + 1]), f'query {r} alone')
    part = _search(q[120:129], ix, k, excl[120:129])                 # other lanes, another block, another split plan input
    _assert_same(part, (full[0][120:129], full[1][120:129]), 'queries 120 .. 128 on their own')


# ---- status codes ------------------------------------------------------------------------------------------------------------------

def test_status_codes_leave_the_outputs_untouched(nafp):
    L, lib = _L()
    n, nq, d, k = 129, 5, 128, 20
    q, x = sr.exact_set(n, nq, d, 1, 61)
    ix = Index(x)
    q_t = _dev(q)
    e_t = _dev(np.zeros((nq, 2), np.int32))
    need = int(lib.nafp_search_workspace_bytes(nq, n, k))
    ws = torch.zeros((need,), dtype=torch.uint8, device='cuda')
    D = torch.full((nq, 33), 123.0, dtype=torch.float32, device='cuda')
    I = torch.full((nq, 33), -7, dtype=torch.int32, device='cuda')

    def call(excl=e_t, kk=k, dim=d, wsb=need, query=q_t):
        return lib.nafp_search_topk_l2_excl(L.ptr(query), nq, L.ptr(ix.x), L.ptr(ix.aux), n, dim, kk, L.ptr(excl), L.ptr(D), L.ptr(I),
                                            L.ptr(ws), wsb, L.current_stream())
    assert call(excl=None) == INVALID
    assert call(query=None) == INVALID
    assert call(kk=33) == UNSUPPORTED
    assert call(kk=0) == INVALID
    assert call(dim=100) == UNSUPPORTED
    assert call(wsb=need - 1) == WORKSPACE
    torch.cuda.synchronize()
    assert bool((D == 123.0).all()) and bool((I == -7).all())
    assert lib.nafp_last_hip_error() == 0
