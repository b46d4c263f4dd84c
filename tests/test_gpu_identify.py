"""GPU: nafp_search_identify (csrc/search.hip), the track-aware sequence matcher, against its numpy restatement
(tests/_identify_ref.py).  Track, alignment, votes, overlap and n_cand are EQUAL to the restatement; every score has the bits
nafp_search_seq_scores gives for the overlap sub-range (the existing entry point is the yardstick: the restatement ranks by those
bits) and lies within (dim + n_ov + 2) * 2^-24 of the float64 mean (unit rows: |q . x| <= 1, fp32 accumulation); a task alone
gives the bytes it gives inside a batch, and two runs give the same bytes.

The index: 292 random unit rows in tracks of 1, 2, 5, 40, 64, 100, 40 and 40 rows; the last two tracks hold identical rows; one
row of the 100-row track is NaN.  Slots per task: 1, 3, 400 (the default 20 x 20 window), 8192 with k = 32, 8192 with k = 1."""
import functools

import numpy as np
import pytest
import torch

import _identify_ref as R

pytestmark = pytest.mark.gpu
TRACK_LEN = [1, 2, 5, 40, 64, 100, 40, 40]
FIRST = np.concatenate([[0], np.cumsum(TRACK_LEN)]).astype(np.int32)
N = int(FIRST[-1])
NAN_ROW = int(FIRST[5]) + 50
OUT = ('track', 'align', 'score', 'votes', 'overlap')


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).cuda()


def _unit(rng, n, d):
    x = rng.normal(size=(n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _index(d):
    x = _unit(np.random.default_rng(100 + d), N, d)
    x[FIRST[7]:FIRST[8]] = x[FIRST[6]:FIRST[7]]                     # two tracks of identical rows
    clean = x.copy()
    x[NAN_ROW] = np.nan
    return x, clean


def _raw(nafp, q, x, topk, q0, ln, max_len, first, min_overlap, min_votes, n_short, n_out, with_n_cand=True, n_index=N):
    """The C entry point itself (device tensors in, dict of numpy out); the outputs start from sentinels."""
    L = nafp._lib
    lib = L.load()
    T = len(q0)
    o = {n: torch.full((T, n_out), -7, dtype=torch.int32, device='cuda') for n in OUT if n != 'score'}
    o['score'] = torch.full((T, n_out), 123.0, dtype=torch.float32, device='cuda')
    nc = torch.full((T,), -7, dtype=torch.int32, device='cuda')
    assert lib.nafp_search_identify_check_tracks_host(first.ctypes.data, len(first) - 1, n_index) == 0
    fd = _dev(first)
    L.check(lib.nafp_search_identify(L.ptr(q), q.shape[0], L.ptr(x), n_index, q.shape[1], L.ptr(topk), topk.shape[1], L.ptr(q0), L.ptr(ln),
                                     T, int(max_len), L.ptr(fd), len(first) - 1, min_overlap, min_votes, n_short, n_out, L.ptr(o['track']),
                                     L.ptr(o['align']), L.ptr(o['score']), L.ptr(o['votes']), L.ptr(o['overlap']),
                                     L.ptr(nc) if with_n_cand else None, L.current_stream()), 'search_identify')
    torch.cuda.synchronize()
    out = {n: t.cpu().numpy() for n, t in o.items()}
    out['n_cand'] = nc.cpu().numpy()
    return out


def _yardstick(nafp, q, x):
    """score_fn of the restatement: nafp_search_seq_scores on the sub-range, one task per candidate."""
    L = nafp._lib
    lib = L.load()

    def fn(q_start, n_ov, cand):
        n = len(cand)
        out = torch.empty((n, 1), dtype=torch.float32, device='cuda')
        tq, tl, tc = _dev(q_start, np.int32), _dev(n_ov, np.int32), _dev(np.asarray(cand)[:, None], np.int32)      # held until the launch is done
        L.check(lib.nafp_search_seq_scores(L.ptr(q), L.ptr(x), N, q.shape[1], L.ptr(tq), L.ptr(tl), n, L.ptr(tc), 1, L.ptr(out),
                                           L.current_stream()), 'search_seq_scores')
        torch.cuda.synchronize()
        return out.cpu().numpy()[:, 0]
    return fn


def _same_bytes(a, b):
    return all(a[n].dtype == b[n].dtype and a[n].shape == b[n].shape and a[n].tobytes() == b[n].tobytes() for n in OUT + ('n_cand',))


def _check(nafp, d, query, topk, q0, ln, max_len, params, alone=()):
    """One launch against the restatement, the yardstick's bits, the float64 bound, itself again and chosen tasks alone."""
    x, clean = _index(d)
    qd, xd, td, q0d, lnd = _dev(query), _dev(x), _dev(topk, np.int32), _dev(q0, np.int32), _dev(ln, np.int32)
    mo, mv, ns, no = params
    got = _raw(nafp, qd, xd, td, q0d, lnd, max_len, FIRST, mo, mv, ns, no)
    want = R.identify(topk, q0, ln, max_len, len(query), N, FIRST, _yardstick(nafp, qd, xd), mo, mv, ns, no)
    for n in ('track', 'align', 'votes', 'overlap', 'n_cand'):
        assert np.array_equal(got[n], want[n]), (n, np.argwhere(got[n] != want[n])[:5])
    assert got['score'].tobytes() == want['score'].tobytes()       # the bits of nafp_search_seq_scores on the sub-range
    q64 = np.asarray(query, np.float64)
    worst = 0.0
    for t, r in np.argwhere(got['track'] >= 0):
        tr, a, n_ov = int(got['track'][t, r]), int(got['align'][t, r]), int(got['overlap'][t, r])
        i0 = max(0, int(FIRST[tr]) - a)
        assert n_ov == min(R.effective_len(q0[t], ln[t], max_len, len(query)), int(FIRST[tr + 1]) - a) - i0 >= 1
        exact = (q64[q0[t] + i0:q0[t] + i0 + n_ov] * x[a + i0:a + i0 + n_ov].astype(np.float64)).sum() / n_ov
        err, bound = abs(float(got['score'][t, r]) - exact), (d + n_ov + 2) * 2.0 ** -24
        worst = max(worst, err / bound)
        assert err <= bound, (t, r, err, bound)
    print(f'd {d}, {topk.shape[1]} x {max_len} slots, {params}: largest |score - float64 mean| / bound = {worst:.3f}')
    assert _same_bytes(got, _raw(nafp, qd, xd, td, q0d, lnd, max_len, FIRST, mo, mv, ns, no))       # run to run
    for t in alone:                                                  # a task does not depend on what else is in the launch
        one = _raw(nafp, qd, xd, td, q0d[t:t + 1].clone(), lnd[t:t + 1].clone(), max_len, FIRST, mo, mv, ns, no)
        assert _same_bytes(one, {n: got[n][t:t + 1] for n in OUT + ('n_cand',)}), t
    return got, want


def _plant(topk, query, clean, q0, a, segs, col=0, noise=None):
    """The recording's segments `segs` of the task at q0 are the index rows a + i: the search finds them (column `col`)."""
    for i in segs:
        row = topk[q0 + i]
        row[row == a + i] = -1                                       # ids inside a row stay distinct
        row[col] = a + i
        if noise is not False:
            query[q0 + i] = clean[a + i] if noise is None else noise(clean[a + i])


@functools.lru_cache(maxsize=None)
def _window_batch(d):
    """50 tasks of 20 segments x k = 20 (400 slots each), task t on the query rows [20 t, 20 t + 20): the hand-built cases first,
    random tasks with planted runs after them.  Every row of the random background holds -1 and ids >= n_index (holes)."""
    rng = np.random.default_rng(d)
    x, clean = _index(d)
    T, W, k = 50, 20, 20
    nq = T * W
    query = _unit(rng, nq, d)
    topk = np.stack([rng.permutation(N + 4)[:k] - 2 for _ in range(nq)]).astype(np.int32)      # distinct ids in -2 .. N + 1 per row
    q0 = (np.arange(T) * W).astype(np.int32)
    ln = np.full(T, W, np.int32)
    f = [int(v) for v in FIRST]
    for t in (0, 1, 2, 3, 4, 6):                                     # the hand-built tasks hold nothing but holes and what is planted
        topk[q0[t]:q0[t] + W] = np.where(np.arange(k) % 2 == 0, -1, N + np.arange(k) % 3)[None, :]
    _plant(topk, query, clean, q0[0], -2, range(5, 10))              # 0: a < 0 -- the recording starts before track 2 (rows 3 .. 7)
    _plant(topk, query, clean, q0[1], f[4] - 6, range(6, 20))        # 1: a before its track's first row (track 4)
    _plant(topk, query, clean, q0[2], f[4] - 8, range(0, 8))         # 2: the window runs past the end of track 3
    _plant(topk, query, clean, q0[3], f[4] - 3, range(0, 8))         # 3: one a through two tracks: rows 45 .. 47 of track 3, 48 .. of track 4
    _plant(topk, query, clean, q0[4], f[6] + 5, range(0, 20), col=0)  # 4: both copies of the identical rows found: scores tie exactly
    _plant(topk, query, clean, q0[4], f[7] + 5, range(0, 20), col=1, noise=False)
    _plant(topk, query, clean, q0[5], NAN_ROW - 10, range(0, 20), noise=False)      # 5: an alignment over the NaN row: the most votes, no score
    topk[q0[6] + 4, 0] = 0                                           # 6: one vote for the 1-row track, nothing else
    ln[7] = 0                                                        # 7: empty
    q0[8] = nq                                                       # 8, 9: q0 outside [0, n_query)
    q0[9] = -3
    q0[10], ln[10] = nq - 5, W                                       # 10: the rows run past n_query: 5 segments
    ln[11] = W + 7                                                   # 11: clipped by max_len
    for t in range(12, T):                                           # planted runs of 2 .. 20 segments at any alignment, -19 .. N - 1
        a = int(rng.integers(-W + 1, N)) if t != 30 else f[5] + 10
        segs = [i for i in rng.permutation(W)[:int(rng.integers(2, W + 1)) if t != 30 else 12] if 0 <= a + i < N and a + i != NAN_ROW]
        jitter = lambda v: (lambda w: (w / np.linalg.norm(w)).astype(np.float32))(v.astype(np.float64) + 0.02 * rng.normal(size=d))
        for i in segs:
            col = int(rng.integers(0, k))
            row = topk[q0[t] + i]
            row[row == a + i] = -1                                   # ids inside a row stay distinct
            row[col] = a + i
            query[q0[t] + i] = jitter(clean[a + i])
    return query, topk, q0, ln


PARAMS = [(1, 1, 32, 8), (2, 1, 32, 8), (1, 2, 8, 4), (4, 2, 32, 1), (1, 1, 256, 32)]


@pytest.mark.parametrize('d', [64, 128, 256])
def test_windows_of_400_slots(nafp, d):
    query, topk, q0, ln = _window_batch(d)
    assert (topk == -1).any() and (topk >= N).any()
    f = [int(v) for v in FIRST]
    res = {p: _check(nafp, d, query, topk, q0, ln, 20, p, alone=(0, 2, 3, 4, 7, 8, 10, 30) if p == PARAMS[0] else (3, 12)) for p in PARAMS}
    got, want = res[PARAMS[0]]                                       # min_overlap 1, min_votes 1: every pair is a candidate
    top = lambda t: (int(got['track'][t, 0]), int(got['align'][t, 0]), int(got['votes'][t, 0]), int(got['overlap'][t, 0]))
    assert top(0) == (2, -2, 5, 5)                                   # a < 0
    assert top(1) == (4, f[4] - 6, 14, 14)                           # a before the track
    assert top(2) == (3, f[4] - 8, 8, 8) and got['score'][2, 0] > 0.999      # only the overlap is scored: 8 rows of track 3
    rows = {(int(r[0]), int(r[1])): r for r in want['scored'][3][0]}
    assert (3, f[4] - 3) in rows and (4, f[4] - 3) in rows           # the same a through two tracks: two candidates
    assert rows[(3, f[4] - 3)][2:].tolist() == [3, 0, 3] and rows[(4, f[4] - 3)][2:].tolist() == [5, 3, 17]
    assert got['track'][4, :2].tolist() == [6, 7] and got['score'][4, 0] == got['score'][4, 1]      # exactly equal scores: the track decides
    assert got['align'][4, :2].tolist() == [f[6] + 5, f[7] + 5]
    rows5, sc5 = want['scored'][5]
    assert rows5[0].tolist()[:3] == [5, NAN_ROW - 10, 20] and np.isnan(sc5[0])     # the NaN row: first of the shortlist, dropped from the ranking
    assert not ((got['track'][5] == 5) & (got['align'][5] == NAN_ROW - 10)).any()
    assert top(6) == (0, -4, 1, 1) and got['n_cand'][6] == 1 and got['track'][6, 1] == -1
    for t in (7, 8, 9):                                              # no candidates: all padding
        assert got['n_cand'][t] == 0 and (got['track'][t] == -1).all() and (got['align'][t] == 0).all()
        assert (got['score'][t] == -np.inf).all() and (got['votes'][t] == 0).all() and (got['overlap'][t] == 0).all()
    assert got['overlap'][10].max() <= 5 and got['n_cand'][10] > 0
    # the shortlist cut falls inside a vote tie (singletons on both sides), broken by track then alignment
    full = {t: R.shortlist(topk, int(q0[t]), 20, N, FIRST, 1, 1, 10 ** 6) for t in range(12, 50)}
    assert all(got['n_cand'][t] == n for t, (_, n) in full.items())
    assert [t for t, (rows, n) in full.items() if n > 32 and rows[31, 2] == rows[32, 2]]
    # min_overlap = 2 drops the 1-row overlap of task 6; min_votes = 2 drops the singletons
    assert res[PARAMS[1]][0]['n_cand'][6] == 0 and res[PARAMS[1]][0]['track'][6, 0] == -1
    g2 = res[PARAMS[2]][0]
    assert g2['n_cand'][6] == 0 and (g2['votes'][g2['track'] >= 0] >= 2).all() and 0 < g2['n_cand'][30] < got['n_cand'][30]
    assert (res[PARAMS[3]][0]['overlap'][res[PARAMS[3]][0]['track'] >= 0] >= 4).all()


@pytest.mark.parametrize('d', [64, 128, 256])
def test_boundary_is_honoured_where_seq_match_crosses_it(nafp, d):
    """Task 2 of the batch: the recording's first 8 segments are the last 8 rows of track 3.  nafp_search_seq_match scores the
    candidate over all 20 segments, into the next track's rows; nafp_search_identify over the 8 rows of the overlap."""
    query, topk, q0, ln = _window_batch(d)
    x, _ = _index(d)
    L = nafp._lib
    qd, xd, td = _dev(query), _dev(x), _dev(topk, np.int32)
    q0d, lnd = _dev(q0[2:3]), _dev(ln[2:3])
    got = _raw(nafp, qd, xd, td, q0d, lnd, 20, FIRST, 1, 1, 32, 1)
    ids = torch.empty((1, 10), dtype=torch.int32, device='cuda')
    sc = torch.empty((1, 10), dtype=torch.float32, device='cuda')
    L.check(L.load().nafp_search_seq_match(L.ptr(qd), qd.shape[0], L.ptr(xd), N, d, L.ptr(td), 20, L.ptr(q0d), L.ptr(lnd), 1, 20,
                                           10, L.ptr(ids), L.ptr(sc), None, L.current_stream()), 'search_seq_match')
    ids, sc = ids.cpu().numpy()[0], sc.cpu().numpy()[0]
    a = int(FIRST[4]) - 8
    assert got['align'][0, 0] == a and got['overlap'][0, 0] == 8 and a in ids.tolist()
    assert sc[ids.tolist().index(a)] != got['score'][0, 0] and sc[ids.tolist().index(a)] < 0.9 < got['score'][0, 0]


@pytest.mark.parametrize('d', [64, 128, 256])
@pytest.mark.parametrize('k,length', [(1, 1), (3, 1), (1, 3)])
def test_smallest_windows(nafp, d, k, length):
    rng = np.random.default_rng(7 * d + 3 * k + length)
    x, clean = _index(d)
    T = 12
    nq = T * length
    query = _unit(rng, nq, d)
    topk = np.stack([rng.permutation(N + 2)[:k] - 1 for _ in range(nq)]).astype(np.int32)
    best = int(FIRST[6]) - 1                                          # the last row of track 5, found for segment 0 of task 0
    topk[0][topk[0] == best] = -1
    topk[0, 0], topk[nq - 1, 0] = best, 0
    query[0] = clean[best]
    q0 = (np.arange(T) * length).astype(np.int32)
    ln = np.full(T, length, np.int32)
    got, _ = _check(nafp, d, query, topk, q0, ln, length, (1, 1, 4, 3), alone=(0, T - 1))
    assert (got['track'][0, 0], got['align'][0, 0], got['votes'][0, 0], got['overlap'][0, 0]) == (5, best, 1, 1)
    _check(nafp, d, query, topk, q0, ln, length, (4, 1, 1, 1))       # min_overlap above the window: min(min_overlap, len) applies


@pytest.mark.parametrize('d', [64, 128, 256])
@pytest.mark.parametrize('k,length', [(32, 256), (1, 8192)])
def test_8192_slots(nafp, d, k, length):
    """The largest task: 96 KB of LDS.  k = 32: far more than 256 distinct candidates, with votes above 1 from chance alone;
    k = 1: one id per segment of an 8192-segment window."""
    rng = np.random.default_rng(11 * d + k)
    x, clean = _index(d)
    nq = length + length // 2
    query = _unit(rng, nq, d)
    topk = np.stack([rng.permutation(N + 4)[:k] - 2 for _ in range(nq)]).astype(np.int32)
    q0 = np.array([0, length // 2, nq - 3], np.int32)                # the second task is clipped by max_len, the third by n_query to 3
    ln = np.array([length, length + 9, length], np.int32)
    a = int(FIRST[4]) - 100                                          # a < 0: the 64 rows of track 4 are segments 100 .. 163 of task 0
    for i in range(100, 164):
        row = topk[i]
        row[row == a + i] = -1
        row[0] = a + i
        query[i] = clean[a + i]
    got, want = _check(nafp, d, query, topk, q0, ln, length, (4, 2, 256, 32), alone=(0, 2))
    assert (got['track'][0, 0], got['align'][0, 0], got['overlap'][0, 0]) == (4, a, 64) and got['votes'][0, 0] == 64
    got1, _ = _check(nafp, d, query, topk, q0, ln, length, (1, 1, 16, 16))
    assert got1['n_cand'][0] > 256 and got1['n_cand'][0] >= got['n_cand'][0]      # more distinct candidates than one compaction pass of 256 slots holds
