"""GPU: nafp_search_identify_tempo (csrc/search.hip), the matcher along slanted lines, against its numpy restatement
(tests/_identify_tempo_ref.py) and against nafp_search_identify.  Track, rho, alignment, votes, overlap and n_cand are EQUAL to the
restatement; every score has the bits nafp_search_seq_scores gives on the rows index[a + off_r(i)] gathered into an array of their
own (the yardstick of tests/test_gpu_identify.py: the restatement ranks by those bits); a task alone gives the bytes it gives inside
a launch, and two runs give the same bytes.  With the single hypothesis 65536 every array is nafp_search_identify's, byte for byte.

The index is that of tests/test_gpu_identify.py: 292 random unit rows in tracks of 1, 2, 5, 40, 64, 100, 40 and 40 rows; the last
two tracks hold identical rows; one row of the 100-row track is NaN.  The command-line part runs `run.py identify --tempos` on a
synthetic library with MODEL.HOP = MODEL.DUR, where a time-stretched recording can be spliced from whole library segments."""
import copy
import functools
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch
import yaml

import _identify_tempo_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACK_LEN = [1, 2, 5, 40, 64, 100, 40, 40]
FIRST = np.concatenate([[0], np.cumsum(TRACK_LEN)]).astype(np.int32)
N = int(FIRST[-1])
NAN_ROW = int(FIRST[5]) + 50
ONE = 1 << 16
RHO = lambda tempo: int(round(ONE * tempo))
FIVE = [ONE, RHO(0.93), RHO(1.07), RHO(0.8), RHO(1.25)]            # as `--tempos` would hand them over: nearest 1 first
OUT = ('track', 'align', 'score', 'votes', 'overlap')
OUT_T = OUT + ('rho', 'n_cand')


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


def _outputs(T, n_out, names):
    o = {n: torch.full((T, n_out), -7, dtype=torch.int32, device='cuda') for n in names if n not in ('score', 'n_cand')}
    o['score'] = torch.full((T, n_out), 123.0, dtype=torch.float32, device='cuda')
    o['n_cand'] = torch.full((T,), -7, dtype=torch.int32, device='cuda')
    return o


def _raw_plain(nafp, q, x, topk, q0, ln, max_len, params):
    """nafp_search_identify itself (device tensors in, dict of numpy out); the outputs start from sentinels."""
    L = nafp._lib
    mo, mv, ns, no = params
    o = _outputs(len(q0), no, OUT)
    fd = _dev(FIRST)
    L.check(L.load().nafp_search_identify(L.ptr(q), q.shape[0], L.ptr(x), N, q.shape[1], L.ptr(topk), topk.shape[1], L.ptr(q0), L.ptr(ln),
                                          len(q0), int(max_len), L.ptr(fd), len(FIRST) - 1, mo, mv, ns, no, L.ptr(o['track']), L.ptr(o['align']),
                                          L.ptr(o['score']), L.ptr(o['votes']), L.ptr(o['overlap']), L.ptr(o['n_cand']), L.current_stream()),
            'search_identify')
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in o.items()}


def _raw(nafp, q, x, topk, q0, ln, max_len, rhos, params, first=FIRST, n_index=N):
    """nafp_search_identify_tempo itself (device tensors in, dict of numpy out); the outputs start from sentinels."""
    L = nafp._lib
    mo, mv, ns, no = params
    o = _outputs(len(q0), no, OUT_T)
    fd, rho = _dev(first), np.asarray(rhos, np.int32)
    L.check(L.load().nafp_search_identify_tempo(L.ptr(q), q.shape[0], L.ptr(x), n_index, q.shape[1], L.ptr(topk), topk.shape[1], L.ptr(q0),
                                                L.ptr(ln), len(q0), int(max_len), L.ptr(fd), len(first) - 1, rho.ctypes.data, len(rho), mo, mv,
                                                ns, no, L.ptr(o['track']), L.ptr(o['align']), L.ptr(o['score']), L.ptr(o['votes']),
                                                L.ptr(o['overlap']), L.ptr(o['n_cand']), L.ptr(o['rho']), L.current_stream()),
            'search_identify_tempo')
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in o.items()}


def _yardstick(nafp, q, x):
    """score_fn of the restatement: the candidates' rows index[a + off_r(i)] gathered end to end into an array of their own, and
    nafp_search_seq_scores on it, one task per candidate."""
    L = nafp._lib

    def fn(q_start, n_ov, rows):
        n = len(rows)
        at = np.concatenate([[0], np.cumsum(n_ov)]).astype(np.int64)
        g = x[torch.from_numpy(np.concatenate(rows).astype(np.int64)).cuda()].contiguous()
        out = torch.empty((n, 1), dtype=torch.float32, device='cuda')
        tq, tl, tc = _dev(q_start, np.int32), _dev(n_ov, np.int32), _dev(at[:-1, None], np.int32)      # held until the launch is done
        L.check(L.load().nafp_search_seq_scores(L.ptr(q), L.ptr(g), g.shape[0], q.shape[1], L.ptr(tq), L.ptr(tl), n, L.ptr(tc), 1, L.ptr(out),
                                                L.current_stream()), 'search_seq_scores')
        torch.cuda.synchronize()
        return out.cpu().numpy()[:, 0]
    return fn


def _same_bytes(a, b, names=OUT_T):
    return all(a[n].dtype == b[n].dtype and a[n].shape == b[n].shape and a[n].tobytes() == b[n].tobytes() for n in names)


def _check(nafp, d, query, topk, q0, ln, max_len, rhos, params, alone=()):
    """One launch against the restatement, the yardstick's bits, itself again and chosen tasks alone.  Every row a result was scored
    over lies inside its track."""
    x, _ = _index(d)
    qd, xd, td, q0d, lnd = _dev(query), _dev(x), _dev(topk, np.int32), _dev(q0, np.int32), _dev(ln, np.int32)
    mo, mv, ns, no = params
    got = _raw(nafp, qd, xd, td, q0d, lnd, max_len, rhos, params)
    want = R.identify(topk, q0, ln, max_len, len(query), N, FIRST, rhos, _yardstick(nafp, qd, xd), mo, mv, ns, no)
    for n in ('track', 'rho', 'align', 'votes', 'overlap', 'n_cand'):
        assert np.array_equal(got[n], want[n]), (n, np.argwhere(got[n] != want[n])[:5])
    assert got['score'].tobytes() == want['score'].tobytes()       # the bits of nafp_search_seq_scores on the gathered rows
    for t, r in np.argwhere(got['track'] >= 0):
        tr, a, rho, n_ov = int(got['track'][t, r]), int(got['align'][t, r]), rhos[int(got['rho'][t, r])], int(got['overlap'][t, r])
        length = R.effective_len(q0[t], ln[t], max_len, len(query))
        i0, i1 = R.overlap(a, rho, length, int(FIRST[tr]), int(FIRST[tr + 1]))
        rows = a + R.off(np.arange(i0, i1), rho)
        assert n_ov == i1 - i0 >= 1 and rows.min() >= FIRST[tr] and rows.max() < FIRST[tr + 1]
    assert _same_bytes(got, _raw(nafp, qd, xd, td, q0d, lnd, max_len, rhos, params))        # run to run
    for t in alone:                                                  # a task does not depend on what else is in the launch
        one = _raw(nafp, qd, xd, td, q0d[t:t + 1].clone(), lnd[t:t + 1].clone(), max_len, rhos, params)
        assert _same_bytes(one, {n: got[n][t:t + 1] for n in OUT_T}), t
    return got, want


# ---- the window batch of tests/test_gpu_identify.py, rebuilt -------------------------------------------------------------------
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
def test_hypothesis_one_alone_gives_the_bytes_of_identify(nafp, d):
    query, topk, q0, ln = _window_batch(d)
    x, _ = _index(d)
    qd, xd, td, q0d, lnd = _dev(query), _dev(x), _dev(topk, np.int32), _dev(q0, np.int32), _dev(ln, np.int32)
    for p in PARAMS:
        plain = _raw_plain(nafp, qd, xd, td, q0d, lnd, 20, p)
        tempo = _raw(nafp, qd, xd, td, q0d, lnd, 20, [ONE], p)
        assert _same_bytes(plain, tempo, OUT + ('n_cand',)), p
        assert np.array_equal(tempo['rho'], np.where(plain['track'] >= 0, 0, -1))
        assert (plain['track'] >= 0).sum() > 20 and (plain['track'] < 0).any()       # results and padding both


# ---- planted lines in a random background --------------------------------------------------------------------------------------
def _line(topk, query, clean, q0, a, rho, segs, col=0):
    """The recording's segments `segs` of the task at q0 are the index rows a + off(i): the search finds them in column `col`."""
    for i in segs:
        row_id = a + int(R.off(i, rho))
        row = topk[q0 + i]
        row[row == row_id] = -1
        row[col] = row_id
        query[q0 + i] = clean[row_id]


@functools.lru_cache(maxsize=None)
def _tempo_batch(d):
    """30 tasks of 20 segments x k = 8 under the five hypotheses (800 slots each): per hypothesis r one line inside the 100-row
    track, one that starts before the 64-row track (a below its first row, also a < 0 for the 40-row track), one that runs off the end
    of the 40-row track, and one through the track of one row; random tasks with planted partial lines after them."""
    rng = np.random.default_rng(1000 + d)
    x, clean = _index(d)
    T, W, k = 30, 20, 8
    nq = T * W
    query = _unit(rng, nq, d)
    topk = np.stack([rng.permutation(N + 4)[:k] - 2 for _ in range(nq)]).astype(np.int32)
    q0 = (np.arange(T) * W).astype(np.int32)
    ln = np.full(T, W, np.int32)
    f = [int(v) for v in FIRST]
    inside = {}
    for r, rho in enumerate(FIVE):
        inside[r] = f[5] + 3 + 2 * r                                 # rows f[5] + 3 .. at most f[5] + 35: clear of the NaN row
        _line(topk, query, clean, q0[4 * r], inside[r], rho, range(W))
        a = f[4] - 7                                                 # the first 6 .. 9 segments fall on the 40-row track before it
        _line(topk, query, clean, q0[4 * r + 1], a, rho, [i for i in range(W) if a + int(R.off(i, rho)) >= f[4]])
        a = f[4] - 9                                                 # the window runs off the end of the 40-row track
        _line(topk, query, clean, q0[4 * r + 2], a, rho, [i for i in range(W) if a + int(R.off(i, rho)) < f[4]])
        a = -int(R.off(6, rho))                                      # a < 0: segment 6 falls on row 0, the track of one row
        _line(topk, query, clean, q0[4 * r + 3], a, rho, [i for i in range(W) if 0 <= a + int(R.off(i, rho)) < f[3]])
    for t in range(20, T):                                           # partial lines at any hypothesis and alignment
        rho = FIVE[int(rng.integers(0, 5))]
        a = int(rng.integers(-W, N))
        segs = [i for i in rng.permutation(W)[:int(rng.integers(2, W + 1))] if 0 <= a + int(R.off(i, rho)) < N and a + int(R.off(i, rho)) != NAN_ROW]
        _line(topk, query, clean, q0[t], a, rho, segs, col=int(rng.integers(0, k)))
    ln[29] = W + 5                                                   # clipped by max_len
    return query, topk, q0, ln, inside


@pytest.mark.parametrize('d', [64, 128, 256])
def test_planted_lines_against_the_restatement(nafp, d):
    query, topk, q0, ln, inside = _tempo_batch(d)
    f = [int(v) for v in FIRST]
    got, want = _check(nafp, d, query, topk, q0, ln, 20, FIVE, (1, 1, 64, 8), alone=(0, 1, 2, 3, 25))
    _check(nafp, d, query, topk, q0, ln, 20, FIVE, (4, 2, 32, 4), alone=(7,))
    for r in range(5):
        # a line inside its track: found under its own hypothesis, over all 20 rows, with the score of equal rows
        t = 4 * r
        assert (got['track'][t, 0], got['rho'][t, 0], got['align'][t, 0], got['overlap'][t, 0]) == (5, r, inside[r], 20) and got['votes'][t, 0] >= 20
        assert got['score'][t, 0] > 0.9999 and got['score'][t, 1] < 0.99
        # the three lines across a boundary are candidates with exactly the rows their track holds (the uncut shortlist)
        rho = FIVE[r]
        cands = lambda task: {(int(c[0]), int(c[1]), int(c[2])): c[4:].tolist() for c in R.shortlist(topk, int(q0[task]), 20, N, FIRST, FIVE, 1, 1, 10 ** 6)[0]}
        n_before = sum(1 for i in range(20) if f[4] - 7 + int(R.off(i, rho)) < f[4])
        assert cands(t + 1)[(4, r, f[4] - 7)] == [n_before, 20 - n_before] and 6 <= n_before <= 9      # a before its track
        n_in = sum(1 for i in range(20) if f[4] - 9 + int(R.off(i, rho)) < f[4])
        assert cands(t + 2)[(3, r, f[4] - 9)] == [0, n_in] and n_in < 20                               # off the track's end
        one_row = [i for i in range(20) if int(R.off(i, rho)) == int(R.off(6, rho))]
        assert cands(t + 3)[(0, r, -int(R.off(6, rho)))] == [one_row[0], len(one_row)] and 6 in one_row  # a < 0, the track of one row
    assert got['n_cand'].max() > 64                                  # more candidates than the shortlist holds


# ---- the shapes at which the kernel takes another path --------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (3, 1, 2), (1, 3, 2), (32, 16, 16), (1, 8192, 1), (1, 512, 16), (20, 20, 9)]
SIXTEEN = sorted({RHO(0.8 + 0.03 * n) for n in range(15)} | {ONE}, key=lambda rho: (abs(rho - ONE), rho))


@pytest.mark.parametrize('d', [64, 128, 256])
@pytest.mark.parametrize('k,length,n_rho', SHAPES)
def test_edge_shapes(nafp, d, k, length, n_rho):
    """1, 6, 6, 8192, 8192, 8192 and 3600 slots (the command line's default window under nine hypotheses); three tasks: a whole
    window with a planted line, one clipped by max_len, one clipped by n_query to 3 segments (1 where the window is shorter)."""
    rng = np.random.default_rng(13 * d + 5 * k + length + n_rho)
    x, clean = _index(d)
    rhos = SIXTEEN[:n_rho]
    assert len(rhos) == n_rho and k * length * n_rho <= 8192
    nq = length + length // 2 + 1
    query = _unit(rng, nq, d)
    topk = np.stack([rng.permutation(N + 4)[:k] - 2 for _ in range(nq)]).astype(np.int32)
    q0 = np.array([0, length // 2, nq - min(3, length)], np.int32)
    ln = np.array([length, length + 9, length], np.int32)
    rho = rhos[-1]                                                   # the hypothesis furthest from 1
    a = int(FIRST[5]) + 40 - int(R.off(length - 1, rho))             # the window's last segment falls on row 40 of the 100-row track, short of the NaN row
    segs = [i for i in range(length) if FIRST[5] <= a + int(R.off(i, rho))]
    _line(topk, query, clean, 0, a, rho, segs)
    params = (1, 1, 4, 3) if k * length * n_rho <= 6 else (4, 2, 256, 32)
    got, _ = _check(nafp, d, query, topk, q0, ln, length, rhos, params, alone=(0, 2))
    if len(segs) >= 4:                                               # (the windows of 1 and 3 segments have no such line)
        assert (got['track'][0, 0], got['align'][0, 0], got['overlap'][0, 0]) == (5, a, len(segs)) and got['score'][0, 0] > 0.9999
        assert np.array_equal(R.off(segs, rhos[got['rho'][0, 0]]), R.off(segs, rho))      # the planted hypothesis, or one with the same rows before it
    if k * length * n_rho == 8192:
        got1, _ = _check(nafp, d, query, topk, q0, ln, length, rhos, (1, 1, 16, 16))
        assert got1['n_cand'][0] > 256                               # more distinct candidates than one compaction pass of 256 slots holds


# ---- two hypotheses that give the same rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [64, 128, 256])
def test_duplicate_hypotheses(nafp, d):
    """Over 20 segments 65536 and 65537 give the same off (19 / 65536 < 1 / 2): every candidate comes twice, with equal votes, overlap
    and score bits, and the one first in the list is ranked first -- whichever of the two values that is.  min_votes = 2 keeps the
    candidates below n_short = 256, so that the shortlist cuts no pair in two."""
    query, topk, q0, ln, _ = _tempo_batch(d)
    assert np.array_equal(R.off(np.arange(20), ONE), R.off(np.arange(20), ONE + 1))
    params = (1, 2, 256, 8)
    got, _ = _check(nafp, d, query, topk, q0, ln, 20, [ONE, ONE + 1], params, alone=(0,))
    swapped, _ = _check(nafp, d, query, topk, q0, ln, 20, [ONE + 1, ONE], params)
    assert _same_bytes(got, swapped)                                 # the place in the list decides, not the value
    assert got['n_cand'].max() <= 256 and (got['n_cand'] % 2 == 0).all() and (got['track'][:, 0] >= 0).sum() >= 10
    for t in range(len(q0)):
        n_res = int((got['track'][t] >= 0).sum())
        assert n_res % 2 == 0 and n_res <= got['n_cand'][t]
        for n in range(0, n_res, 2):
            assert got['rho'][t, n:n + 2].tolist() == [0, 1], (t, n)
            for name in OUT:
                assert got[name][t, n].tobytes() == got[name][t, n + 1].tobytes(), (t, n, name)


# ---- ids at the edges of the index ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [64, 128, 256])
def test_ids_at_the_edges_of_the_index(nafp, d):
    """topk_ids of nothing but 0, n_index - 1 and the two values next to them that the contract defines as absent, -1 and n_index:
    every line through row 0 (a track of one row) and through the last row, under the five hypotheses."""
    rng = np.random.default_rng(17 + d)
    T, W, k = 6, 20, 8
    query = _unit(rng, T * W, d)
    topk = rng.choice(np.array([0, N - 1, -1, N], np.int32), size=(T * W, k))
    topk[W:2 * W] = -1                                               # a task of absent ids only
    topk[2 * W:3 * W] = N
    topk[3 * W:4 * W] = 0
    topk[4 * W:5 * W] = N - 1
    q0 = (np.arange(T) * W).astype(np.int32)
    ln = np.full(T, W, np.int32)
    got, _ = _check(nafp, d, query, topk, q0, ln, W, FIVE, (1, 1, 256, 32), alone=(0, 1, 3, 4))
    _check(nafp, d, query, topk, q0, ln, W, FIVE, (4, 2, 32, 8))
    assert got['n_cand'][1] == got['n_cand'][2] == 0 and (got['track'][1:3] == -1).all() and (got['rho'][1:3] == -1).all()
    assert set(got['track'][3][got['track'][3] >= 0]) == {0} and (got['overlap'][3][got['track'][3] >= 0] >= 1).all()
    assert set(got['track'][4][got['track'][4] >= 0]) == {7} and got['align'][4].max() <= N - 1 and got['n_cand'][4] > 32


# ---- a task alone and inside a large launch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [64, 128, 256])
def test_a_task_inside_a_launch_of_1000(nafp, d):
    query, topk, q0, ln, _ = _tempo_batch(d)
    x, _ = _index(d)
    rng = np.random.default_rng(d)
    order = rng.integers(0, len(q0), size=1000)
    order[[0, 499, 999]] = [4, 13, 25]
    qd, xd, td = _dev(query), _dev(x), _dev(topk, np.int32)
    params = (4, 2, 96, 4)
    big = _raw(nafp, qd, xd, td, _dev(q0[order]), _dev(ln[order]), 20, FIVE[:3], params)
    small = _raw(nafp, qd, xd, td, _dev(q0), _dev(ln), 20, FIVE[:3], params)
    assert _same_bytes(big, {n: small[n][order] for n in OUT_T})     # each of the 1,000 is the task of the 30-task launch
    for at in (0, 499, 999):
        t = int(order[at])
        one = _raw(nafp, qd, xd, td, _dev(q0[t:t + 1]), _dev(ln[t:t + 1]), 20, FIVE[:3], params)
        assert _same_bytes(one, {n: big[n][at:at + 1] for n in OUT_T}), at
    assert (big['track'] >= 0).sum() > 500


# ---- the command line -------------------------------------------------------------------------------------------------------------
FS = 8000


def _wav(path, pcm):
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    with wave.open(str(path), 'w') as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(FS)
        w.writeframes(np.clip(pcm, -32768, 32767).astype('<i2').tobytes())


def _music(rng, n):
    """The generator of tests/test_gpu_identify_cli.py."""
    t = np.arange(n) / 8000.0
    x = rng.integers(-1200, 1200, size=n).astype(np.float64)
    for f in rng.uniform(250, 3800, size=4):
        x += 5000 * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28)) * (0.5 + 0.5 * np.sin(2 * np.pi * rng.uniform(0.2, 2.0) * t))
    return x


def test_identify_tempos_cli(nafp, cfg, tmp_path, monkeypatch):
    """MODEL.HOP = MODEL.DUR = 1 s and FEAT 'melspec_maxnorm': the segments do not overlap and a fingerprint depends on its own second
    of PCM alone, so a recording spliced from the whole library segments a + off(i) has exactly the library's rows a + off(i) for
    fingerprints -- at 1.1 every tenth segment is skipped, at 0.9 every tenth is there twice.  With --window 10 --window_hop 10 each
    window starts where off repeats (off(10 + i) = off(10) + off(i), held below), so under its own hypothesis every window is the
    library's rows exactly and scores 1 to rounding; along a line of slope 1 at most 5 of its 10 rows are the library's, the
    others are different unit rows, and the score is strictly less (Cauchy-Schwarz).  Seen on one MI355X run: 1.0000 for all three
    recordings with --tempos; without it 0.957 for the fast one (reported 2 s off) and 0.964 for the slow one, broken into two matches."""
    from neural_audio_fp_amd.model import generate as g
    rng = np.random.default_rng(2028)
    ds = str(tmp_path / 'dataset') + '/'
    pcm = lambda: np.clip(_music(rng, 30 * FS), -32768, 32767).astype('<i2')
    dummy, db = [pcm() for _ in range(2)], [pcm() for _ in range(3)]
    for i, x in enumerate(dummy):
        _wav(f'{ds}music/test-dummy-db-100k-full/x/{i}.wav', x)
    for i, x in enumerate(db):
        _wav(f'{ds}music/test-query-db-500-30s/db/x/{i}.wav', x)
        _wav(f'{ds}music/test-query-db-500-30s/query/x/{i}.wav', x)
    work = tmp_path / 'work'
    (work / 'config').mkdir(parents=True)
    c = copy.deepcopy(cfg)
    c['DIR'].update({'SOURCE_ROOT_DIR': ds + 'music/', 'BG_ROOT_DIR': ds + 'aug/bg/', 'IR_ROOT_DIR': ds + 'aug/ir/',
                     'OUTPUT_ROOT_DIR': str(work) + '/logs/emb/', 'LOG_ROOT_DIR': str(work) + '/logs/'})
    c['MODEL']['FEAT'] = 'melspec_maxnorm'
    c['MODEL']['HOP'] = c['MODEL']['DUR']
    yaml.safe_dump(c, open(work / 'config' / 'tiny.yaml', 'w'))
    g.save_checkpoint(c['DIR']['LOG_ROOT_DIR'] + 'checkpoint/', 'EXP', 1, nafp.get_fingerprinter(c))
    emb = work / 'logs' / 'emb' / 'EXP' / '1'
    for k in ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS', 'NAFP_INGEST_FLAC'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('NAFP_TRACK_TABLE', '1')
    monkeypatch.chdir(work)
    g.generate_fingerprint(c, 'EXP', 1, None, None, False)
    assert json.load(open(emb / 'db_tracks.json'))['first'] == [0, 30, 60, 90]

    seg = int(c['MODEL']['DUR'] * FS)
    r110, r090 = RHO(1.1), RHO(0.9)
    for rho in (r110, r090):
        assert np.array_equal(R.off(np.arange(10, 20), rho) - R.off(10, rho), R.off(np.arange(10), rho))
    splice = lambda x, a, rho: np.concatenate([x[(a + int(R.off(i, rho))) * seg:(a + int(R.off(i, rho)) + 1) * seg] for i in range(20)])
    rec = str(tmp_path / 'rec') + '/'
    _wav(rec + 'a_fast.wav', splice(db[1], 2, r110))                 # 20 s of track 1 from 2 s at tempo 1.1: its segments 2 .. 23, two skipped
    _wav(rec + 'b_slow.wav', splice(db[2], 7, r090))                 # 20 s of track 2 from 7 s at tempo 0.9: its segments 7 .. 24, two repeated
    _wav(rec + 'c_plain.wav', splice(db[0], 3, ONE))                 # 20 s of track 0 from 3 s as it is

    env = {k: v for k, v in os.environ.items() if not k.startswith('NAFP_INGEST') and k not in ('NAFP_RESAMPLE', 'NAFP_TRACK_TABLE')}
    env['PYTHONPATH'] = ROOT

    def identify(out, *args):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), 'identify', 'EXP', '1', rec, '-c', 'tiny', '-i', 'L2', '--window', '10',
                            '--window_hop', '10', '--output', out, *args], cwd=work, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        print(r.stdout[-2000:])
        by = {}
        for m in json.load(open(out))['matches']:
            by.setdefault(os.path.basename(m['recording']), []).append(m)
        return json.load(open(out)), by, r.stdout

    track = lambda i: f'{ds}music/test-query-db-500-30s/db/x/{i}.wav'
    hop_s = float(c['MODEL']['HOP'])
    res, by, text = identify(str(tmp_path / 'tempos.json'), '--tempos', '0.9,1,1.1')
    assert res['tempos'] == [1.0, r090 / ONE, r110 / ONE] and res['n_short'] == 96 and res['n_windows'] == 6
    (fast,), (slow,), (plain,) = by['a_fast.wav'], by['b_slow.wav'], by['c_plain.wav']
    assert fast['track'] == track(1) and fast['tempo'] == r110 / ONE and abs(fast['track_position_s'] - 2.0) <= hop_s and fast['windows'] == 2
    assert slow['track'] == track(2) and slow['tempo'] == r090 / ONE and abs(slow['track_position_s'] - 7.0) <= hop_s and slow['windows'] == 2
    assert plain['track'] == track(0) and plain['tempo'] == 1.0 and plain['track_position_s'] == 3.0 and plain['windows'] == 2
    for m in (fast, slow, plain):
        assert abs(m['score'] - 1.0) < 1e-5 and m['recording_span_s'] == [0.0, 20.0]
    header = lambda out: next(ln for ln in out.splitlines() if ln.startswith('recording '))
    assert header(text).endswith(' tempo') and 'speed' not in header(text)

    # without --tempos: the old matcher, none of the new keys, and a lower best score for the two stretched recordings
    old, old_by, old_text = identify(str(tmp_path / 'plain.json'))
    assert 'tempos' not in old and old['n_short'] == 32 and 'tempo' not in header(old_text)
    assert all('tempo' not in m for ms in old_by.values() for m in ms)
    for name, m in (('a_fast.wav', fast), ('b_slow.wav', slow)):
        best = max((x['score'] for x in old_by.get(name, [])), default=-np.inf)
        print(f'{name}: best score {best} without --tempos, {m["score"]} with')
        assert best < m['score']
    (same,) = old_by['c_plain.wav']
    assert {k: v for k, v in plain.items() if k != 'tempo'} == same
