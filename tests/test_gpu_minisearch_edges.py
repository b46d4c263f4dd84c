"""GPU: nafp_minisearch_scores / nafp_minisearch_ranks at their edges, through the C entry points: dims that are no multiple of the
32-wide k-step, query / db counts that are no multiple of the 32 x 32 tile together with such a dim, one query against one row, the
tie rule of both modes, one single target (scope == n_query) and the largest admitted gt_id_offset (n_db - n_query).

LATTICE data: every entry is a multiple of 1/8 in [-1/4, 1/4].  Products and squares are multiples of 1/64 and every sum of at most
1024 of them (and every diagonal sum of at most 140 scores) is an integer multiple of 1/64 far below 2^24 / 64, so float32 is exact
in any order: the scores EQUAL the float64 oracle's and equal diagonal sums are equal in the kernel as well.  The db rows repeat
with a period, which puts candidates with the ground truth's own sum on BOTH sides of it: 'argmin' ranks the smaller id first,
'argmax' (the stable order reversed as a whole) the larger."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import minisearch as M

pytestmark = pytest.mark.gpu

MODES = {0: 'argmin', 1: 'argmax'}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _data(nQ, nD, d, off, seed):
    """db: rows of a pool, repeated with period P (row i == row i + P); query t: db row t + off, a third of them untouched, the
    rest with lattice noise on an eighth of the entries or replaced by a fresh row (the ground truth is found, nearly found, or lost)."""
    rng = np.random.default_rng(seed)
    P = max(1, nD // 3)
    db = (rng.integers(-2, 3, size=(P, d)) / 8.0)[np.arange(nD) % P]
    q = db[off:off + nQ].copy()
    for t in range(nQ):
        n_noisy = [0, max(1, d // 8), d][rng.integers(0, 3)]
        where = rng.permutation(d)[:n_noisy]
        q[t, where] = np.clip(q[t, where] * 8 + rng.integers(-2, 3, size=n_noisy), -2, 2) / 8.0 if n_noisy < d else rng.integers(-2, 3, size=d) / 8.0
    return q.astype(np.float32), db.astype(np.float32)


@pytest.mark.parametrize('nQ,nD', [(1, 1), (31, 33), (65, 97), (140, 150)])
@pytest.mark.parametrize('d', [1, 33, 100, 1024])
def test_scores_and_ranks_are_exact(nafp, d, nQ, nD):
    lib = nafp._lib.load()
    seen_before = seen_after = 0
    for off in sorted({0, nD - nQ}):                               # n_t - 1 + off <= n_db - scope  <=>  off <= n_db - n_query, whatever the scope
        q, db = _data(nQ, nD, d, off, 1000 * d + nQ + off)
        tq, tdb = torch.from_numpy(q).cuda(), torch.from_numpy(db).cuda()
        for mode in (0, 1):
            want = M.pairwise(q, db, MODES[mode])
            scores = torch.full((nQ, nD), float('nan'), device='cuda')
            assert lib.nafp_minisearch_scores(_ptr(tq), _ptr(tdb), nQ, nD, d, mode, _ptr(scores), _stream()) == 0
            assert np.array_equal(scores.cpu().numpy(), want)
            for s in sorted({1, min(2, nQ), nQ}):
                n_t = nQ - s + 1
                rank = torch.full((n_t + 8,), -7, dtype=torch.int32, device='cuda')
                assert lib.nafp_minisearch_ranks(_ptr(scores), nQ, nD, s, mode, off, _ptr(rank), _stream()) == 0
                got = rank.cpu().numpy()
                want_rank = M.ranks(want, s, MODES[mode], off)
                assert np.array_equal(got[:n_t], want_rank) and (got[n_t:] == -7).all(), (off, mode, s)
                # the planted ties are there: candidates with the ground truth's own sum before and after it
                conv = M.conv_eye(want, s)
                for t in range(n_t):
                    same = np.flatnonzero(conv[t] == conv[t, t + off])
                    seen_before += (same < t + off).any()
                    seen_after += (same > t + off).any()
    if nD >= 33:
        assert seen_before > 0 and seen_after > 0
