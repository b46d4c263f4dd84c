"""CPU: the host side of the HNSW index (neural-audio-fp_amd/eval/hnsw.py: level draws, round bounds, static bound), the argument
checks of the nafp_hnsw_* entry points (include/nafp.h "HNSW"; no GPU call is reached), and the float64 restatement's own
invariants (tests/_hnsw_ref.py)."""
import ctypes

import numpy as np
import pytest

import _hnsw_ref as R


@pytest.fixture(scope='module')
def H(nafp):
    from neural_audio_fp_amd.eval import hnsw
    return hnsw


@pytest.mark.parametrize('n', [0, 1, 2, 9, 1000])
def test_levels_and_rounds_equal_the_restatement(H, n):
    assert np.array_equal(H.draw_levels(1234, 0, n), R.draw_levels(1234, 0, n))
    assert H.draw_levels(1234, 0, n).dtype == np.int32
    assert H.round_bounds(0, n) == R.round_bounds(0, n)
    b = H.round_bounds(0, n)
    assert [s for s, _ in b] == [0] + [e for _, e in b[:-1]] if n else b == []
    assert all(e - s == min(max(1, s // 8), 16384, n - s) for s, e in b)


def test_a_straddling_second_add_and_the_cap(H):
    # a row's level depends on its id only
    whole = H.draw_levels(7, 0, 1000)
    assert np.array_equal(np.concatenate([H.draw_levels(7, 0, 333), H.draw_levels(7, 333, 1000)]), whole)
    assert not np.array_equal(whole, H.draw_levels(8, 0, 1000))
    # rounds continue from the inserted count: a build at 333 rows, then at 1000
    assert H.round_bounds(333, 1000) == R.round_bounds(333, 1000)
    assert H.round_bounds(333, 1000)[0] == (333, 333 + 41)
    assert H.round_bounds(0, 333) + H.round_bounds(333, 1000) != H.round_bounds(0, 1000)
    # the cap (bounds only)
    b = H.round_bounds(0, 200000)
    assert b == R.round_bounds(0, 200000) and b[-1][1] == 200000
    assert max(e - s for s, e in b) == 16384
    first_capped = next(s for s, e in b if e - s == 16384)
    assert first_capped >= 8 * 16384 and all(e - s == 16384 for s, e in b if s >= first_capped and e < 200000)
    assert H.default_max_expansions(1) == 260 and H.default_max_expansions(128) == 768 == R.default_max_expansions(128)


def test_level_frequencies(H):
    n = 100000
    lv = H.draw_levels(1234, 0, n)
    assert lv.min() == 0 and lv.max() <= 7
    for l in range(4):
        p = (1 - 1 / 16) * 16.0 ** -l
        assert abs((lv == l).mean() - p) <= 4 * np.sqrt(p * (1 - p) / n), l
    assert (lv >= 4).sum() <= 16.0 ** -4 * n + 4 * np.sqrt(16.0 ** -4 * n) + 1


def test_argument_checks_without_gpu(nafp):
    lib = nafp._lib.load()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)                    # never dereferenced: every refusal precedes the first GPU call
    assert lib.nafp_hnsw_default_max_expansions(16) == 320 and lib.nafp_hnsw_default_max_expansions(129) == -1
    assert lib.nafp_hnsw_reverse_workspace_bytes(1000, 100, 16, 0) > 1000 * 8 + 100 * 32 * 24
    assert lib.nafp_hnsw_reverse_workspace_bytes(1000, 100, 16, 1) < lib.nafp_hnsw_reverse_workspace_bytes(1000, 100, 16, 0)
    assert lib.nafp_hnsw_reverse_workspace_bytes(1000, 100, 8, 0) == -1 and lib.nafp_hnsw_reverse_workspace_bytes(-1, 100, 16, 0) == -1
    assert lib.nafp_hnsw_reverse_workspace_bytes(1000, 100, 16, 8) == -1
    assert lib.nafp_hnsw_search_workspace_bytes(10, 16, 20) >= 80
    assert lib.nafp_hnsw_search_workspace_bytes(10, 129, 20) == -1 and lib.nafp_hnsw_search_workspace_bytes(10, 16, 33) == -1
    assert lib.nafp_hnsw_search_workspace_bytes(-1, 16, 20) == -1

    def layer(x=p, dim=128, M=16, level=0, ef=16, nq=0):
        return lib.nafp_hnsw_search_layer(x, 10, dim, p, None, 10, 32, M, level, p, nq, p, None, ef, 100, 1, p, p, None)
    assert layer(x=None) == 1 and layer(nq=-1) == 1
    assert layer(dim=100) == 2 and layer(M=8) == 2 and layer(level=8) == 2 and layer(ef=129) == 2
    assert layer() == 0                                        # no query: nothing launched
    # entries inside the output: refused (a block's results would overwrite entries that other blocks have not read yet)
    ids = np.zeros(64, np.int32)
    pi = lambda off: ctypes.c_void_p(ids.ctypes.data + 4 * off)
    overlap = lambda ent, out: lib.nafp_hnsw_search_layer(p, 10, 128, p, None, 10, 32, 16, 0, p, 4, ent, None, 8, 100, 8, p, out, None)
    assert overlap(pi(0), pi(0)) == 1 and overlap(pi(31), pi(0)) == 1 and overlap(pi(0), pi(3)) == 1

    def select(x=p, dim=128, M=16, level=0, ef=16, n_new=0):
        return lib.nafp_hnsw_select_forward(x, 10, dim, 5, n_new, p, level, M, p, p, ef, p, None, 10, 32, None)
    assert select(x=None) == 1 and select(n_new=-1) == 1 and select(n_new=6) == 1
    assert select(dim=32) == 2 and select(M=32) == 2 and select(level=8) == 2 and select(ef=200) == 2
    assert select() == 0

    def reverse(x=p, dim=128, M=16, level=0, n_new=0):
        return lib.nafp_hnsw_reverse_links(x, 10, dim, 5, n_new, p, level, M, p, None, 10, 32, None, 0, None)
    assert reverse(x=None) == 1 and reverse(n_new=-1) == 1
    assert reverse(dim=512) == 2 and reverse(M=15) == 2 and reverse(level=9) == 2
    assert reverse() == 0
    assert reverse(n_new=5) == 1                               # rows to link back, and no workspace

    def search(x=p, dim=128, M=16, L=0, ef=16, k=20, nq=0, entry=0):
        return lib.nafp_hnsw_search(x, 10, dim, p, p, p, 4, M, entry, L, p, nq, ef, k, p, p, None, 0, None)
    assert search(x=None) == 1 and search(nq=-1) == 1 and search(entry=10) == 1
    assert search(dim=96) == 2 and search(M=4) == 2 and search(L=8) == 2 and search(ef=129) == 2 and search(k=33) == 2
    assert search() == 0
    assert search(nq=3) == 1                                   # queries, and no workspace


@pytest.fixture(scope='module')
def lattice_graph():
    x = R.lattice(400, 64, 11)
    return x, R.build(x, 1234, ef_construction=20)


def test_restatement_invariants(lattice_graph):
    x, g = lattice_graph
    assert g.n == 400 and g.history == R.round_bounds(0, 400)
    R.check_invariants(g.levels, lambda l: (g.level_rows(l), g.links[l][g.level_rows(l)]), g.n)
    xd = x.astype(np.float64)
    for level in range(R.MAX_LEVEL + 1):
        for r in g.level_rows(level):
            ids = [t for t in g.links[level][r] if t >= 0]
            keys = [(((xd[t] - xd[r]) ** 2).sum(), t) for t in ids]
            assert keys == sorted(keys), (level, r)
        below = np.nonzero(g.levels < level)[0]
        assert (g.links[level][below] == -1).all()
    assert g.entry == (int(np.argmax(g.levels)), int(g.levels.max()))
    assert (g.links[0] >= 0).sum(1).min() >= 1                 # every row is linked on level 0


def test_restatement_search_is_exhaustive_when_ef_covers_the_graph():
    x = R.lattice(30, 64, 5, n_dup=2)
    g = R.build(x, 99, ef_construction=40)
    q = R.lattice(7, 64, 6, n_dup=0)
    D, I = g.search(q, 30, ef_search=64)
    d = ((q[:, None, :].astype(np.float64) - x[None].astype(np.float64)) ** 2).sum(-1)
    for r in range(len(q)):
        order = np.lexsort((np.arange(30), d[r]))
        assert np.array_equal(I[r], order) and np.array_equal(D[r], d[r][order])
    # fewer rows than k: padding
    D, I = g.search(q[:2], 32, ef_search=16)
    assert (I[:, 30:] == -1).all() and np.isinf(D[:, 30:]).all() and (I[:, :30] >= 0).all()


def test_select_and_search_layer_small_cases():
    x = np.array([[0, 0], [1, 0], [2, 0], [0, 3], [1, 0]], np.float64)
    # owner 0: candidates 1, 4 (duplicate row of 1), 2, 3 in order.  4 is at distance 0 of 1 < 1: pruned; 2 is nearer to 1 than to 0
    cands = sorted([(((x[c] - x[0]) ** 2).sum(), c) for c in (1, 2, 3, 4, 0, 1)])
    assert R.select(x, 0, cands, 2) == [1, 3]
    assert R.select(x, 0, cands, 1) == [1]
    links = np.array([[1, -1], [0, 2], [1, 3], [2, -1], [-1, -1]])
    q = np.array([2.2, 0.0])
    assert [i for _, i in R.search_layer(x, links, q, 0, 1)] == [2]
    assert [i for _, i in R.search_layer(x, links, q, 0, 3)] == [2, 1, 0]
    assert [i for _, i in R.search_layer(x, links, q, 0, 3, max_expansions=1)] == [1, 0]
    assert [i for _, i in R.search_layer(x, links, q, 4, 3)] == [4]          # an isolated entry
    assert R.search_layer(x, links, q, -1, 3) == []
