"""CPU: nafp_search_seq_match (include/nafp.h) is declared, bound and refuses bad arguments before any GPU call; its numpy
restatement (tests/_seq_match_ref.py) is pinned to the float64 oracle of the evaluation loop (oracle/search.py); and
`search_and_score(device_rank=True)` refuses an index that cannot rank on the device."""
import ctypes

import numpy as np
import pytest

import _seq_match_ref as M
from oracle import search as S

FAKE = ctypes.c_void_p(4096)          # a non-null pointer that is never dereferenced: every check below fails before use


def test_symbol_is_declared_and_bound(nafp):
    import test_abi
    assert 'nafp_search_seq_match' in test_abi._declared()
    assert 'nafp_search_seq_match' in nafp._lib.PROTOTYPES
    assert nafp._lib.load().nafp_search_seq_match is not None


def test_refusals_come_before_any_gpu_call(nafp):
    lib = nafp._lib.load()
    OK, INVALID, UNSUPPORTED = 0, 1, 2

    def call(**kw):
        g = lambda name, dflt: kw.get(name, dflt)
        return lib.nafp_search_seq_match(g('query', FAKE), g('n_query', 100), g('index', FAKE), g('n_index', 1000), g('dim', 128),
                                         g('topk', FAKE), g('k', 20), g('q0', FAKE), g('len', FAKE), g('n_tasks', 5), g('max_len', 19),
                                         g('n_out', 10), g('out_ids', FAKE), g('out_scores', FAKE), g('out_n_cand', FAKE), None)

    for name in ('query', 'index', 'topk', 'q0', 'len', 'out_ids', 'out_scores'):
        assert call(**{name: None}) == INVALID, name
    for name in ('n_query', 'n_index', 'n_tasks'):
        assert call(**{name: -1}) == INVALID, name
    assert call(dim=96) == UNSUPPORTED
    assert call(k=0) == UNSUPPORTED and call(k=33) == UNSUPPORTED
    assert call(max_len=0) == UNSUPPORTED
    assert call(k=32, max_len=65) == UNSUPPORTED and call(k=1, max_len=2049) == UNSUPPORTED      # more than 2048 slots
    assert call(n_out=0) == UNSUPPORTED and call(n_out=33) == UNSUPPORTED
    assert call(n_index=1 << 31) == UNSUPPORTED
    # nothing to do: OK without a launch (there is no GPU here to launch on), with and without the optional output
    assert call(n_tasks=0) == OK and call(n_tasks=0, out_n_cand=None) == OK
    assert call(n_tasks=0, k=32, max_len=64, n_out=32, dim=256) == OK                            # the 2048-slot maximum is accepted


def _lattice_case():
    rng = np.random.default_rng(11)
    d = 64
    dummy = rng.integers(-2, 3, size=(150, d)).astype(np.float32)
    db = rng.integers(-2, 3, size=(90, d)).astype(np.float32)
    db[40:50] = db[20:30]                                  # a repeated passage: distinct candidates tie exactly
    query = db.copy()
    redraw = rng.random(size=db.shape) < 0.15
    query[redraw] = rng.integers(-2, 3, size=int(redraw.sum())).astype(np.float32)
    test_ids = np.array([0, 5, 20, 21, 40, 60, 85, 88, 89])      # the last three are clipped by the end of `query`
    return query, db, dummy, test_ids, (1, 3, 5, 19), 20


def test_restatement_equals_the_oracle_on_lattice_data_with_ties():
    query, db, dummy, test_ids, lens, k = _lattice_case()
    index = np.concatenate([dummy, db])
    want = S.evaluate(query, db, dummy, test_ids, lens, k_probe=k)
    got = M.evaluate_with(query, index, lambda q: S.flat_l2_search(q, index, k)[1], test_ids, lens, k, len(dummy))
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    # the case does what it is for: predictions with exactly equal neighbouring scores, hits and misses both present
    I = S.flat_l2_search(query, index, k)[1]
    _, s, n_cand = M.seq_match(query, index, I, test_ids, np.full(len(test_ids), 5), 5, 10)
    assert (s[:, 1:] == s[:, :-1])[np.isfinite(s[:, 1:])].sum() >= 5
    assert 0 < want[0].sum() < want[0].size and (n_cand > 10).all()


def test_restatement_rules_one_by_one():
    index = np.zeros((12, 64), np.float32)
    index[:, 0] = np.arange(12)
    query = np.zeros((4, 64), np.float32)
    query[:, 0] = 1.0                                                      # score(c) = mean of the ids c .. c + len - 1
    topk = np.array([[3, 3, -1, 50], [4, 0, 11, 7], [5, 5, 5, 5], [2, 9, 13, -7]], np.int32)
    ids, sc, n = M.seq_match(query, index, topk, [0, 0, 2, 4, -1, 1], [3, 1, 5, 2, 2, 0], 3, n_out=4)
    # task 0: rows 0..2 -> {3} | {4-1, 11-1, 7-1} (0-1 < 0 dropped) | {5-2}: candidates 3, 6, 10; 10 is shortened to rows 10, 11
    assert ids[0].tolist() == [10, 6, 3, -1] and sc[0].tolist()[:3] == [10.5, 7.0, 4.0] and np.isneginf(sc[0, 3]) and n[0] == 3
    assert ids[1].tolist() == [3, -1, -1, -1] and n[1] == 1                       # 50 >= n_index and -1: absent
    # task 2: q0 = 2, length min(5, 3, 4 - 2) = 2: {5} | {2-1, 9-1} (13, -7 absent)
    assert ids[2].tolist() == [8, 5, 1, -1] and n[2] == 3
    for t in (3, 4, 5):                                                          # q0 outside the range twice, length 0
        assert (ids[t] == -1).all() and np.isneginf(sc[t]).all() and n[t] == 0
    # equal scores: the smaller id first; NaN and -inf scores are dropped
    index2 = np.zeros((6, 64), np.float32)
    index2[2, 0], index2[4, 0] = np.nan, -np.inf
    ids, sc, n = M.seq_match(query[:1], index2, np.array([[5, 1, 2, 3, 4, 0]], np.int32), [0], [1], 1, n_out=6)
    assert ids[0].tolist() == [0, 1, 3, 5, -1, -1] and n[0] == 4


class _NoMatchIndex:
    """An index object of an older kind: it can search and score, but has no `sequence_match`."""
    d = 64
    device = 'cpu'

    def search_device(self, q, k):
        raise AssertionError('the refusal comes before the search')


def test_device_rank_refuses_an_index_without_sequence_match(nafp):
    from neural_audio_fp_amd.eval import eval_faiss as E
    query = np.zeros((30, 64), np.float32)
    assert not E.seq_match_supported(_NoMatchIndex(), 20, 19)
    with pytest.raises(NotImplementedError):
        E.search_and_score(_NoMatchIndex(), query, np.arange(5), (1, 3), 20, 0, device_rank=True)

    class WithMatch(_NoMatchIndex):
        def sequence_match(self, *a, **kw):
            raise AssertionError('not called')
    assert E.seq_match_supported(WithMatch(), 20, 19) and E.seq_match_supported(WithMatch(), 32, 64)
    assert not E.seq_match_supported(WithMatch(), 20, 103) and not E.seq_match_supported(WithMatch(), 33, 1)
    assert not E.seq_match_supported(WithMatch(), 0, 5)
    with pytest.raises(NotImplementedError):
        E.search_and_score(WithMatch(), query, np.arange(5), (1, 70), 32, 0, device_rank=True)


def test_the_switch_reads_the_environment(nafp, monkeypatch):
    from neural_audio_fp_amd.eval import eval_faiss as E
    monkeypatch.delenv('NAFP_SEQ_MATCH', raising=False)
    assert not E.seq_match_enabled()
    monkeypatch.setenv('NAFP_SEQ_MATCH', '0')
    assert not E.seq_match_enabled()
    monkeypatch.setenv('NAFP_SEQ_MATCH', '1')
    assert E.seq_match_enabled()
