"""CPU: identification's host side -- the numpy restatement of nafp_search_identify against a brute-force count, the track table
checker and the argument refusals of the entry point (before any GPU call), the window plan, the merge, and the track table
`generate` writes under NAFP_TRACK_TABLE=1."""
import ctypes
import json
import os
import wave

import numpy as np
import pytest

import _identify_ref as R

OK, INVALID, UNSUPPORTED = 0, 1, 2


# ---- the restatement against a dictionary count -------------------------------------------------------------------------------
def _brute(topk, q0, length, n_index, first, min_overlap, min_votes, n_short):
    votes = {}
    for i in range(length):
        for j in range(topk.shape[1]):
            idx = int(topk[q0 + i, j])
            if 0 <= idx < n_index:
                tr = max(t for t in range(len(first) - 1) if first[t] <= idx)
                votes[(tr, idx - i)] = votes.get((tr, idx - i), 0) + 1
    rows = []
    for (tr, a), v in votes.items():
        i0, i1 = max(0, first[tr] - a), min(length, first[tr + 1] - a)
        assert i1 - i0 >= 1                                        # by construction
        if i1 - i0 >= min(min_overlap, length) and v >= min_votes:
            rows.append((tr, a, v, i0, i1 - i0))
    rows.sort(key=lambda r: (-r[2], r[0], r[1]))
    return rows[:n_short], len(rows)


def test_restatement_equals_a_dictionary_count():
    rng = np.random.default_rng(7)
    for case in range(60):
        n_tracks = int(rng.integers(1, 7))
        lens = rng.integers(1, 12, size=n_tracks)
        first = np.concatenate([[0], np.cumsum(lens)])
        n_index = int(first[-1])
        k, length = int(rng.integers(1, 6)), int(rng.integers(1, 10))
        nq = length + int(rng.integers(0, 4))
        q0 = int(rng.integers(0, nq - length + 1))
        topk = rng.integers(-2, n_index + 3, size=(nq, k))
        if case % 3 == 0:                                          # a planted alignment, so that votes above 1 occur
            a = int(rng.integers(-length, n_index))
            col = np.clip(a + np.arange(nq) - q0, -1, n_index)
            topk[:, 0] = col
        mo, mv, ns = int(rng.integers(1, 5)), int(rng.integers(1, 4)), int(rng.integers(1, 8))
        got, n_cand = R.shortlist(topk, q0, length, n_index, first, mo, mv, ns)
        want, want_n = _brute(topk, q0, length, n_index, [int(v) for v in first], mo, mv, ns)
        assert n_cand == want_n and [tuple(int(v) for v in r) for r in got] == want, case


def test_restatement_ranks_by_the_scores_it_is_given():
    first = np.array([0, 4, 8])
    topk = np.array([[0, 4], [1, 5], [2, 6]])                      # alignment 0 through track 0, alignment 4 through track 1
    table = {(0, 3, 0): 0.5, (0, 3, 4): 0.5}
    fn = lambda q, n, c: np.array([table[(int(a), int(b), int(d))] for a, b, d in zip(q, n, c)], np.float32)
    out = R.identify(topk, [0, 5, 0], [3, 3, 0], 3, 3, 8, first, fn, min_overlap=1, min_votes=1, n_short=4, n_out=3)
    assert out['track'][0].tolist() == [0, 1, -1] and out['align'][0].tolist() == [0, 4, 0]      # equal scores: the smaller track first
    assert out['votes'][0].tolist() == [3, 3, 0] and out['overlap'][0].tolist() == [3, 3, 0] and out['n_cand'].tolist() == [2, 0, 0]
    assert out['track'][1].tolist() == [-1, -1, -1] and np.all(out['score'][1:] == -np.inf)       # q0 out of range; an empty task
    table[(0, 3, 0)] = np.nan                                      # a NaN score drops the candidate, n_cand still counts it
    out = R.identify(topk, [0], [3], 3, 3, 8, first, fn, min_overlap=1, min_votes=1, n_short=4, n_out=2)
    assert out['track'][0].tolist() == [1, -1] and out['n_cand'].tolist() == [2]


# ---- the library's host-side checks -------------------------------------------------------------------------------------------
def _check(lib, first, n_index):
    first = np.asarray(first, np.int32)
    return lib.nafp_search_identify_check_tracks_host(first.ctypes.data, len(first) - 1, n_index)


def test_track_table_checker(nafp):
    lib = nafp._lib.load()
    assert _check(lib, [0, 1, 3, 8, 48], 48) == OK
    assert _check(lib, [0, 48], 48) == OK
    assert _check(lib, [1, 3, 8, 48], 48) == INVALID                # first[0] != 0
    assert _check(lib, [0, 1, 3, 8, 47], 48) == INVALID             # the last entry is not n_index
    assert _check(lib, [0, 1, 3, 8, 49], 48) == INVALID
    assert _check(lib, [0, 3, 3, 8, 48], 48) == INVALID             # a repeated entry
    assert _check(lib, [0, 8, 3, 9, 48], 48) == INVALID             # a decreasing entry
    assert lib.nafp_search_identify_check_tracks_host(None, 1, 48) == INVALID
    assert lib.nafp_search_identify_check_tracks_host(np.zeros(2, np.int32).ctypes.data, 0, 48) == INVALID


def _call(lib, p=ctypes.c_void_p(16), n_query=10, n_index=100, dim=128, k=20, n_tasks=1, max_len=20, n_tracks=1, min_overlap=4,
          min_votes=2, n_short=32, n_out=1, null=()):
    """nafp_search_identify with `p` for every pointer (never dereferenced: every call here is refused first), None for `null`."""
    a = {n: (None if n in null else p) for n in ('query', 'index', 'topk', 'q0', 'len', 'first', 'track', 'align', 'score', 'votes',
                                                  'overlap', 'n_cand')}
    return lib.nafp_search_identify(a['query'], n_query, a['index'], n_index, dim, a['topk'], k, a['q0'], a['len'], n_tasks, max_len,
                                    a['first'], n_tracks, min_overlap, min_votes, n_short, n_out, a['track'], a['align'], a['score'],
                                    a['votes'], a['overlap'], a['n_cand'], None)


def test_identify_refuses_before_any_gpu_call(nafp):
    lib = nafp._lib.load()
    assert lib.nafp_search_identify(None, 10, None, 100, 128, None, 20, None, None, 1, 20, None, 1, 4, 2, 32, 1, None, None, None,
                                    None, None, None, None) == INVALID
    for name in ('query', 'index', 'topk', 'q0', 'len', 'first', 'track', 'align', 'score', 'votes', 'overlap'):
        assert _call(lib, null=(name,)) == INVALID, name
    assert _call(lib, n_tasks=-1) == INVALID and _call(lib, n_query=-1) == INVALID and _call(lib, n_index=-1) == INVALID
    assert _call(lib, k=33) == UNSUPPORTED and _call(lib, k=0) == UNSUPPORTED
    assert _call(lib, k=1, max_len=8193) == UNSUPPORTED and _call(lib, k=32, max_len=257) == UNSUPPORTED      # k * max_len = 8193, 8224
    assert _call(lib, dim=96) == UNSUPPORTED
    assert _call(lib, n_short=4, n_out=5) == UNSUPPORTED            # n_out > n_short
    assert _call(lib, n_short=257) == UNSUPPORTED and _call(lib, n_short=0) == UNSUPPORTED
    assert _call(lib, n_short=64, n_out=33) == UNSUPPORTED and _call(lib, n_out=0) == UNSUPPORTED
    assert _call(lib, max_len=0) == UNSUPPORTED and _call(lib, min_overlap=0) == UNSUPPORTED and _call(lib, min_votes=0) == UNSUPPORTED
    assert _call(lib, n_index=(1 << 31) - (1 << 14) + 1) == UNSUPPORTED
    assert _call(lib, n_tracks=0) == UNSUPPORTED and _call(lib, n_tracks=(1 << 24) + 1) == UNSUPPORTED
    # inside the limits, nothing to do: OK without a launch (out_n_cand may be null)
    assert _call(lib, n_tasks=0) == OK and _call(lib, n_tasks=0, null=('n_cand',)) == OK
    assert _call(lib, n_tasks=0, k=32, max_len=256, n_short=256, n_out=32, n_index=(1 << 31) - (1 << 14), n_tracks=1 << 24) == OK


# ---- plan_windows / merge_windows ---------------------------------------------------------------------------------------------
def test_plan_windows(nafp):
    from neural_audio_fp_amd.eval.identify import plan_windows
    rec, s0, ln = plan_windows([5], 20, 10)                         # shorter than a window: one window of its own length
    assert (rec.tolist(), s0.tolist(), ln.tolist()) == ([0], [0], [5])
    rec, s0, ln = plan_windows([20], 8, 4)                          # an exact multiple: every window full, none beyond the end
    assert (s0.tolist(), ln.tolist()) == ([0, 4, 8, 12], [8, 8, 8, 8])
    rec, s0, ln = plan_windows([22], 8, 4)                          # the last window is shortened, not dropped
    assert (s0.tolist(), ln.tolist()) == ([0, 4, 8, 12, 16], [8, 8, 8, 8, 6])
    rec, s0, ln = plan_windows([8, 1, 9], 8, 4)                     # recordings in order; exactly one window, one segment, one over
    assert (rec.tolist(), s0.tolist(), ln.tolist()) == ([0, 1, 2, 2], [0, 0, 0, 4], [8, 1, 8, 5])
    for n in range(1, 40):                                          # every segment is inside some window
        _, s0, ln = plan_windows([n], 7, 3)
        covered = np.zeros(n, bool)
        for a, l in zip(s0, ln):
            covered[a:a + l] = True
        assert covered.all() and (s0 + ln).max() == n and ln.min() >= 1
    with pytest.raises(ValueError):
        plan_windows([4], 0, 1)


def _merge(rows, **kw):
    from neural_audio_fp_amd.eval.identify import merge_windows
    rec, s0, ln, tr, al, sc, vo = (np.asarray(c) for c in zip(*rows))
    return merge_windows(rec, s0, ln, tr, al, sc.astype(np.float32), vo, **kw)


def test_merge_windows(nafp):
    # two tracks back to back in one recording: windows 0, 4 on track 3 at a_rec 100, windows 8, 12 on track 5 at a_rec 300
    m = _merge([(0, 0, 8, 3, 100, .9, 8), (0, 4, 8, 3, 104, .7, 5), (0, 8, 8, 5, 308, .8, 6), (0, 12, 7, 5, 312, 1., 7)])
    assert [(x['track'], x['a_rec'], x['seg0'], x['seg1'], x['windows'], x['votes']) for x in m] == [(3, 100, 0, 12, 2, 5), (5, 300, 8, 19, 2, 6)]
    assert abs(m[0]['score'] - .8) < 1e-6 and abs(m[1]['score'] - .9) < 1e-6
    # +-1 jitter merges (a_rec 100, 101, 100), +-2 does not
    assert len(_merge([(0, 0, 8, 3, 100, .9, 8), (0, 4, 8, 3, 105, .9, 8), (0, 8, 8, 3, 108, .9, 8)])) == 1
    assert len(_merge([(0, 0, 8, 3, 100, .9, 8), (0, 4, 8, 3, 106, .9, 8)])) == 2
    assert len(_merge([(0, 0, 8, 3, 100, .9, 8), (0, 4, 8, 3, 102, .9, 8)])) == 2
    assert len(_merge([(0, 0, 8, 3, 100, .9, 8), (0, 4, 8, 3, 106, .9, 8)], align_tol=2)) == 1
    # the alignment reported is the best-scoring window's
    assert _merge([(0, 0, 8, 3, 100, .5, 8), (0, 4, 8, 3, 105, .9, 8)])[0]['a_rec'] == 101
    # a window below the threshold is no match and splits the run; without a threshold it merges
    rows = [(0, 0, 8, 3, 100, .9, 8), (0, 4, 8, 3, 104, .2, 8), (0, 8, 8, 3, 108, .9, 8)]
    assert len(_merge(rows)) == 1
    m = _merge(rows, min_score=.5)
    assert [(x['seg0'], x['seg1'], x['windows']) for x in m] == [(0, 8, 1), (8, 16, 1)]
    # a window without a result (track -1) splits too; the same track and alignment in ANOTHER recording is another match
    assert len(_merge([(0, 0, 8, 3, 100, .9, 8), (0, 4, 8, -1, 0, -np.inf, 0), (0, 8, 8, 3, 108, .9, 8)])) == 2
    assert [x['rec'] for x in _merge([(0, 0, 8, 3, 100, .9, 8), (1, 0, 8, 3, 100, .9, 8)])] == [0, 1]
    assert _merge([(0, 0, 8, -1, 0, -np.inf, 0)]) == []


# ---- the track table of `generate` --------------------------------------------------------------------------------------------
def _wav(path, n):
    with wave.open(str(path), 'w') as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(8000)
        w.writeframes(np.zeros(n, '<i2').tobytes())


def test_track_table_only_under_the_variable(nafp, cfg, tmp_path, monkeypatch):
    """`generate_fingerprint` on a custom source with the device work stubbed out: files of 1, 1, 2 and 39 segments."""
    from neural_audio_fp_amd.model import generate as G
    src = tmp_path / 'src'
    src.mkdir()
    for name, n in (('a', 4000), ('b', 8000), ('c', 12000), ('d', 160000)):      # half a segment, one, two, many
        _wav(src / f'{name}.wav', n)
    for k in ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS', 'NAFP_INGEST_FLAC', 'NAFP_MELSPEC_ANY'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(G, 'build_fp', lambda cfg: (None, None))
    monkeypatch.setattr(G, 'load_checkpoint', lambda *a, **k: 1)
    monkeypatch.setattr(G, 'StreamedEmbedder', lambda *a, **k: None)
    monkeypatch.setattr(G, 'write_fingerprints', lambda *a, **k: None)
    monkeypatch.delenv('NAFP_TRACK_TABLE', raising=False)
    G.generate_fingerprint(cfg, 'EXP', 1, str(src), str(tmp_path / 'plain'), True)
    assert sorted(os.listdir(tmp_path / 'plain' / 'EXP' / '1')) == ['custom_source.mm', 'custom_source_shape.npy']
    monkeypatch.setenv('NAFP_TRACK_TABLE', '1')
    G.generate_fingerprint(cfg, 'EXP', 1, str(src), str(tmp_path / 'table'), True)
    out = tmp_path / 'table' / 'EXP' / '1'
    assert sorted(os.listdir(out)) == ['custom_source.mm', 'custom_source_shape.npy', 'custom_source_tracks.json']
    t = json.load(open(out / 'custom_source_tracks.json'))
    assert t['first'] == [0, 1, 2, 4, 43] and t['first'][-1] == int(np.load(out / 'custom_source_shape.npy')[0])
    assert [os.path.basename(f) for f in t['files']] == ['a.wav', 'b.wav', 'c.wav', 'd.wav'] and all(os.path.isabs(f) or f.startswith(str(src)) for f in t['files'])
    assert (t['hop_s'], t['duration_s'], t['fs']) == (.5, 1., 8000)
    lib = nafp._lib.load()
    assert _check(lib, t['first'], 43) == OK


def test_identify_names_the_variable_when_a_table_is_missing(nafp, tmp_path):
    from neural_audio_fp_amd.eval.identify import load_track_tables
    with pytest.raises(SystemExit) as e:
        load_track_tables(str(tmp_path) + '/', ['dummy_db', 'db'], [(10, 128), (10, 128)])
    assert 'NAFP_TRACK_TABLE=1' in str(e.value)
    json.dump({'hop_s': .5, 'duration_s': 1., 'fs': 8000, 'files': ['x.wav', 'y.wav'], 'first': [0, 4, 10]}, open(tmp_path / 'dummy_db_tracks.json', 'w'))
    json.dump({'hop_s': .5, 'duration_s': 1., 'fs': 8000, 'files': ['z.wav'], 'first': [0, 7]}, open(tmp_path / 'db_tracks.json', 'w'))
    files, first, hop_s, dur_s = load_track_tables(str(tmp_path) + '/', ['dummy_db', 'db'], [(10, 128), (7, 128)])
    assert files == ['x.wav', 'y.wav', 'z.wav'] and first.tolist() == [0, 4, 10, 17] and first.dtype == np.int32 and (hop_s, dur_s) == (.5, 1.)
    with pytest.raises(SystemExit):                                # a table that does not describe its .mm file
        load_track_tables(str(tmp_path) + '/', ['dummy_db', 'db'], [(10, 128), (8, 128)])
