"""CPU: the host side of tempo hypotheses -- the refusals of nafp_search_identify_tempo and of `--tempos` (before any GPU call), the
`--tempos` parser, the merge rule along slanted lines, `select_across_speeds` with a tempo, and the numpy restatement
(tests/_identify_tempo_ref.py): a planted (track, rho, a) is recovered, and the single hypothesis 65536 is tests/_identify_ref.py."""
import ctypes

import numpy as np
import pytest

import _identify_ref as R1
import _identify_tempo_ref as R

OK, INVALID, UNSUPPORTED = 0, 1, 2
ONE = 1 << 16


# ---- the entry point's refusals -------------------------------------------------------------------------------------------------
def _call(lib, p=ctypes.c_void_p(16), n_query=10, n_index=100, dim=128, k=20, n_tasks=1, max_len=20, n_tracks=1, rho=(ONE,), n_rho=None,
          min_overlap=4, min_votes=2, n_short=32, n_out=1, null=()):
    """nafp_search_identify_tempo with `p` for every device pointer (never dereferenced: every call here is refused first, or has
    nothing to launch), a real host array for rho, None for the names in `null`."""
    a = {n: (None if n in null else p) for n in ('query', 'index', 'topk', 'q0', 'len', 'first', 'track', 'align', 'score', 'votes',
                                                  'overlap', 'n_cand', 'rho_out')}
    rho = np.asarray(rho, np.int32)
    return lib.nafp_search_identify_tempo(a['query'], n_query, a['index'], n_index, dim, a['topk'], k, a['q0'], a['len'], n_tasks, max_len,
                                          a['first'], n_tracks, None if 'rho' in null else rho.ctypes.data, len(rho) if n_rho is None else n_rho,
                                          min_overlap, min_votes, n_short, n_out, a['track'], a['align'], a['score'], a['votes'],
                                          a['overlap'], a['n_cand'], a['rho_out'], None)


def test_identify_tempo_refuses_before_any_gpu_call(nafp):
    lib = nafp._lib.load()
    for name in ('query', 'index', 'topk', 'q0', 'len', 'first', 'rho', 'track', 'align', 'score', 'votes', 'overlap', 'rho_out'):
        assert _call(lib, null=(name,)) == INVALID, name
    assert _call(lib, n_tasks=-1) == INVALID and _call(lib, n_query=-1) == INVALID and _call(lib, n_index=-1) == INVALID
    # the hypotheses
    assert _call(lib, rho=(ONE,) * 17) == UNSUPPORTED and _call(lib, n_rho=0) == UNSUPPORTED and _call(lib, n_rho=-1) == UNSUPPORTED
    assert _call(lib, rho=(52428,)) == UNSUPPORTED and _call(lib, rho=(81921,)) == UNSUPPORTED
    assert _call(lib, rho=(ONE, 0)) == UNSUPPORTED and _call(lib, rho=(ONE, -ONE)) == UNSUPPORTED
    assert _call(lib, k=4, rho=(ONE, 70000, 90000, ONE)) == UNSUPPORTED        # any of them, not only the first
    # k * max_len * n_rho: 8192 passes, one hypothesis more does not
    assert _call(lib, n_tasks=0, k=32, max_len=16, rho=(ONE,) * 16) == OK and _call(lib, n_tasks=0, k=1, max_len=512, rho=(ONE,) * 16) == OK
    assert _call(lib, k=32, max_len=17, rho=(ONE,) * 16) == UNSUPPORTED and _call(lib, k=1, max_len=513, rho=(ONE,) * 16) == UNSUPPORTED
    assert _call(lib, n_tasks=0, k=20, max_len=20, rho=(ONE,) * 16) == OK               # the default window under 16 hypotheses: 6400 slots
    # every limit of nafp_search_identify
    assert _call(lib, k=33) == UNSUPPORTED and _call(lib, k=0) == UNSUPPORTED
    assert _call(lib, k=1, max_len=8193) == UNSUPPORTED and _call(lib, k=32, max_len=257) == UNSUPPORTED
    assert _call(lib, dim=96) == UNSUPPORTED
    assert _call(lib, n_short=4, n_out=5) == UNSUPPORTED
    assert _call(lib, n_short=257) == UNSUPPORTED and _call(lib, n_short=0) == UNSUPPORTED
    assert _call(lib, n_short=64, n_out=33) == UNSUPPORTED and _call(lib, n_out=0) == UNSUPPORTED
    assert _call(lib, max_len=0) == UNSUPPORTED and _call(lib, min_overlap=0) == UNSUPPORTED and _call(lib, min_votes=0) == UNSUPPORTED
    assert _call(lib, n_index=(1 << 31) - (1 << 14) + 1) == UNSUPPORTED
    assert _call(lib, n_tracks=0) == UNSUPPORTED and _call(lib, n_tracks=(1 << 24) + 1) == UNSUPPORTED
    # inside the limits, nothing to do: OK without a launch (out_n_cand may be null)
    assert _call(lib, n_tasks=0) == OK and _call(lib, n_tasks=0, null=('n_cand',)) == OK
    assert _call(lib, n_tasks=0, rho=(52429, 81920)) == OK
    assert _call(lib, n_tasks=0, k=32, max_len=256, n_short=256, n_out=32, n_index=(1 << 31) - (1 << 14), n_tracks=1 << 24) == OK


# ---- --tempos -------------------------------------------------------------------------------------------------------------------
def test_tempo_spec(nafp):
    from neural_audio_fp_amd.eval.identify import MAX_TEMPOS, parse_tempos
    assert MAX_TEMPOS == 16
    assert parse_tempos('0.9,1,1.1') == [ONE, round(ONE * 0.9), round(ONE * 1.1)]      # |rho - 1| ties (6554 both): the smaller value
    assert parse_tempos('1.1,0.9,1') == parse_tempos('0.9,1,1.1')                       # the order given does not matter
    assert parse_tempos('1.04, 0.98') == [round(ONE * 0.98), round(ONE * 1.04)]         # nearest 1 first
    got = parse_tempos('0.96:1.04:0.01')
    assert len(got) == 9 and got[0] == ONE and got[1:3] == [round(ONE * 0.99), round(ONE * 1.01)] and got[-1] == round(ONE * 1.04)
    assert all(abs(a - ONE) <= abs(b - ONE) for a, b in zip(got, got[1:]))
    assert parse_tempos(' 1 , 0.99:1.01:0.01, 1.0') == [ONE, round(ONE * 0.99), round(ONE * 1.01)]      # named twice, kept once
    assert parse_tempos('1,1.000001,0.999999') == [ONE]                                  # duplicates AFTER rounding
    assert parse_tempos('0.8,1.25') == [52429, 81920]
    assert len(parse_tempos('0.8:1.25:0.03')) == 16
    # 17 values that round to 16 hypotheses pass; 17 hypotheses do not
    assert len(parse_tempos(','.join(['1.0000001'] + [str(0.9 + 0.01 * k) for k in range(MAX_TEMPOS)]))) == MAX_TEMPOS
    for bad, word in (('', 'not a tempo'), ('fast', 'not a tempo'), ('1,,1.04', 'not a tempo'), ('0.9:1.1', 'not a tempo'),
                      ('0.9:1.1:0.1:3', 'not a tempo'), ('1.1:0.9:0.01', 'lo <= hi'), ('0.9:1.1:0', 'inc > 0'), ('0.9:1.1:-0.1', 'inc > 0'),
                      ('0.79', 'outside'), ('1,1.26', 'outside'), ('0.7:1.0:0.1', 'outside'), ('nan', 'outside'), ('inf', 'outside'),
                      ('0.9:1.1:nan', 'outside'), ('0.9:1.1:1e-320', 'at most 16'), ('0.9:1.1:0.01', 'at most 16'),
                      (','.join(str(0.9 + 0.01 * k) for k in range(MAX_TEMPOS + 1)), 'at most 16')):
        with pytest.raises(ValueError, match=word) as e:
            parse_tempos(bad)
        assert str(e.value).startswith('--tempos')


def test_identify_refuses_bad_tempos_first(nafp, cfg):
    """Before the library is looked for, let alone a GPU call: the paths below do not exist."""
    from neural_audio_fp_amd.eval.identify import identify
    for bad, word in (('1.3', 'outside'), ('0.9:1.1:0.01', 'at most 16'), ('x', 'not a tempo')):
        with pytest.raises(SystemExit, match=word):
            identify(cfg, 'no_such_experiment', '1', ['/nonexistent/recording.wav'], emb_dir='/nonexistent/emb/', tempos=bad)
    # window x k_probe x n_tempos: 20 x 20 x 20 would be refused by the parser (16), 20 x 20 x 16 = 6400 passes this check and goes
    # on to miss the library; 32 x 32 x 9 = 9216 is refused by name
    with pytest.raises(SystemExit, match=r'--tempos.*9216 slots.*nafp_search_identify_tempo.*8192'):
        identify(cfg, 'no_such_experiment', '1', ['/nonexistent/recording.wav'], emb_dir='/nonexistent/emb/', window=32, k_probe=32,
                 tempos='0.96:1.04:0.01')
    with pytest.raises(SystemExit, match='is missing'):
        identify(cfg, 'no_such_experiment', '1', ['/nonexistent/recording.wav'], emb_dir='/nonexistent/emb/', tempos='0.85:1.15:0.02')
    with pytest.raises(SystemExit, match='not a speed'):          # both options: each is parsed before anything else happens
        identify(cfg, 'no_such_experiment', '1', ['/nonexistent/recording.wav'], emb_dir='/nonexistent/emb/', tempos='1', speeds='x')


# ---- the merge along slanted lines ----------------------------------------------------------------------------------------------
def _merge(rows, **kw):
    from neural_audio_fp_amd.eval.identify import merge_windows
    rec, s0, ln, tr, al, sc, vo, rho = (np.asarray(c) for c in zip(*rows))
    return merge_windows(rec, s0, ln, tr, al, sc.astype(np.float32), vo, rho=rho, **kw)


def _merge_plain(rows):
    """The same windows through the merge without a tempo."""
    from neural_audio_fp_amd.eval.identify import merge_windows
    rec, s0, ln, tr, al, sc, vo, _ = (np.asarray(c) for c in zip(*rows))
    return merge_windows(rec, s0, ln, tr, al, sc.astype(np.float32), vo)


def test_merge_windows_under_tempo(nafp):
    from neural_audio_fp_amd.eval.identify import tempo_off
    r110, r105, r090 = round(ONE * 1.1), round(ONE * 1.05), round(ONE * 0.9)
    assert [tempo_off(n, r110) for n in (0, 1, 4, 5, 10)] == [0, 1, 4, 6, 11] and tempo_off(10, r090) == 9 and tempo_off(7, ONE) == 7
    # a recording at tempo 1.1 from library row 200: the window at segment s starts at row 200 + off(s)
    line = lambda s, rho=r110: 200 + tempo_off(s, rho)
    rows = [(0, s, 8, 3, line(s), sc, 8, r110) for s, sc in ((0, .8), (4, .9), (8, .7), (12, .85))]
    (m,) = _merge(rows)
    assert (m['track'], m['seg0'], m['seg1'], m['windows'], m['rho']) == (3, 0, 20, 4, r110)
    assert m['a_rec'] == line(4) - tempo_off(4, r110) == 200      # extrapolated from the best-scoring window to segment 0
    # with rho = 1 the rule of the plain merge (a_rec = align - s0) would break this run at once: 4 segments on, the line is 4.4 rows on ...
    plain = _merge_plain(rows)
    assert len(plain) == 1                                         # ... which align_tol = 1 still absorbs at a hop of 4;
    far = [(0, s, 8, 3, line(s), .9, 8, r110) for s in (0, 20, 40)]
    assert len(_merge(far)) == 1                                   # at a hop of 20 it does not (2 rows of drift per window), the slanted rule does
    assert len(_merge_plain(far)) == 3
    # the tempo index flips between neighbouring hypotheses from window to window: still one run, each step taken along the line
    # of the window before; the match reports the best-scoring window's rho
    flip = [(0, 0, 8, 3, 200, .8, 8, r110), (0, 4, 8, 3, 204, .95, 8, r105), (0, 8, 8, 3, 209, .7, 8, r110), (0, 12, 8, 3, 213, .7, 8, r105)]
    (m,) = _merge(flip)
    assert m['windows'] == 4 and m['rho'] == r105 and m['a_rec'] == 204 - tempo_off(4, r105) == 200
    # a run that must break: the same track, but the line of the window before predicts row 204 + off(4) = 208, and 211 is 3 away
    two = _merge(flip[:2] + [(0, 8, 8, 3, 211, .7, 8, r110)])
    assert [(x['seg0'], x['seg1'], x['windows']) for x in two] == [(0, 12, 2), (8, 16, 1)]
    assert len(_merge(flip[:2] + [(0, 8, 8, 3, 211, .7, 8, r110)], align_tol=3)) == 1
    # the prediction uses the PREVIOUS window's rho: under 0.9 four segments advance 4 rows (3.6 rounded), under 1.1 they advance 4 too,
    # ten segments advance 9 and 11
    assert len(_merge([(0, 0, 8, 3, 200, .9, 8, r090), (0, 10, 8, 3, 209, .9, 8, r110)])) == 1
    assert len(_merge([(0, 0, 8, 3, 200, .9, 8, r110), (0, 10, 8, 3, 209, .9, 8, r090)])) == 2
    # another track, another recording, a window without a result or below the threshold: as in the plain merge
    assert len(_merge([(0, 0, 8, 3, 200, .9, 8, r110), (0, 4, 8, 4, 204, .9, 8, r110)])) == 2
    assert [x['rec'] for x in _merge([(0, 0, 8, 3, 200, .9, 8, r110), (1, 0, 8, 3, 200, .9, 8, r110)])] == [0, 1]
    assert len(_merge([(0, 0, 8, 3, 200, .9, 8, r110), (0, 4, 8, -1, 0, -np.inf, 0, ONE), (0, 8, 8, 3, 209, .9, 8, r110)])) == 2
    assert len(_merge([(0, 0, 8, 3, 200, .9, 8, r110), (0, 4, 8, 3, 204, .2, 8, r110), (0, 8, 8, 3, 209, .9, 8, r110)], min_score=.5)) == 2
    # rho = 1 everywhere: the plain merge's matches, plus `rho`
    ones = [(0, 0, 8, 3, 100, .5, 8, ONE), (0, 4, 8, 3, 105, .9, 8, ONE), (0, 8, 8, 3, 110, .9, 8, ONE)]
    got, want = _merge(ones), _merge_plain(ones)
    assert [{k: v for k, v in m.items() if k != 'rho'} for m in got] == want and 'rho' not in want[0] and got[0]['rho'] == ONE


def test_select_across_speeds_with_a_tempo(nafp):
    from neural_audio_fp_amd.eval.identify import select_across_speeds as sel
    m = lambda score, speed, tempo: {'recording': 'r', 'recording_span_s': [0, 8], 'score': score, 'speed': speed, 'tempo': tempo, 'track': 't'}
    assert sel([m(.9, 1.04, 1.0), m(.9, 1.0, 1.04)])[0]['speed'] == 1.0             # score ties: the speed nearest 1 first,
    assert sel([m(.9, 1.0, 1.04), m(.9, 1.0, 1.02)])[0]['tempo'] == 1.02            # then the tempo nearest 1,
    assert sel([m(.9, 1.0, 2.0), m(.9, 1.0, 0.5)])[0]['tempo'] == 0.5               # then the lower tempo
    assert sel([m(.9, 1.0, 1.0), m(.95, 1.04, 1.1)])[0]['score'] == .95             # the score comes before both


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_recovers_a_planted_line():
    rng = np.random.default_rng(11)
    first = np.array([0, 30, 31, 90, 200])
    n_index, k, length = 200, 6, 20
    rhos = [ONE, round(ONE * 0.93), round(ONE * 1.07), round(ONE * 0.8), round(ONE * 1.25)]
    x = rng.normal(size=(n_index, 16))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    def planted(r, a):
        topk = rng.integers(-2, n_index + 3, size=(length, k))
        rows = a + R.off(np.arange(length), rhos[r])
        topk[:, 1] = rows
        query = x[rows] + 0.01 * rng.normal(size=(length, 16))
        out = R.identify(topk, [0], [length], length, length, n_index, first, rhos, R.score_f64(query, x), min_overlap=4, min_votes=2,
                         n_short=64, n_out=2)
        return rows, {(int(out['track'][0, n]), int(out['rho'][0, n]), int(out['align'][0, n])): (int(out['votes'][0, n]), int(out['overlap'][0, n]),
                                                                                                 float(out['score'][0, n])) for n in range(2)}, out

    for r, a in ((1, 95), (2, 40), (3, 100), (4, 120), (0, 50)):   # lines that lie inside one track
        rows, top, out = planted(r, a)
        tr = int(np.searchsorted(first, a, side='right')) - 1
        assert (out['track'][0, 0], out['rho'][0, 0], out['align'][0, 0]) == (tr, r, a), (r, a, top)
        assert out['overlap'][0, 0] == length and out['votes'][0, 0] >= length and out['score'][0, 0] > 0.99
    # a line through two tracks is two candidates, each scored over its own rows: 80 + off(i) is 89 at i = 7 and 90 at i = 8
    rows, top, _ = planted(4, 80)
    assert set(top) == {(2, 4, 80), (3, 4, 80)} and top[(2, 4, 80)][1] == 8 and top[(3, 4, 80)][1] == 12
    assert top[(2, 4, 80)][0] >= 8 and top[(3, 4, 80)][0] >= 12 and min(v[2] for v in top.values()) > 0.99
    # overlap by brute force: a before the track, a window off the track's end, the one-row track, and nothing in common
    assert R.overlap(25, rhos[2], 20, 30, 31) == (5, 6)             # 25 + off(5) = 30 is the one row of track 1; 25 + off(6) = 31
    assert R.overlap(-5, ONE, 20, 0, 30) == (5, 20) and R.overlap(20, ONE, 20, 0, 30) == (0, 10)
    assert R.overlap(100, ONE, 20, 0, 30) == (0, 0) and R.overlap(-40, ONE, 20, 0, 30) == (20, 20)
    assert R.overlap(28, rhos[4], 8, 30, 31) == (2, 2)              # 28 + off(1) = 29, 28 + off(2) = 31: the slanted line steps over the row


def test_single_hypothesis_one_is_the_plain_restatement():
    rng = np.random.default_rng(7)
    for case in range(40):
        n_tracks = int(rng.integers(1, 7))
        first = np.concatenate([[0], np.cumsum(rng.integers(1, 12, size=n_tracks))])
        n_index = int(first[-1])
        k, length, T = int(rng.integers(1, 6)), int(rng.integers(1, 10)), 4
        nq = T * length + int(rng.integers(0, 4))
        topk = rng.integers(-2, n_index + 3, size=(nq, k))
        q0 = rng.integers(-1, nq + 1, size=T)
        ln = rng.integers(0, length + 3, size=T)
        if case % 3 == 0:                                          # a planted alignment, so that votes above 1 occur
            q0[0] = 0
            topk[:, 0] = np.clip(int(rng.integers(-length, n_index)) + np.arange(nq), -1, n_index)
        query, x = rng.normal(size=(nq, 8)), rng.normal(size=(n_index, 8))
        mo, mv, ns, no = int(rng.integers(1, 5)), int(rng.integers(1, 4)), int(rng.integers(1, 8)), int(rng.integers(1, 4))
        got = R.identify(topk, q0, ln, length, nq, n_index, first, [ONE], R.score_f64(query, x), mo, mv, ns, no)
        want = R1.identify(topk, q0, ln, length, nq, n_index, first, R1.score_f64(query, x), mo, mv, ns, no)
        for n in ('track', 'align', 'score', 'votes', 'overlap', 'n_cand'):
            assert got[n].tobytes() == want[n].tobytes(), (case, n)
        assert np.array_equal(got['rho'], np.where(want['track'] >= 0, 0, -1))
