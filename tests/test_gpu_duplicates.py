"""GPU: `run.py duplicates` (neural-audio-fp_amd/eval/duplicates.py) on a library written directly -- custom_source.mm, its shape
and its track table in a temporary directory; no model, no audio.

The library: 12 tracks of 30 .. 120 rows, d = 128, every entry an integer in -2 .. 2, so every dot product, key and distance is
exact in float32 and the masked search is determined bit for bit.
  track 2  an exact copy of track 0 (80 rows)
  track 4  7 rows of its own, then rows 10 .. 49 of track 3, then 15 rows of its own: track 4's segment = track 3's segment - 3
  track 6  track 5 (90 rows) with +-1 on five coordinates of every row
  the rest unrelated.
A row of this alphabet has |x|^2 = 256 on average, so a window laid on its copy scores about 256, and one laid on unrelated rows
0 +- 22 / sqrt(rows): `--min_score 64`, the user's threshold, is what tells them apart here (without one every window reports its
best candidate, as in `identify`).

Every window's (track, align, votes) is held EQUAL to the numpy pipeline -- tests/_search_excl_ref.py for the masked search, then
tests/_identify_ref.py ranking by the bits of nafp_search_seq_scores, as tests/test_gpu_identify.py does -- with no threshold at
all, and the pairs, spans, offsets and groups are stated below from the construction."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import _identify_ref as R
import _search_excl_ref as xr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 128
LENS = [80, 60, 80, 100, 62, 90, 90, 30, 120, 45, 33, 71]
FIRST = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
N = int(FIRST[-1])
HOP_S, DUR_S = 0.5, 1.0
PARAMS = dict(window=20, window_hop=10, k_probe=20, min_overlap=4, min_votes=2, n_short=32)


@functools.lru_cache(maxsize=None)
def _rows():
    rng = np.random.default_rng(2031)
    t = [rng.integers(-2, 3, size=(n, D)).astype(np.float32) for n in LENS]
    t[2] = t[0].copy()
    t[4][7:47] = t[3][10:50]
    t[6] = t[5].copy()
    for r in range(LENS[6]):
        c = rng.permutation(D)[:5]
        t[6][r, c] = np.clip(t[6][r, c] + rng.choice([-1, 1], size=5), -3, 3)
    x = np.concatenate(t)
    assert x.shape == (N, D) and np.array_equal(x, np.round(x))
    return x


def _write_library(path):
    d = str(path) + '/'
    os.makedirs(d, exist_ok=True)
    _rows().tofile(d + 'custom_source.mm')
    np.save(d + 'custom_source_shape.npy', np.array([N, D]))
    with open(d + 'custom_source_tracks.json', 'w') as f:
        json.dump({'files': [f'/lib/track{t:02d}.wav' for t in range(len(LENS))], 'first': [int(v) for v in FIRST], 'hop_s': HOP_S,
                   'duration_s': DUR_S}, f)
    return d


def _flat(nafp):
    from neural_audio_fp_amd.eval.eval_faiss import FlatL2Index
    flat = FlatL2Index(D)
    flat.add(_rows())
    return flat


def test_every_window_equals_the_numpy_pipeline(nafp):
    from neural_audio_fp_amd.eval import duplicates as dup
    from neural_audio_fp_amd.eval.identify import plan_windows
    x = _rows()
    flat = _flat(nafp)
    rec, s0, ln, track, align, score, votes = dup.match_library(flat, FIRST, **PARAMS)
    # the numpy pipeline: masked search, then the matcher's restatement ranking by the bits of nafp_search_seq_scores
    tr = np.searchsorted(FIRST, np.arange(N), side='right') - 1
    excl = np.stack([FIRST[tr], FIRST[tr + 1]], 1)
    _, ids = xr.topk_excl_exact(x, x, PARAMS['k_probe'], excl)
    assert not ((ids >= excl[:, :1]) & (ids < excl[:, 1:])).any() and (ids >= 0).all()
    w_rec, w_s0, w_ln = plan_windows(np.diff(FIRST), PARAMS['window'], PARAMS['window_hop'])
    assert np.array_equal(rec, w_rec) and np.array_equal(s0, w_s0) and np.array_equal(ln, w_ln)
    q0 = (FIRST[w_rec] + w_s0).astype(np.int32)
    xd = torch.from_numpy(x).cuda()

    def yardstick(q_start, n_ov, cand):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32))).cuda()
        return flat.sequence_scores(xd, dev(q_start), dev(n_ov), dev(np.asarray(cand)[:, None])).cpu().numpy()[:, 0]
    want = R.identify(ids, q0, w_ln.astype(np.int32), PARAMS['window'], N, N, FIRST, yardstick, PARAMS['min_overlap'], PARAMS['min_votes'],
                      PARAMS['n_short'], 1)
    assert np.array_equal(track, want['track'][:, 0]) and np.array_equal(align, want['align'][:, 0])
    assert np.array_equal(votes, want['votes'][:, 0])
    assert score.tobytes() == want['score'][:, 0].tobytes()          # the bits of nafp_search_seq_scores on the overlap
    # and the float64 mean: the sums are exact integers, only the division rounds
    x64 = x.astype(np.float64)
    for w in np.nonzero(track >= 0)[0]:
        t, a = int(track[w]), int(align[w])
        i0, i1 = max(0, int(FIRST[t]) - a), min(int(ln[w]), int(FIRST[t + 1]) - a)
        exact = (x64[q0[w] + i0:q0[w] + i1] * x64[a + i0:a + i1]).sum() / (i1 - i0)
        assert abs(float(score[w]) - exact) <= 2.0 ** -23 * abs(exact), (w, float(score[w]), exact)
    assert not (track == rec).any()                                  # never the own track
    # chunks of whole tracks of at most 64 rows (most tracks alone, tracks of 30 and 33 rows too): the same bytes
    small = dup.match_library(flat, FIRST, chunk_rows=64, **PARAMS)
    for a, b in zip(small, (rec, s0, ln, track, align, score, votes)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_result(res):
    assert res['index_type_used'].startswith('L2') and res['n_tracks'] == 12 and res['n_rows'] == N
    assert res['n_windows'] == sum(max(1, -(-(n - 20) // 10) + 1) for n in LENS)
    by = {(p['a_index'], p['b_index']): p for p in res['pairs']}
    assert sorted(by) == [(0, 2), (3, 4), (5, 6)] and len(res['pairs']) == 3
    assert [(p['a_index'], p['b_index']) for p in res['pairs']] == sorted(by)
    span = lambda a, b: [a * HOP_S, (b - 1) * HOP_S + DUR_S]
    p = by[(0, 2)]                                                   # the exact copy: the whole track, both directions
    assert p['a'] == '/lib/track00.wav' and p['b'] == '/lib/track02.wav'
    assert p['a_span_s'] == span(0, 80) and p['b_span_s'] == span(0, 80) and p['offset_s'] == 0.0
    assert p['directions'] == 2 and p['coverage'] == 1.0 and p['score'] > 250 and p['windows'] == 14 and p['min_votes'] >= 20
    p = by[(5, 6)]                                                   # the perturbed copy
    assert p['a_span_s'] == span(0, 90) and p['b_span_s'] == span(0, 90) and p['offset_s'] == 0.0
    assert p['directions'] == 2 and p['coverage'] == 1.0 and p['score'] > 240 and p['windows'] == 16
    # rows 10 .. 49 of track 3 inside track 4 at 7: track 4's segment = track 3's - 3.  The spans are made of whole windows: of track
    # 3 those that hold at least 10 copied rows (0 .. 59), of track 4 those from 0 to 59 (the window at 40 holds 7 copied rows of 20 and
    # scores 7 / 20 of 256, above the threshold), clipped to the segments both tracks have: [3, 63) of track 3, [0, 60) of track 4
    p = by[(3, 4)]
    assert p['offset_s'] == -3 * HOP_S and p['directions'] == 2
    assert p['a_span_s'] == span(3, 63) and p['b_span_s'] == span(0, 60) and p['coverage'] == 60 / 62
    assert [g['tracks'] for g in res['groups']] == [[0, 2], [3, 4], [5, 6]]
    assert res['groups'][1]['files'] == ['/lib/track03.wav', '/lib/track04.wav']


def test_pairs_groups_chunks_and_the_command_line(nafp, cfg, tmp_path):
    import copy
    from neural_audio_fp_amd.eval import duplicates as dup
    work = tmp_path / 'work'
    (work / 'config').mkdir(parents=True)
    c = copy.deepcopy(cfg)
    c['DIR'].update({'OUTPUT_ROOT_DIR': str(work) + '/logs/emb/', 'LOG_ROOT_DIR': str(work) + '/logs/'})
    yaml.safe_dump(c, open(work / 'config' / 'tiny.yaml', 'w'))
    emb = _write_library(work / 'logs' / 'emb' / 'EXP' / '1')
    res = dup.duplicates(c, 'EXP', '1', min_score=64.0, **PARAMS)
    assert json.load(open(emb + 'duplicates.json')) == res
    _check_result(res)
    # chunks of at most 64 rows: identical JSON
    out64 = str(tmp_path / 'chunks64.json')
    dup.duplicates(c, 'EXP', '1', min_score=64.0, chunk_rows=64, output=out64, **PARAMS)
    assert open(out64).read() == open(emb + 'duplicates.json').read()
    # --min_coverage above the partial copy's 60 / 62 cuts that link only
    cut = dup.duplicates(c, 'EXP', '1', min_score=64.0, min_coverage=0.99, output=str(tmp_path / 'cut.json'), **PARAMS)
    assert [g['tracks'] for g in cut['groups']] == [[0, 2], [5, 6]] and len(cut['pairs']) == 3
    # the command line, in a process of its own
    out = str(tmp_path / 'cli.json')
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), 'duplicates', 'EXP', '1', '-c', 'tiny', '--min_score', '64',
                        '--output', out], cwd=work, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'track00.wav' in r.stdout and 'group 0: track00.wav, track02.wav' in r.stdout
    assert open(out).read() == open(emb + 'duplicates.json').read()
    # a library without its track table is refused by name
    os.remove(emb + 'custom_source_tracks.json')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), 'duplicates', 'EXP', '1', '-c', 'tiny'], cwd=work, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and 'NAFP_TRACK_TABLE=1' in r.stdout + r.stderr
