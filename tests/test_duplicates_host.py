"""CPU: the host side of `run.py duplicates` (neural-audio-fp_amd/eval/duplicates.py): the canonical form of a directed match,
folding, grouping, the chunk plan, and the refusals -- every one of which fires before the library is loaded."""
import json

import numpy as np
import pytest

from neural_audio_fp_amd.eval import duplicates as dup

N_SEG = [100, 60, 80, 40]                                           # segments of tracks 0 .. 3


def _m(x, y, seg0, seg1, pos, score=1.0, votes=5, windows=1):
    return {'rec': x, 'track': y, 'seg0': seg0, 'seg1': seg1, 'pos': pos, 'score': score, 'votes': votes, 'windows': windows}


def test_canonical_form():
    # X is lo: nothing moves
    assert dup.canonical(0, 1, 10, 50, 5, N_SEG) == (0, 1, 5, 10, 50, 0)
    # X > Y: track 1's segments [10, 50) are track 0's [15, 55): offset -pos, the span in lo's segments
    assert dup.canonical(1, 0, 10, 50, 5, N_SEG) == (0, 1, -5, 15, 55, 1)
    # the two directions of one duplicate agree: 0 -> 1 with pos -5 over [15, 55)
    assert dup.canonical(0, 1, 15, 55, -5, N_SEG)[:5] == (0, 1, -5, 15, 55)
    # clipping to lo's segments: track 2's [0, 30) at pos -10 would start at track 0's segment -10
    assert dup.canonical(2, 0, 0, 30, -10, N_SEG) == (0, 2, 10, 0, 20, 1)
    # ... and to those whose partner hi has: track 0's [30, 100) at pos 0 against the 60 segments of track 1
    assert dup.canonical(0, 1, 30, 100, 0, N_SEG) == (0, 1, 0, 30, 60, 0)
    assert dup.canonical(0, 1, 0, 20, -8, N_SEG) == (0, 1, -8, 8, 20, 0)      # hi's segment = lo's - 8 >= 0
    lo, hi, off, s0, s1, _ = dup.canonical(3, 1, 0, 40, 70, N_SEG)             # nothing left: track 1 has no segment 70
    assert s1 <= s0
    with pytest.raises(ValueError):
        dup.canonical(2, 2, 0, 5, 0, N_SEG)


def test_both_directions_fold_into_one_pair():
    pairs = dup.fold_matches([_m(0, 1, 10, 50, -10, 0.9, 7, 3), _m(1, 0, 0, 40, 10, 0.8, 4, 3)], N_SEG)
    assert len(pairs) == 1
    p = pairs[0]
    assert (p['lo'], p['hi'], p['offset'], p['s0'], p['s1']) == (0, 1, -10, 10, 50)
    assert p['score'] == 0.9 and p['votes'] == 4 and p['windows'] == 6 and p['directions'] == 2
    assert p['coverage'] == 40 / 60


def test_one_direction_only():
    pairs = dup.fold_matches([_m(2, 0, 0, 30, 20, 0.7, 3, 2)], N_SEG)
    assert len(pairs) == 1 and pairs[0]['directions'] == 1
    assert (pairs[0]['lo'], pairs[0]['hi'], pairs[0]['offset'], pairs[0]['s0'], pairs[0]['s1']) == (0, 2, -20, 20, 50)
    assert pairs[0]['coverage'] == 30 / 80


def test_offsets_within_and_beyond_align_tol():
    a, b = _m(0, 1, 10, 50, -10, 0.5), _m(1, 0, 0, 40, 11, 0.9)     # offsets -10 and -11
    one = dup.fold_matches([a, b], N_SEG, align_tol=1)
    assert len(one) == 1 and one[0]['directions'] == 2 and one[0]['offset'] == -11 and one[0]['score'] == 0.9      # the better member's
    assert (one[0]['s0'], one[0]['s1']) == (10, 51)                  # the union span
    two = dup.fold_matches([a, b], N_SEG, align_tol=0)
    assert len(two) == 2 and [p['directions'] for p in two] == [1, 1]
    far = dup.fold_matches([a, _m(1, 0, 0, 40, 13, 0.9)], N_SEG, align_tol=1)
    assert len(far) == 2


def test_spans_that_overlap_less_than_half_stay_apart():
    # the same pair and offset, spans [10, 30) and [25, 45): 5 of 20 segments shared
    pairs = dup.fold_matches([_m(0, 1, 10, 30, 0), _m(1, 0, 25, 45, 0)], N_SEG)
    assert [(p['s0'], p['s1'], p['directions']) for p in pairs] == [(10, 30, 1), (25, 45, 1)]
    # exactly half is not more than half
    assert len(dup.fold_matches([_m(0, 1, 10, 30, 0), _m(1, 0, 20, 40, 0)], N_SEG)) == 2
    assert len(dup.fold_matches([_m(0, 1, 10, 30, 0), _m(1, 0, 19, 39, 0)], N_SEG)) == 1
    # same direction twice (a match that broke in the middle) folds as well, and stays one direction
    p = dup.fold_matches([_m(0, 1, 10, 30, 0), _m(0, 1, 15, 45, 0)], N_SEG)
    assert len(p) == 1 and p[0]['directions'] == 1 and (p[0]['s0'], p[0]['s1']) == (10, 45)


def test_pairs_are_ordered_and_other_pairs_do_not_fold():
    pairs = dup.fold_matches([_m(3, 2, 0, 40, 0), _m(1, 0, 30, 50, 0), _m(0, 2, 0, 20, 0), _m(0, 1, 0, 12, 0)], N_SEG)
    assert [(p['lo'], p['hi'], p['s0']) for p in pairs] == [(0, 1, 0), (0, 1, 30), (0, 2, 0), (2, 3, 0)]


def test_groups_chain_and_min_coverage_cuts_a_link():
    pairs = dup.fold_matches([_m(0, 1, 0, 60, 0), _m(1, 0, 0, 60, 0), _m(1, 2, 0, 12, 0), _m(3, 2, 0, 40, 5)], N_SEG)
    assert [(p['lo'], p['hi']) for p in pairs] == [(0, 1), (1, 2), (2, 3)]
    assert [round(p['coverage'], 3) for p in pairs] == [1.0, 0.2, 1.0]
    assert dup.group_pairs(pairs, 0.0) == [[0, 1, 2, 3]]             # three links chain four tracks into one group
    assert dup.group_pairs(pairs, 0.5) == [[0, 1], [2, 3]]           # the 20 % link is cut
    assert dup.group_pairs(pairs, 1.01) == []                        # singletons are omitted
    assert dup.group_pairs([], 0.0) == []


def test_plan_chunks():
    first = np.array([0, 30, 60, 200, 210, 220, 300], np.int32)
    assert dup.plan_chunks(first, 1 << 20) == [(0, 6)]
    assert dup.plan_chunks(first, 64) == [(0, 2), (2, 3), (3, 5), (5, 6)]      # the 140-row track is a chunk of its own
    assert dup.plan_chunks(first, 1) == [(t, t + 1) for t in range(6)]
    with pytest.raises(ValueError):
        dup.plan_chunks(first, 0)


def test_pairs_from_windows_uses_the_alignment_in_the_tracks_frame():
    """Track 1 (rows 100 .. 159) equals rows 20 .. 79 of track 0 (rows 0 .. 99): the windows of both directions, as the matcher
    reports them (align = the library row segment 0 of the WINDOW falls on)."""
    first = np.array([0, 100, 160], np.int32)
    rec = np.array([0, 0, 0, 0, 1, 1, 1])
    s0 = np.array([20, 30, 40, 50, 0, 20, 40])
    ln = np.array([20, 20, 20, 20, 20, 20, 20])
    track = np.array([1, 1, 1, 1, 0, 0, 0])
    align = np.where(rec == 0, 100 + s0 - 20, s0 + 20)
    score = np.full(7, 0.95, np.float32)
    votes = np.array([20, 20, 20, 20, 20, 18, 20])
    directed, pairs = dup.pairs_from_windows(rec, s0, ln, track, align, score, votes, first)
    assert [(m['rec'], m['track'], m['seg0'], m['seg1'], m['pos']) for m in directed] == [(0, 1, 20, 70, -20), (1, 0, 0, 60, 20)]
    assert len(pairs) == 1
    p = pairs[0]
    assert (p['lo'], p['hi'], p['offset'], p['s0'], p['s1'], p['directions'], p['votes'], p['windows']) == (0, 1, -20, 20, 80, 2, 18, 7)
    assert p['coverage'] == 1.0
    _, none = dup.pairs_from_windows(rec, s0, ln, track, align, score, votes, first, min_score=0.99)
    assert none == []


# ---- refusals: all before any GPU call ------------------------------------------------------------------------------------------

def _library(tmp_path, n_tracks=3, tables=True, mm=True):
    d = str(tmp_path) + '/'
    first = [0] + [10 * (t + 1) for t in range(n_tracks)]
    if mm:
        np.zeros((first[-1], 128), np.float32).tofile(d + 'custom_source.mm')
        np.save(d + 'custom_source_shape.npy', np.array([first[-1], 128]))
    if tables:
        with open(d + 'custom_source_tracks.json', 'w') as f:
            json.dump({'files': [f't{t}.wav' for t in range(n_tracks)], 'first': first, 'hop_s': 0.5, 'duration_s': 1.0}, f)
    return d


@pytest.fixture
def no_gpu(monkeypatch):
    """Anything that would reach the library or the device raises."""
    from neural_audio_fp_amd import _lib
    from neural_audio_fp_amd.eval import eval_faiss

    def boom(*a, **k):
        raise AssertionError('the GPU library was reached before the refusal')
    monkeypatch.setattr(_lib, 'load', boom)
    monkeypatch.setattr(eval_faiss, 'FlatL2Index', boom)
    monkeypatch.setattr(dup, 'match_library', boom)


def _refused(emb_dir, **kw):
    with pytest.raises(SystemExit) as e:
        dup.duplicates({}, 'name', '0', emb_dir=emb_dir, **kw)
    return str(e.value)


def test_refusals_fire_before_any_gpu_call(tmp_path, no_gpu):
    d = _library(tmp_path)
    msg = _refused(d, window=300, k_probe=32)
    assert '--window 300 x --k_probe 32' in msg and '8192' in msg
    assert '--k_probe' in _refused(d, k_probe=33) and '1..32' in _refused(d, k_probe=0)
    assert '--n_short' in _refused(d, n_short=257)
    assert '--window' in _refused(d, window=0)
    assert '--chunk_rows' in _refused(d, chunk_rows=0)
    assert '--min_coverage' in _refused(d, min_coverage=float('nan'))


def test_fewer_than_two_tracks_is_refused(tmp_path, no_gpu):
    assert 'two are needed' in _refused(_library(tmp_path, n_tracks=1))


def test_missing_files_are_refused_by_name(tmp_path, no_gpu):
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    (tmp_path / 'c').mkdir()
    msg = _refused(_library(tmp_path / 'a', tables=False))
    assert 'custom_source_tracks.json is missing' in msg and 'NAFP_TRACK_TABLE=1' in msg
    msg = _refused(str(tmp_path / 'b') + '/')                        # nothing there: the default library's first file is named
    assert 'dummy_db.mm is missing' in msg and 'generate' in msg
    d = _library(tmp_path / 'c')
    with open(d + 'custom_source_tracks.json', 'w') as f:            # a table that does not describe the rows
        json.dump({'files': ['t0.wav'], 'first': [0, 7], 'hop_s': 0.5, 'duration_s': 1.0}, f)
    assert 'NAFP_TRACK_TABLE=1' in _refused(d)


def test_the_command_is_an_extension_and_has_no_index_option():
    import run
    assert 'duplicates' in run.extensions.commands and 'duplicates' not in run.cli.commands
    opts = {o for p in run.extensions.commands['duplicates'].params for o in p.opts}
    assert '--index_type' not in opts and '-i' not in opts
    assert {'--window', '--window_hop', '--k_probe', '--min_overlap', '--min_votes', '--n_short', '--min_score', '--align_tol',
            '--min_coverage', '--chunk_rows', '--output', '--config'} <= opts
    assert 'no -i' in run.extensions.commands['duplicates'].help
