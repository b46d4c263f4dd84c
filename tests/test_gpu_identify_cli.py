"""GPU: `run.py identify` end to end on a synthetic library -- `generate` with NAFP_TRACK_TABLE=1, recordings cut out of the
library's own files, and the matches the command reports.

Nothing is trained: the checkpoint is a freshly initialised model.  The expectations are derived, not measured.  The recordings
are excerpts cut at multiples of the hop, so their 1-s PCM windows are the library's windows; with FEAT 'melspec_maxnorm' (every
segment normalised by its own maximum, not by its batch's) a fingerprint depends on its window alone, so the recording's
fingerprints are the library's rows.  The true alignment of a window that lies inside its track then scores 1 to rounding, and
every other alignment strictly less (Cauchy-Schwarz on unit rows that differ).

The run sets `--min_score 0.999`: a window that lies inside its track scores at least 1 - (128 + 8 + 2) * 2^-24 - the rounding of the
row norms, far above it, and a window that holds a segment of other material (the joint of two tracks, the noise) cannot reach 1.
Without a threshold such a window still returns its best candidate -- on the first GPU run of this test the window across the joint
returned a 5-row overlap at the wrong offset with 0.965, because rows of one synthetic track resemble each other under untrained
weights and a short overlap is scored over fewer rows -- which is why the command reports scores and leaves the threshold to the
user."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, HOP = 8000, 4000


def _wav(path, pcm, fs=FS, channels=1):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, 'w') as w:
        w.setnchannels(channels); w.setsampwidth(2); w.setframerate(fs)
        w.writeframes(np.clip(pcm, -32768, 32767).astype('<i2').tobytes())


def _music(rng, n):
    """The generator of tests/test_gpu_pipeline.py."""
    t = np.arange(n) / 8000.0
    x = rng.integers(-1200, 1200, size=n).astype(np.float64)
    for f in rng.uniform(250, 3800, size=4):
        x += 5000 * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28)) * (0.5 + 0.5 * np.sin(2 * np.pi * rng.uniform(0.2, 2.0) * t))
    return x


def test_identify_cli(nafp, cfg, tmp_path, monkeypatch):
    import copy
    from neural_audio_fp_amd.model import generate as g
    rng = np.random.default_rng(2027)
    ds = str(tmp_path / 'dataset') + '/'
    pcm = lambda: np.clip(_music(rng, 20 * FS), -32768, 32767).astype('<i2')
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
    yaml.safe_dump(c, open(work / 'config' / 'tiny.yaml', 'w'))
    g.save_checkpoint(c['DIR']['LOG_ROOT_DIR'] + 'checkpoint/', 'EXP', 1, nafp.get_fingerprinter(c))
    emb = work / 'logs' / 'emb' / 'EXP' / '1'

    # the recordings: excerpts at multiples of the hop (0.5 s)
    rec = str(tmp_path / 'rec') + '/'
    first = db[1][10 * HOP:26 * HOP]                                  # 8 s from the middle of db track 1, from 5.0 s
    _wav(rec + 'a_middle.wav', first)
    _wav(rec + 'b_tail_then_noise.wav', np.concatenate([db[2][32 * HOP:], rng.integers(-6000, 6000, size=4 * FS)]))   # the last 4 s of track 2
    _wav(rec + 'c_two_tracks.wav', np.concatenate([db[0][4 * HOP:16 * HOP], db[2][20 * HOP:32 * HOP]]))   # 6 s from 2.0 s, then 6 s from 10.0 s
    up = np.interp(np.arange(int(len(first) * 44100 / FS)) * (FS / 44100), np.arange(len(first)), first.astype(np.float64))
    _wav(str(tmp_path / 'stereo') + '/a_middle_44k1_stereo.wav', np.repeat(np.round(up)[:, None], 2, 1).reshape(-1), fs=44100, channels=2)

    env = {k: v for k, v in os.environ.items() if not k.startswith('NAFP_INGEST') and k not in ('NAFP_RESAMPLE', 'NAFP_TRACK_TABLE')}
    env['PYTHONPATH'] = ROOT

    def identify(*args, **extra):
        return subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), 'identify', 'EXP', '1', *args, '-c', 'tiny', '-i', 'L2',
                               '--window', '8', '--window_hop', '4'], cwd=work, env=dict(env, **extra), capture_output=True, text=True, timeout=600)

    # without the variable `generate` writes no table, and `identify` says which variable writes one
    for k in ('NAFP_TRACK_TABLE', 'NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS', 'NAFP_INGEST_FLAC'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.chdir(work)
    g.generate_fingerprint(c, 'EXP', 1, None, None, False)
    assert not [f for f in os.listdir(emb) if f.endswith('_tracks.json')]
    r = identify(rec)
    assert r.returncode != 0 and 'NAFP_TRACK_TABLE=1' in r.stdout + r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    monkeypatch.setenv('NAFP_TRACK_TABLE', '1')
    monkeypatch.setenv('NAFP_OVERWRITE', '1')
    g.generate_fingerprint(c, 'EXP', 1, None, None, False)
    assert sorted(f for f in os.listdir(emb) if f.endswith('_tracks.json')) == ['db_tracks.json', 'dummy_db_tracks.json', 'query_tracks.json']
    assert json.load(open(emb / 'db_tracks.json'))['first'] == [0, 39, 78, 117]          # (the query files are a SegmentSource too)

    r = identify(rec, '--min_score', '0.999')
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout[-2500:])
    res = json.load(open(emb / 'identify.json'))
    assert res['index_type_used'].startswith('L2') and res['window'] == 8 and res['n_windows'] == 3 + 3 + 5
    by = {}
    for m in res['matches']:
        by.setdefault(os.path.basename(m['recording']), []).append(m)
    track = lambda i: f'{ds}music/test-query-db-500-30s/db/x/{i}.wav'
    # 8 s from the middle of db track 1: three windows, one alignment, one match
    (m,) = by['a_middle.wav']
    assert m['track'] == track(1) and m['track_position_s'] == 5.0 and m['recording_span_s'] == [0.0, 8.0] and m['windows'] == 3
    assert abs(m['score'] - 1.0) < 1e-5 and m['min_votes'] >= 7
    # the last 4 s of track 2, then noise: the first window runs past the end of the track and is scored over the 7 rows it shares
    # (overlap 7 of 8, score 1); the windows that hold noise stay below the threshold
    (m,) = by['b_tail_then_noise.wav']
    assert m['track'] == track(2) and m['track_position_s'] == 16.0 and m['recording_span_s'] == [0.0, 4.5] and abs(m['score'] - 1.0) < 1e-5
    # 6 s of track 0 then 6 s of track 2: two matches.  Segments 0 .. 10 are track 0, 11 straddles the joint, 12 .. 22 are track 2: the
    # windows at 0 and at 12, 16 are pure; those at 4 and 8 hold the joint and may or may not pass
    m0, m2 = by['c_two_tracks.wav']
    assert m0['track'] == track(0) and m0['track_position_s'] == 2.0 and m0['recording_span_s'][0] == 0.0 and m0['recording_span_s'][1] in (4.5, 6.5, 8.5)
    assert m2['track'] == track(2) and m2['track_position_s'] == 10.0 - 6.0 and m2['recording_span_s'][0] in (4.0, 6.0) and m2['recording_span_s'][1] == 12.0
    assert m0['windows'] >= 1 and m2['windows'] >= 2

    # the same excerpt as 16-bit stereo at 44.1 kHz: converted on the device (NAFP_INGEST_ANY=1), so not bit-equal: same track, +- one hop
    out = str(tmp_path / 'stereo.json')
    r = identify(str(tmp_path / 'stereo' / 'a_middle_44k1_stereo.wav'), '--output', out, NAFP_INGEST_ANY='1')
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ms = json.load(open(out))['matches']
    assert ms and all(m['track'] == track(1) and abs(m['track_position_s'] - 5.0) <= 0.5 for m in ms), ms
