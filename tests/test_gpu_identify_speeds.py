"""GPU: speed hypotheses end to end -- the fingerprints of `SegmentSource(step=...)` against files converted beforehand by the numpy
restatements, and `run.py identify --speeds` on the library of tests/test_gpu_identify_cli.py with a recording played 4 % fast.

Nothing is trained: the model is freshly initialised, FEAT is 'melspec_maxnorm' (a fingerprint depends on its own window alone).  The
in-process part is bit equality: the device's varispeed bytes are the restatement's, so the fingerprints of a file under a step are
those of the restatement's output written as a WAV.  The command-line part asserts comparisons, not thresholds: on the CPU oracle
the hypothesis 1.04 scored 0.996 at the true position against 0.857 (hypothesis 1) and 0.838 (0.96) anywhere."""
import copy
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import yaml

import _ingest_ref as iref
import _varispeed_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, HOP = 8000, 4000
ONE = 1 << 24


def _wav(path, pcm, fs=FS, channels=1):
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    with wave.open(str(path), 'w') as w:
        w.setnchannels(channels); w.setsampwidth(2); w.setframerate(fs)
        w.writeframes(np.clip(pcm, -32768, 32767).astype('<i2').tobytes())


def _music(rng, n, fs=8000.0):
    """The generator of tests/test_gpu_identify_cli.py."""
    t = np.arange(n) / fs
    x = rng.integers(-1200, 1200, size=n).astype(np.float64)
    for f in rng.uniform(250, 3800, size=4):
        x += 5000 * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28)) * (0.5 + 0.5 * np.sin(2 * np.pi * rng.uniform(0.2, 2.0) * t))
    return x


def test_fingerprints_under_a_step(nafp, cfg, tmp_path, monkeypatch):
    """A native 8 kHz file and a 44.1 kHz stereo file (NAFP_INGEST_ANY=1) at the steps for 1.04 and 0.96, launch sizes 7 and 64:
    byte-identical to the fingerprints of WAVs converted beforehand by _ingest_ref, then _varispeed_ref."""
    from neural_audio_fp_amd.model import generate as g
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    for k in ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS', 'NAFP_INGEST_FLAC'):
        monkeypatch.delenv(k, raising=False)
    c = copy.deepcopy(cfg)
    c['MODEL']['FEAT'] = 'melspec_maxnorm'
    m_pre, m_fp = g.build_fp(c)
    rng = np.random.default_rng(31)
    native = np.clip(_music(rng, 9 * FS + 123), -32768, 32767).astype(np.int16)
    stereo = np.clip(np.stack([_music(rng, 7 * 44100 + 77, 44100.0) for _ in range(2)], axis=1), -32768, 32767).astype(np.int16)
    _wav(tmp_path / 'src' / 'native.wav', native)
    _wav(tmp_path / 'src' / 'stereo.wav', stereo.reshape(-1), fs=44100, channels=2)
    stereo_8k = iref.ingest('s16', stereo.astype('<i2').tobytes(), 2, 44100, FS)

    def run(paths, launch_rows, step=None):
        src = SegmentSource([str(p) for p in paths], bsz=1, step=step)
        arr = np.zeros((src.n_samples, int(c['MODEL']['EMB_SZ'])), np.float32)
        g.write_fingerprints(src, g.StreamedEmbedder(m_pre, m_fp), arr, group=1, launch_rows=launch_rows)
        return arr

    for speed in (1.04, 0.96):
        step = ref.step_for(speed)
        conv = tmp_path / f'conv{speed}'
        _wav(conv / 'native.wav', ref.varispeed(native, step))
        _wav(conv / 'stereo.wav', ref.varispeed(stereo_8k, step))
        monkeypatch.delenv('NAFP_INGEST_ANY', raising=False)
        want_native = run([conv / 'native.wav'], 64)
        want_both = run([conv / 'stereo.wav', conv / 'native.wav'], 64)
        assert np.abs(want_native).sum() > 0 and len(want_native) == len(run([tmp_path / 'src' / 'native.wav'], 64, step))
        for launch_rows in (7, 64):
            monkeypatch.delenv('NAFP_INGEST_ANY', raising=False)
            assert run([tmp_path / 'src' / 'native.wav'], launch_rows, step).tobytes() == want_native.tobytes(), (speed, launch_rows)
            monkeypatch.setenv('NAFP_INGEST_ANY', '1')
            got = run([tmp_path / 'src' / 'stereo.wav', tmp_path / 'src' / 'native.wav'], launch_rows, step)
            assert got.tobytes() == want_both.tobytes(), (speed, launch_rows)


def _play_faster(x, speed):
    """x played `speed` times as fast, by a float64 Kaiser-windowed sinc of this test's own (40 zero crossings a side, cut-off at
    0.45 of the lower rate): y[n] = sum_j x[j] h(n speed - j)."""
    x = np.asarray(x, np.float64)
    f2 = 0.9 / max(speed, 1.0)
    half = int(np.ceil(40 / f2))
    n = np.arange(int(len(x) / speed))
    t = n * float(speed)
    j0 = np.floor(t).astype(np.int64)
    k = np.arange(-half + 1, half + 1)
    u = (t - j0)[:, None] - k[None, :]
    h = f2 * np.sinc(f2 * u) * np.i0(9.0 * np.sqrt(np.maximum(0.0, 1.0 - (u / half) ** 2))) / np.i0(9.0)
    xp = np.concatenate([np.zeros(half), x, np.zeros(half + 1)])
    return np.round(np.sum(h * xp[(j0[:, None] + k[None, :]) + half], axis=1))


def test_identify_speeds_cli(nafp, cfg, tmp_path, monkeypatch):
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
    for k in ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS', 'NAFP_INGEST_FLAC'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('NAFP_TRACK_TABLE', '1')
    monkeypatch.chdir(work)
    g.generate_fingerprint(c, 'EXP', 1, None, None, False)

    # the recording: the 8-s excerpt from 5.0 s of db track 1, played 4 % fast; and the same with the speed undone by the restatement
    fast = np.clip(_play_faster(db[1][10 * HOP:26 * HOP], 1.04), -32768, 32767).astype(np.int16)
    step = ref.step_for(1.04)
    rec, undone = str(tmp_path / 'rec' / 'fast.wav'), str(tmp_path / 'undone' / 'fast.wav')
    _wav(rec, fast)
    _wav(undone, ref.varispeed(fast, step))

    env = {k: v for k, v in os.environ.items() if not k.startswith('NAFP_INGEST') and k not in ('NAFP_RESAMPLE', 'NAFP_TRACK_TABLE')}
    env['PYTHONPATH'] = ROOT

    def identify(path, out, *args):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), 'identify', 'EXP', '1', path, '-c', 'tiny', '-i', 'L2', '--window', '8',
                            '--window_hop', '4', '--output', out, *args], cwd=work, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        print(r.stdout[-1500:])
        return json.load(open(out)), r.stdout

    track1 = f'{ds}music/test-query-db-500-30s/db/x/1.wav'
    res, text = identify(rec, str(tmp_path / 'three.json'), '--speeds', '0.96,1,1.04')
    assert res['speeds'] == [ONE / round(ONE / 0.96), 1.0, ONE / round(ONE / 1.04)]
    (m,) = res['matches']
    assert m['track'] == track1 and m['speed'] == ONE / round(ONE / 1.04) and m['track_position_s'] == 5.0
    assert abs(m['recording_span_s'][0] - 0.0) <= 0.5 and abs(m['recording_span_s'][1] - 8 / 1.04) <= 0.5
    s096, s1, s104 = (row[0] for row in res['speed_best_scores'])
    print(f'best window scores: 0.96 -> {s096}, 1 -> {s1}, 1.04 -> {s104}')
    assert s104 > s1 and s104 > s096
    header = lambda out: next(ln for ln in out.splitlines() if ln.startswith('recording '))
    assert header(text).endswith(' speed')

    # --speeds 1.04 alone is the plain run on the file converted beforehand: same match, scores bit-equal
    one, _ = identify(rec, str(tmp_path / 'one.json'), '--speeds', '1.04')
    plain, plain_text = identify(undone, str(tmp_path / 'plain.json'))
    (a,), (b,) = one['matches'], plain['matches']
    assert a['speed'] == m['speed'] and a == m
    for key in ('track', 'track_index', 'track_position_s', 'score', 'min_votes', 'windows'):
        assert a[key] == b[key], key
    assert a['recording_span_s'] == [v * step / ONE for v in b['recording_span_s']]
    assert one['speed_best_scores'] == [[s104]]
    # without --speeds: none of the new keys, and no speed column
    assert 'speeds' not in plain and 'speed_best_scores' not in plain and 'speed' not in b
    assert 'speed' not in header(plain_text)
