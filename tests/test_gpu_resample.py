"""GPU: the resampler (csrc/resample.hip) EQUALS the int64 restatement (tests/_resample_ref.py) built from the library's own
table -- every rate class, stereo, files shorter than the filter, the clamp, any cut into pieces -- and the two consumers
(generate: SegmentSource + StreamedEmbedder; train: PcmArena.device) deliver the same bytes as pre-converted 8 kHz files.
No tolerance anywhere."""
import copy
import ctypes
import json
import wave

import numpy as np
import pytest
import torch

import _resample_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = 0x5555


def _lib_table(nafp, fs):
    L, M, half, T = ref.geometry(fs)
    tab = np.zeros((L, T), np.int32)
    assert nafp._lib.load().nafp_resample_table_host(fs, 8000, tab.ctypes.data_as(ctypes.c_void_p)) == 0
    return tab


def _want(nafp, x, fs):
    return ref.resample(x, fs, tab=_lib_table(nafp, fs))


def _noise(n, ch=1, seed=0):
    x = np.random.default_rng(seed).integers(-32768, 32768, size=(n, ch)).astype(np.int16)
    return x[:, 0] if ch == 1 else x


def _layout(fs, files, cuts, order=None):
    """Pieces of `files` (int16 (n,) or (n, 2)) at rate fs: file i is cut at the output indices cuts[i]; every piece uploads
    only the frames it reads.  -> (raw arena, piece array, out size, [(file, out0, n_out, out_off)])."""
    from neural_audio_fp_amd.model.utils import resample as rs
    rows, raw, where, raw_pos, out_pos = [], [], [], 0, 0
    todo = []
    for i, x in enumerate(files):
        n_total = ref.n_out(len(x), fs)
        edges = [0] + sorted(c for c in set(cuts[i]) if 0 < c < n_total) + [n_total]
        todo += [(i, a, b) for a, b in zip(edges, edges[1:])] if n_total else [(i, 0, 0)]
    for i, a, b in (todo if order is None else [todo[k] for k in order(len(todo))]):
        x = files[i]
        ch = 1 if x.ndim == 1 else 2
        first, last = rs.input_range(a, b, len(x), fs, 8000)
        rows.append((raw_pos, first, last - first, len(x), a, out_pos, b - a, ch))
        chunk = np.zeros(((last - first) * ch + 7) // 8 * 8, np.int16)
        chunk[:(last - first) * ch] = x[first:last].reshape(-1)
        raw.append(chunk)
        where.append((i, a, b - a, out_pos))
        raw_pos += len(chunk)
        out_pos += (b - a + 7) // 8 * 8
    raw = np.concatenate(raw + [np.zeros(8, np.int16)])
    return raw, np.array(rows, dtype=rs.PIECE_DTYPE), out_pos + 8, where


def _run(fs, files, cuts, order=None):
    """-> (per-file outputs, the whole output arena); int16 outside the pieces must be left alone."""
    from neural_audio_fp_amd.model.utils import resample as rs
    raw, pieces, out_total, where = _layout(fs, files, cuts, order)
    out = torch.full((out_total,), SENTINEL, dtype=torch.int16, device='cuda')
    rs.plan_for(fs, 8000).run(torch.from_numpy(raw).cuda(), pieces, out)
    arena = out.cpu().numpy()
    got = [np.zeros(ref.n_out(len(x), fs), np.int16) for x in files]
    untouched = np.ones(out_total, bool)
    for i, a, n, off in where:
        got[i][a:a + n] = arena[off:off + n]
        untouched[off:off + n] = False
    assert np.all(arena[untouched] == SENTINEL)
    return got, arena


@pytest.mark.parametrize('fs', [44100, 48000, 11025, 16000])
def test_rates_mono(nafp, fs):
    """0.6 s of full-range noise: 4,800 outputs (at 44100 Hz: 60 passes over all 80 phases; 11025 Hz: L = 320, the largest
    table stride; 48000 / 16000 Hz: L = 1)."""
    x = _noise(int(0.6 * fs), seed=fs)
    (got,), _ = _run(fs, [x], [[]])
    assert len(got) == 4800 and np.array_equal(got, _want(nafp, x, fs))


def test_stereo(nafp):
    x = _noise(26460, 2, seed=3)                               # independent channels
    (got,), _ = _run(44100, [x], [[]])
    assert np.array_equal(got, _want(nafp, x, 44100))
    assert not np.array_equal(got, _want(nafp, x[:, 0], 44100))
    y = _noise(5000, 2, seed=4)                                # the model rate in stereo: the average only
    y[:4] = [[32767, 32767], [-32768, -32768], [32767, 32766], [-3, 2]]
    (got,), _ = _run(8000, [y], [[]])
    assert np.array_equal(got, ((y.astype(np.int64).sum(1) + 1) >> 1).astype(np.int16))
    assert np.array_equal(got, _want(nafp, y, 8000))


def test_edges_short_files_and_last_output(nafp):
    """Files shorter than the filter's half-width (185.7 frames at 44100 Hz), an empty file, and n_in * L a multiple of M
    (441 -> exactly 80 outputs) / one frame past it (442 -> 81)."""
    files = [_noise(n, seed=10 + n) for n in (0, 1, 50, 186, 441, 442)] + [_noise(50, 2, seed=9)]
    got, _ = _run(44100, files, [[] for _ in files])
    assert [len(g) for g in got] == [0, 1, 10, 34, 80, 81, 10]
    for g, x in zip(got, files):
        assert np.array_equal(g, _want(nafp, x, 44100))
    assert np.abs(got[1]).max() > 0
    files = [_noise(n, seed=20 + n) for n in (1, 5, 6, 7)]     # 48000 Hz: M = 6
    got, _ = _run(48000, files, [[] for _ in files])
    assert [len(g) for g in got] == [1, 1, 1, 2]
    for g, x in zip(got, files):
        assert np.array_equal(g, _want(nafp, x, 48000))


def test_clamp(nafp):
    """A full-scale square wave overshoots the int16 range behind the filter: the rails are reached."""
    n = np.arange(13230)
    x = np.where((n // 44) % 2 == 0, 32767, -32768).astype(np.int16)        # 501 Hz at 44100 Hz
    want = _want(nafp, x, 44100)
    assert ((want == 32767) | (want == -32768)).mean() >= 0.10              # else the input is wrong
    (got,), _ = _run(44100, [x], [[]])
    assert np.array_equal(got, want)
    xs = np.stack([x, x], axis=1)
    (got2,), _ = _run(44100, [xs], [[1000]])
    assert np.array_equal(got2, _want(nafp, xs, 44100)) and np.array_equal(got2, want)


def test_pieces_do_not_matter(nafp):
    x, other = _noise(15435, seed=31), _noise(9000, 2, seed=32)             # 2,800 and 1,633 outputs
    (one,), arena = _run(44100, [x], [[]])
    assert len(one) == 2800 and np.array_equal(one, _want(nafp, x, 44100))
    cuts = [1, 63, 64, 65, 255, 256, 257, 1023, 1025, 2047, 2049, 2799]
    (cut,), _ = _run(44100, [x], [cuts])
    assert cut.tobytes() == one.tobytes()
    # interleaved with the pieces of a second (stereo) file in one launch, in a shuffled order
    order = lambda n: np.random.default_rng(5).permutation(n)
    (mixed, mixed_other), a1 = _run(44100, [x, other], [cuts, [7, 700, 1200]], order)
    assert mixed.tobytes() == one.tobytes()
    assert np.array_equal(mixed_other, _want(nafp, other, 44100))
    (_, _), a2 = _run(44100, [x, other], [cuts, [7, 700, 1200]], order)     # the same launch again
    assert a1.tobytes() == a2.tobytes()


def test_inconsistent_pieces_are_refused(nafp):
    """A piece that points outside its raw range or the output arena: a status before the launch, nothing written; the device
    makes the same checks for a list it is handed directly (such a piece's outputs are zero, or untouched if they themselves
    lie outside), and the next valid call is right."""
    from neural_audio_fp_amd.model.utils import resample as rs
    lib = nafp._lib.load()
    x = _noise(4410, seed=41)
    raw, pieces, out_total, where = _layout(44100, [x], [[300]])
    d_raw = torch.from_numpy(raw).cuda()
    plan = rs.plan_for(44100, 8000)
    bad = {}
    for name, field, value in (('raw range', 'n_frames', pieces[1]['n_frames'] + len(raw)), ('raw offset', 'raw_off', len(raw) - 3),
                               ('output arena', 'out_off', out_total - 8), ('missing frames', 'frame0', pieces[0]['frame0'] + 1),
                               ('beyond the file', 'n_out', pieces[1]['n_out'] + 1), ('negative', 'out0', -1)):
        p = pieces.copy()
        p[field][1 if field != 'frame0' else 0] = value
        if name == 'missing frames':
            p['n_frames'][0] -= 1
        bad[name] = p
        out = torch.full((out_total,), SENTINEL, dtype=torch.int16, device='cuda')
        assert lib.nafp_resample_check_pieces_host(44100, 8000, p.ctypes.data_as(ctypes.c_void_p), len(p), len(raw), out_total) == 1, name
        with pytest.raises(nafp._lib.NafpError, match='invalid'):
            plan.run(d_raw, p, out)
        assert bool((out == SENTINEL).all()), name
    # the device's own checks, for a list that was not built on the host
    want = _want(nafp, x, 44100)
    for name in ('raw range', 'output arena'):
        p = bad[name]
        out = torch.full((out_total,), SENTINEL, dtype=torch.int16, device='cuda')
        d_p = torch.from_numpy(p.view(np.uint8).reshape(-1)).cuda()
        nafp._lib.check(lib.nafp_resample_i16(plan.handle, nafp._lib.ptr(d_raw), len(raw), nafp._lib.ptr(d_p), len(p), nafp._lib.ptr(out),
                                              out_total, nafp._lib.current_stream()), 'resample_i16')
        arena = out.cpu().numpy()
        assert np.array_equal(arena[:300], want[:300]), name                     # the consistent piece next to it
        n1 = int(pieces[1]['n_out']); off = int(pieces[1]['out_off'])
        tail = arena[off:off + n1]
        assert np.all(tail == (0 if name == 'raw range' else SENTINEL)), name
        assert np.all(arena[off + n1:] == SENTINEL) and np.all(arena[300:off] == SENTINEL), name
    out = torch.full((out_total,), SENTINEL, dtype=torch.int16, device='cuda')
    plan.run(d_raw, pieces, out)
    arena = out.cpu().numpy()
    assert np.array_equal(np.concatenate([arena[:300], arena[int(pieces[1]['out_off']):][:len(want) - 300]]), want)


def _write_wav(path, pcm, fs, channels=1):
    with wave.open(str(path), 'w') as w:
        w.setnchannels(channels); w.setsampwidth(2); w.setframerate(fs)
        w.writeframes(np.asarray(pcm).astype('<i2').tobytes())


def _music(n, fs, ch, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = np.stack([sum(5000 * np.sin(2 * np.pi * f * t + p) for f, p in zip(rng.uniform(200, 3000, 4), rng.uniform(0, 6, 4)))
                  + rng.integers(-3000, 3000, size=n) for _ in range(ch)], axis=1)
    return np.clip(x, -32768, 32767).astype(np.int16)


def test_generate_end_to_end(nafp, cfg, tmp_path, monkeypatch):
    """44.1 kHz stereo + 48 kHz mono through SegmentSource + StreamedEmbedder with the switch on, at two launch sizes and through
    generate_fingerprint itself, vs the restatement's output written as 8 kHz mono WAVs and generated as always: byte-identical."""
    from neural_audio_fp_amd.model import generate as g
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    c = copy.deepcopy(cfg)
    c['BSZ']['TS_BATCH_SZ'] = 5
    c['DIR']['LOG_ROOT_DIR'] = str(tmp_path) + '/logs/'
    c['DIR']['OUTPUT_ROOT_DIR'] = str(tmp_path) + '/logs/emb/'
    src_dir, conv_dir = tmp_path / 'src', tmp_path / 'conv'
    src_dir.mkdir(); conv_dir.mkdir()
    a, b = _music(6 * 44100, 44100, 2, seed=1), _music(int(3.2 * 48000), 48000, 1, seed=2)
    _write_wav(src_dir / 'a.wav', a.reshape(-1), 44100, 2)
    _write_wav(src_dir / 'b.wav', b.reshape(-1), 48000, 1)
    _write_wav(conv_dir / 'a.wav', _want(nafp, a, 44100), 8000)
    _write_wav(conv_dir / 'b.wav', _want(nafp, b[:, 0], 48000), 8000)
    m_pre, m_fp = g.build_fp(c)
    g.save_checkpoint(c['DIR']['LOG_ROOT_DIR'] + 'checkpoint/', 'exp', 3, m_fp)

    def run(paths, launch_rows):
        src = SegmentSource([str(p) for p in paths], bsz=5)
        arr = np.zeros((src.n_samples, 128), np.float32)
        g.write_fingerprints(src, g.StreamedEmbedder(m_pre, m_fp), arr, group=5, launch_rows=launch_rows)
        return arr

    monkeypatch.delenv('NAFP_RESAMPLE', raising=False)
    plain = run([conv_dir / 'a.wav', conv_dir / 'b.wav'], 10)
    assert plain.shape == (11 + 5, 128) and np.abs(plain).sum() > 0
    monkeypatch.setenv('NAFP_RESAMPLE', '1')
    small, large = run([src_dir / 'a.wav', src_dir / 'b.wav'], 5), run([src_dir / 'a.wav', src_dir / 'b.wav'], 15)
    assert small.tobytes() == plain.tobytes()
    assert large.tobytes() == plain.tobytes()
    g.generate_fingerprint(c, 'exp', None, str(src_dir), None, True)
    out_dir = c['DIR']['OUTPUT_ROOT_DIR'] + '/exp/3/'
    got = np.asarray(np.memmap(out_dir + 'custom_source.mm', dtype='float32', mode='r', shape=(16, 128)))
    assert got.tobytes() == plain.tobytes()
    rates = json.load(open(out_dir + 'source_rates.json'))['custom_source']
    assert rates == {'files': 2, 'resampled': 2, 'rates': {'44100x2': 1, '48000x1': 1}}


def test_train_arena(nafp, tmp_path, monkeypatch):
    """PcmArena.device() over a store of one 22.05 kHz and one 8 kHz file: the restatement / the file's own bytes at each
    file's `start`, zero padding between; the raw frames pass the staging buffer in several runs."""
    from neural_audio_fp_amd.model.utils.dataloader_keras import PcmStore, PcmArena
    monkeypatch.setenv('NAFP_RESAMPLE', '1')
    x, y = _noise(33075 + 13, seed=51), _noise(9001, seed=52)
    _write_wav(tmp_path / 'x.wav', x, 22050)
    _write_wav(tmp_path / 'y.wav', y, 8000)
    store = PcmStore([str(tmp_path / 'x.wav'), str(tmp_path / 'y.wav')], 8000, base=16)
    want_x = _want(nafp, x, 22050)
    assert list(store.n_frames) == [len(want_x), 9001] and list(store.start) == [16, 16 + (len(want_x) + 7) // 8 * 8]
    arena = PcmArena([store])
    want = np.zeros(arena.total, np.int16)
    want[16:16 + len(want_x)] = want_x
    want[store.start[1]:store.start[1] + 9001] = y
    got = arena.device(piece=1 << 14).cpu().numpy()
    assert got.tobytes() == want.tobytes()
    assert arena.device().cpu().numpy().tobytes() == want.tobytes()          # one run per file
    with pytest.raises(NotImplementedError):
        arena.host()
