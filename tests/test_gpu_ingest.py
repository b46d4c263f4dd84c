"""GPU: the general ingest (csrc/ingest.hip) EQUALS the integer restatement (tests/_ingest_ref.py) run on the library's own
table -- every sample format and channel count, byte offsets of any alignment, both directions of rate conversion, files shorter
than the filter, the clamp, any cut into pieces or launches -- equals nafp_resample_i16 where both serve, and the two consumers
(generate: SegmentSource + StreamedEmbedder through the command line; train: PcmArena.device) deliver the same bytes as files
converted beforehand to 16-bit mono at the model rate.  No tolerance anywhere."""
import copy
import ctypes
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import _ingest_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5555
FORMATS = list(ref.FORMATS)
_TABLES = {}


def _lib_table(nafp, fs_in, fs_out):
    if (fs_in, fs_out) not in _TABLES:
        L, M, half, T = ref.geometry(fs_in, fs_out)
        tab = np.zeros((L, T), np.int32)
        assert nafp._lib.load().nafp_ingest_table_host(fs_in, fs_out, tab.ctypes.data_as(ctypes.c_void_p)) == 0
        _TABLES[fs_in, fs_out] = tab
    return _TABLES[fs_in, fs_out]


def _want(nafp, f, fs_in, fs_out):
    fmt, body, ch = f
    return ref.ingest(fmt, body, ch, fs_in, fs_out, tab=_lib_table(nafp, fs_in, fs_out))


def _file(fmt, n, ch, seed=0, scale=1.0):
    """Full-range noise in every channel (independent channels), as a file body."""
    q = np.random.default_rng(seed).integers(-2 ** 23, 2 ** 23, size=n * ch)
    return fmt, ref.encode(fmt, (q * scale).astype(np.int64)), ch


def _n_frames(f):
    return len(f[1]) // (f[2] * ref.FORMATS[f[0]][1])


def _layout(fs_in, fs_out, files, cuts, odd=lambda fmt: fmt in ('u8', 's24'), order=None):
    """Pieces of `files` ((fmt, body, channels)): file i is cut at the output indices cuts[i]; every piece uploads only the
    bytes of the frames it reads, at a 16-byte boundary + 1 where odd(fmt).  -> (raw bytes, piece array, out size, [(file, out0,
    n_out, out_off)])."""
    from neural_audio_fp_amd.model.utils import ingest as ig
    rows, chunks, where, raw_pos, out_pos, todo = [], [], [], 0, 0, []
    for i, f in enumerate(files):
        n_total = ref.n_out(_n_frames(f), fs_in, fs_out)
        edges = [0] + sorted(c for c in set(cuts[i]) if 0 < c < n_total) + [n_total]
        todo += [(i, a, b) for a, b in zip(edges, edges[1:])] if n_total else [(i, 0, 0)]
    for i, a, b in (todo if order is None else [todo[k] for k in order(len(todo))]):
        fmt, body, ch = files[i]
        align = ch * ref.FORMATS[fmt][1]
        first, last = ig.input_range(a, b, _n_frames(files[i]), fs_in, fs_out)
        raw_pos = (raw_pos + 15) // 16 * 16 + (1 if odd(fmt) else 0)
        rows.append((raw_pos, first, last - first, _n_frames(files[i]), a, out_pos, b - a, ch, ref.FORMATS[fmt][0], 0))
        chunks.append((raw_pos, body[first * align:last * align]))
        where.append((i, a, b - a, out_pos))
        raw_pos += (last - first) * align
        out_pos += (b - a + 7) // 8 * 8
    raw = np.full(raw_pos + 16, 0xA5, np.uint8)
    for pos, data in chunks:
        raw[pos:pos + len(data)] = np.frombuffer(data, np.uint8)
    return raw, np.array(rows, dtype=ig.PIECE_DTYPE), out_pos + 8, where


def _run(fs_in, fs_out, files, cuts, launches=1, **kw):
    """-> (per-file outputs, the whole output arena); int16 outside the pieces must be left alone.  launches > 1: the pieces go
    in that many separate launches into the same arena."""
    from neural_audio_fp_amd.model.utils import ingest as ig
    raw, pieces, out_total, where = _layout(fs_in, fs_out, files, cuts, **kw)
    out = torch.full((out_total,), SENTINEL, dtype=torch.int16, device='cuda')
    d_raw = torch.from_numpy(raw).cuda()
    for part in np.array_split(np.arange(len(pieces)), launches):
        ig.plan_for(fs_in, fs_out).run(d_raw, pieces[part], out)
    arena = out.cpu().numpy()
    got = [np.zeros(ref.n_out(_n_frames(f), fs_in, fs_out), np.int16) for f in files]
    untouched = np.ones(out_total, bool)
    for i, a, n, off in where:
        got[i][a:a + n] = arena[off:off + n]
        untouched[off:off + n] = False
    assert np.all(arena[untouched] == SENTINEL)
    return got, arena


@pytest.mark.parametrize('fs_in', [44100, 8000])
def test_every_format_and_channel_count(nafp, fs_in):
    """6 formats x {1, 2, 3, 6, 8} channels in one launch, 300 .. 3000 frames each, at 44100 -> 8000 and at the identity rate.
    The byte-wide and 24-bit formats sit at odd byte offsets; at the identity rate EVERY format does (the wider ones are then
    read byte by byte), at 44100 Hz the wider ones are naturally aligned (one load per sample)."""
    files = [_file(fmt, 300 + 140 * (3 * i + j), ch, seed=10 * i + j) for i, fmt in enumerate(FORMATS) for j, ch in enumerate((1, 2, 3, 6, 8))]
    odd = (lambda fmt: True) if fs_in == 8000 else (lambda fmt: fmt in ('u8', 's24'))
    got, _ = _run(fs_in, 8000, files, [[] for _ in files], odd=odd)
    for g, f in zip(got, files):
        want = _want(nafp, f, fs_in, 8000)
        assert len(g) == len(want) > 0 and np.array_equal(g, want), (f[0], f[2])
        assert np.abs(want.astype(int)).max() > 1000
    if fs_in == 8000:                                          # the identity: the rounded channel mean of the canonical samples
        fmt, body, ch = files[7]                               # s16 x 3
        x = np.frombuffer(body, '<i2').astype(np.int64).reshape(-1, 3).sum(1)
        assert np.array_equal(got[7], np.floor((2 * x + 3) / 6.0).astype(np.int16))
        assert np.array_equal(got[5], np.frombuffer(files[5][1], '<i2'))       # s16 x 1: the samples themselves


@pytest.mark.parametrize('fs_in,fs_out', [(4000, 8000), (8000, 16000), (11025, 16000), (6000, 8000)])
def test_upsampling(nafp, fs_in, fs_out):
    files = [_file('s16', 3000, 1, seed=1), _file('s24', 1777, 2, seed=2), _file('f32', 901, 3, seed=3), _file('u8', 300, 1, seed=4)]
    got, _ = _run(fs_in, fs_out, files, [[], [1000], [], []])
    for g, f in zip(got, files):
        want = _want(nafp, f, fs_in, fs_out)
        assert len(g) == -(-_n_frames(f) * fs_out // fs_in) and np.array_equal(g, want), f[0]


@pytest.mark.parametrize('fs_in,fs_out', [(44100, 8000), (4000, 8000), (11025, 16000)])
def test_edges_short_files_last_output_and_block_boundary(nafp, fs_in, fs_out):
    """Files of 0, 1, 2 and T M / L -+ 1 frames (the filter's length in input frames); the last output of each; pieces of 255,
    256 and 257 outputs (one block less one, one block, one block and one output) starting mid-file."""
    L, M, half, T = ref.geometry(fs_in, fs_out)
    k = T * M // L
    files = [_file(fmt, n, ch, seed=n) for n, fmt, ch in ((0, 's24', 2), (1, 's16', 1), (2, 'f32', 3), (k - 1, 's24', 1), (k + 1, 'u8', 2),
                                                         (1, 'f64', 8), (2, 's32', 1))]
    long = _file('s24', -(-1100 * M // L) + 5, 3, seed=99)                # >= 1,100 outputs: the frames that many need
    cuts = [[] for _ in files] + [[300, 300 + 255, 300 + 255 + 256, 300 + 255 + 256 + 257]]
    got, _ = _run(fs_in, fs_out, files + [long], cuts)
    assert [len(g) for g in got[:3]] == [0, -(-L // M), -(-2 * L // M)]
    for g, f in zip(got, files + [long]):
        want = _want(nafp, f, fs_in, fs_out)
        assert len(g) == len(want) and np.array_equal(g, want), (f[0], _n_frames(f))
    assert np.abs(got[1].astype(int)).max() > 0 and len(got[-1]) >= 1100


def test_clamp(nafp):
    """Full-scale square waves of the same sign in every channel overshoot behind the filter: the rails are reached, in both
    directions of conversion, from +-1.0 floats (1.0 itself clamps to 2^23 - 1) and from the 24-bit extremes."""
    Q = 2 ** 23
    n = np.arange(13230)
    sq = np.where((n // 44) % 2 == 0, 1, -1)                               # 501 Hz at 44100 Hz
    f32 = ('f32', np.repeat(sq.astype('<f4'), 3).tobytes(), 3)
    s24 = ('s24', ref.encode('s24', np.repeat(np.where(sq > 0, Q - 1, -Q), 2)), 2)
    got, _ = _run(44100, 8000, [f32, s24], [[], [1000]])
    for g, f in zip(got, (f32, s24)):
        want = _want(nafp, f, 44100, 8000)
        assert ((want == 32767) | (want == -32768)).mean() >= 0.10          # else the input is wrong
        assert np.array_equal(g, want)
    sq = np.where((np.arange(3000) // 5) % 2 == 0, 1.0, -1.0)              # 400 Hz at 4000 Hz
    f64 = ('f64', np.repeat(sq.astype('<f8'), 8).tobytes(), 8)
    (g,), _ = _run(4000, 8000, [f64], [[]])
    want = _want(nafp, f64, 4000, 8000)
    assert ((want == 32767) | (want == -32768)).mean() >= 0.10 and np.array_equal(g, want)


def test_pieces_and_launches_do_not_matter(nafp):
    x, other = _file('s24', 15435, 3, seed=31), _file('f32', 9000, 2, seed=32)       # 2,800 and 1,633 outputs
    (one,), _ = _run(44100, 8000, [x], [[]])
    assert len(one) == 2800 and np.array_equal(one, _want(nafp, x, 44100, 8000))
    two, seven = [1400], [1, 255, 256, 1023, 2049, 2799]
    for cuts in (two, seven):
        (cut,), _ = _run(44100, 8000, [x], [cuts])
        assert cut.tobytes() == one.tobytes()
    (cut,), _ = _run(44100, 8000, [x], [seven], launches=3)
    assert cut.tobytes() == one.tobytes()
    # interleaved with the pieces of a second file in one launch, in a shuffled order; and the same launch again
    order = lambda n: np.random.default_rng(5).permutation(n)
    (mixed, mixed_other), a1 = _run(44100, 8000, [x, other], [seven, [7, 700, 1200]], order=order)
    assert mixed.tobytes() == one.tobytes()
    assert np.array_equal(mixed_other, _want(nafp, other, 44100, 8000))
    (_, _), a2 = _run(44100, 8000, [x, other], [seven, [7, 700, 1200]], order=order)
    assert a1.tobytes() == a2.tobytes()
    # upsampling: the same
    y = _file('s16', 2000, 2, seed=33)
    (one,), _ = _run(11025, 16000, [y], [[]])
    (cut,), _ = _run(11025, 16000, [y], [[1, 255, 511, 512, 2000, 2901]], launches=2)
    assert len(one) == 2903 and cut.tobytes() == one.tobytes() == _want(nafp, y, 11025, 16000).tobytes()


@pytest.mark.parametrize('fs_in', [44100, 8000])
@pytest.mark.parametrize('ch', [1, 2])
def test_sixteen_bit_equals_the_resampler(nafp, fs_in, ch):
    """The one class of files both kernels serve: nafp_ingest_i16 writes what nafp_resample_i16 writes, byte for byte."""
    from neural_audio_fp_amd.model.utils import resample as rs
    x = np.random.default_rng(7 + ch).integers(-32768, 32768, size=(2999, ch)).astype(np.int16)
    x[:4] = [[32767] * ch, [-32768] * ch, [32767] + [32766] * (ch - 1), [-3] + [2] * (ch - 1)]
    n_out = rs.n_out(len(x), fs_in, 8000)
    old = torch.full((n_out + 8,), SENTINEL, dtype=torch.int16, device='cuda')
    piece = np.array([(0, 0, len(x), len(x), 0, 0, n_out, ch)], dtype=rs.PIECE_DTYPE)
    rs.plan_for(fs_in, 8000).run(torch.from_numpy(x.reshape(-1)).cuda(), piece, old)
    (new,), _ = _run(fs_in, 8000, [('s16', x.astype('<i2').tobytes(), ch)], [[]])
    assert new.tobytes() == old.cpu().numpy()[:n_out].tobytes()
    assert np.array_equal(new, _want(nafp, ('s16', x.astype('<i2').tobytes(), ch), fs_in, 8000))


def _write_native(path, pcm, fs=8000):
    with wave.open(str(path), 'w') as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(fs)
        w.writeframes(np.asarray(pcm).astype('<i2').tobytes())


def _music(fmt, n, fs, ch, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = np.stack([sum(0.15 * np.sin(2 * np.pi * f * t + p) for f, p in zip(rng.uniform(200, 0.4 * min(fs, 8000), 4), rng.uniform(0, 6, 4)))
                  + rng.uniform(-0.1, 0.1, size=n) for _ in range(ch)], axis=1)
    return fmt, ref.encode(fmt, np.rint(x.reshape(-1) * 2 ** 23).astype(np.int64)), ch


def test_generate_end_to_end(nafp, cfg, tmp_path, monkeypatch):
    """`run.py generate -s DIR` with NAFP_INGEST_ANY=1 on a tree of mixed formats, channel counts and rates (up and down) vs the
    same tree converted beforehand by the restatement to 16-bit mono 8 kHz and generated as always: the .mm files are
    byte-identical, at two more launch sizes too, and source_rates.json names the formats."""
    import yaml
    from neural_audio_fp_amd.model import generate as g
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    c = copy.deepcopy(cfg)
    c['BSZ']['TS_BATCH_SZ'] = 5
    c['DIR']['LOG_ROOT_DIR'] = str(tmp_path) + '/logs/'
    c['DIR']['OUTPUT_ROOT_DIR'] = str(tmp_path) + '/logs/emb/'
    (tmp_path / 'config').mkdir()
    yaml.safe_dump(c, open(tmp_path / 'config' / 'tiny.yaml', 'w'))
    src_dir, conv_dir = tmp_path / 'src', tmp_path / 'conv'
    src_dir.mkdir(); conv_dir.mkdir()
    tree = [('a', 48000, True, _music('s24', int(3.1 * 48000), 48000, 2, 1)), ('b', 44100, False, _music('f32', 2 * 44100, 44100, 1, 2)),
            ('c', 6000, False, _music('s16', 4 * 6000, 6000, 1, 3)), ('d', 8000, False, _music('u8', 20000, 8000, 1, 4)),
            ('e', 8000, False, _music('s16', 17000, 8000, 1, 5)), ('f', 4000, True, _music('f64', 9000, 4000, 6, 6))]
    for name, fs, ext, f in tree:
        (src_dir / f'{name}.wav').write_bytes(ref.wav_bytes(f[0], f[1], fs, f[2], extensible=ext))
        _write_native(conv_dir / f'{name}.wav', _want(nafp, f, fs, 8000))
    paths = lambda d: [str(d / f'{name}.wav') for name, *_ in tree]
    m_pre, m_fp = g.build_fp(c)
    g.save_checkpoint(c['DIR']['LOG_ROOT_DIR'] + 'checkpoint/', 'exp', 3, m_fp)

    def run(files, launch_rows):
        src = SegmentSource(files, bsz=5)
        arr = np.zeros((src.n_samples, 128), np.float32)
        g.write_fingerprints(src, g.StreamedEmbedder(m_pre, m_fp), arr, group=5, launch_rows=launch_rows)
        return arr

    monkeypatch.delenv('NAFP_RESAMPLE', raising=False)
    monkeypatch.delenv('NAFP_INGEST_ANY', raising=False)
    plain = run(paths(conv_dir), 10)
    assert plain.shape == (5 + 3 + 7 + 4 + 3 + 3, 128) and np.abs(plain).sum() > 0
    monkeypatch.setenv('NAFP_INGEST_ANY', '1')
    small, large = run(paths(src_dir), 5), run(paths(src_dir), 15)
    assert small.tobytes() == plain.tobytes()
    assert large.tobytes() == plain.tobytes()
    env = dict(os.environ, NAFP_INGEST_ANY='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), 'generate', 'exp', '-c', 'tiny', '-s', str(src_dir), '--skip_dummy'],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert '5 of 6 files are decoded' in r.stdout
    out_dir = c['DIR']['OUTPUT_ROOT_DIR'] + '/exp/3/'
    got = np.asarray(np.memmap(out_dir + 'custom_source.mm', dtype='float32', mode='r', shape=plain.shape))
    assert got.tobytes() == plain.tobytes()
    rates = json.load(open(out_dir + 'source_rates.json'))['custom_source']
    assert rates == {'files': 6, 'resampled': 5, 'rates': {'48000x2xs24': 1, '44100x1xf32': 1, '6000x1xs16': 1, '8000x1xu8': 1,
                                                          '8000x1xs16': 1, '4000x6xf64': 1}}


def test_train_arena(nafp, tmp_path, monkeypatch):
    """PcmArena.device() over a store of one 24-bit stereo 22.05 kHz file and one native file: the restatement / the file's own
    bytes at each file's `start`, zero padding between; the raw bytes pass the staging buffer in several runs.  .host() raises."""
    from neural_audio_fp_amd.model.utils.dataloader_keras import PcmStore, PcmArena
    monkeypatch.setenv('NAFP_INGEST_ANY', '1')
    x = _file('s24', 33075 + 13, 2, seed=51)
    y = np.random.default_rng(52).integers(-32768, 32768, size=9001).astype(np.int16)
    (tmp_path / 'x.wav').write_bytes(ref.wav_bytes('s24', x[1], 22050, 2, extensible=True))
    _write_native(tmp_path / 'y.wav', y)
    store = PcmStore([str(tmp_path / 'x.wav'), str(tmp_path / 'y.wav')], 8000, base=16)
    want_x = _want(nafp, x, 22050, 8000)
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
