"""GPU: the codec pre-pass (csrc/codec.hip) writes the bytes of nafp_codec_decode_host -- the same function compiled for the
host, itself held to the numpy restatement by tests/test_codec_host.py -- for every codec, channel count and block size, piece
sizes around the workgroup's block group, odd byte and sample offsets, any cut into pieces or launches; inconsistent pieces are
zeroed or left alone as the contract says; and the two consumers (generate, the training arena) deliver for codec files the bytes
they deliver for the same files converted beforehand to 16-bit PCM by the restatement.  No tolerance anywhere."""
import copy
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _codec_ref as cref
import _ingest_ref as iref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5555
GRID = [(codec, ch, ch) for codec in ('alaw', 'ulaw') for ch in (1, 2, 3, 8)] + \
       [(codec, ch, align) for codec in ('ima4', 'ms4') for ch in (1, 2) for align in (8, 9, 16, 37, 256, 512, 1024, 2048, 4096)
        if cref.samples_per_block(codec, ch, align) > 0]


def _host_decode(nafp, codec, ch, align, data):
    spb = cref.samples_per_block(codec, ch, align)
    n_blocks = len(data) // align
    buf = np.ascontiguousarray(data)
    out = np.zeros(max(n_blocks * spb * ch, 1), np.int16)
    assert nafp._lib.load().nafp_codec_decode_host(cref.CODECS[codec], ch, align, buf.ctypes.data_as(ctypes.c_void_p), n_blocks,
                                                   out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out[:n_blocks * spb * ch]


def _layout(nafp, items, seed=0):
    """items: (codec, channels, block_align, uint8 bytes of whole blocks).  Pieces at byte offsets that are 0, 1, 4 and 7 past a
    16-byte boundary in turn (the three staging widths) and at int16 offsets of alternating parity, 3 or 4 guard samples apart.
    -> (raw, piece array, expected arena)."""
    dt = np.dtype(nafp._lib.CODEC_PIECE_DTYPE)
    rows, chunks, raw_pos, out_pos = [], [], 0, 5
    for i, (codec, ch, align, data) in enumerate(items):
        spb = cref.samples_per_block(codec, ch, align)
        n_blocks = len(data) // align
        raw_pos = (raw_pos + 15) // 16 * 16 + (0, 1, 4, 7)[i % 4]
        rows.append((raw_pos, n_blocks, out_pos, cref.CODECS[codec], ch, align, spb))
        chunks.append((raw_pos, out_pos, data, _host_decode(nafp, codec, ch, align, data)))
        raw_pos += len(data)
        out_pos += n_blocks * spb * ch + 3 + (i % 2)
    raw = np.random.default_rng(seed).integers(0, 256, size=raw_pos + 16, dtype=np.uint8)
    want = np.full(out_pos + 8, SENTINEL, np.int16)
    for rp, op, data, pcm in chunks:
        raw[rp:rp + len(data)] = data
        want[op:op + len(pcm)] = pcm
    return raw, np.array(rows, dtype=dt), want


def _launch(nafp, d_raw, raw_size, pieces, d_out, out_samples):
    """The library entry point itself (no host-side piece check in the way)."""
    d_p = torch.from_numpy(pieces.view(np.uint8).reshape(-1).copy()).cuda()
    st = nafp._lib.load().nafp_codec_decode_i16(nafp._lib.ptr(d_raw), raw_size, nafp._lib.ptr(d_p), len(pieces), nafp._lib.ptr(d_out),
                                                out_samples, nafp._lib.current_stream())
    assert st == 0
    torch.cuda.synchronize()


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


def test_device_equals_host_in_one_mixed_launch(nafp):
    """Every (codec, channels, block_align) of the grid x n_blocks = 0, 1, one less and one more than the workgroup's block group
    and about 1000, random bytes, ALL IN ONE LAUNCH; the whole output arena, guards included, equals the host's."""
    lib = nafp._lib.load()
    items = []
    for k, (codec, ch, align) in enumerate(GRID):
        group = lib.nafp_codec_blocks_per_group(cref.CODECS[codec], ch, align)
        assert group >= 1
        for n_blocks in (0, 1, group - 1, group + 1, 1000 + k):
            items.append((codec, ch, align, _noise(n_blocks * align, 100 * k + n_blocks % 97)))
    order = np.random.default_rng(1).permutation(len(items))
    raw, pieces, want = _layout(nafp, [items[i] for i in order])
    assert lib.nafp_codec_check_pieces_host(pieces.ctypes.data_as(ctypes.c_void_p), len(pieces), len(raw), len(want)) == 0
    out = torch.full((len(want),), SENTINEL, dtype=torch.int16, device='cuda')
    _launch(nafp, torch.from_numpy(raw).cuda(), len(raw), pieces, out, len(want))
    got = out.cpu().numpy()
    if not np.array_equal(got, want):
        bad = [tuple(p) for p in pieces if not np.array_equal(got[p['out_off'] - 3:p['out_off'] + p['n_blocks'] * p['spb'] * p['channels'] + 3],
                                                               want[p['out_off'] - 3:p['out_off'] + p['n_blocks'] * p['spb'] * p['channels'] + 3])]
        raise AssertionError(f'{len(bad)} pieces differ, e.g. {bad[:5]}')
    assert (want == 32767).any() and (want == -32768).any()


@pytest.mark.parametrize('case', ['raw_past_end', 'out_past_end', 'spb', 'codec_0', 'adpcm_3_channels'])
def test_inconsistent_piece(nafp, case):
    """Three pieces, the middle one inconsistent.  raw_size / out_samples are passed SMALLER than the tensors allocated, so every
    access stays inside allocated memory whatever the kernel does and the check is read from the bytes: the piece's stated output
    range is zeroed (left untouched where it leaves the arena), everything past the stated sizes is untouched, the neighbours
    are decoded."""
    a = ('ima4', 2, 256, _noise(7 * 256, 1))
    b = ('ms4', 1, 512, _noise(60 * 512, 2))
    c = ('ulaw', 2, 2, _noise(5001 * 2, 3))
    raw, pieces, want = _layout(nafp, [a, b, c])
    raw_size, out_samples = len(raw), len(want)
    raw = np.concatenate([raw, _noise(1 << 16, 4)])
    want = np.concatenate([want, np.full(1 << 17, SENTINEL, np.int16)])
    p = pieces[1]
    lo, n = int(p['out_off']), int(p['n_blocks'] * p['spb'] * p['channels'])
    if case == 'raw_past_end':              # its last block ends one byte past raw_size
        pieces[1]['raw_off'] = raw_size - 60 * 512 + 1
        want[lo:lo + n] = 0
    elif case == 'out_past_end':            # its last sample is one past out_samples: nothing is written
        pieces[1]['out_off'] = out_samples - n + 1
        want[lo:lo + n] = SENTINEL
    elif case == 'spb':                     # states one frame per block too few: the range it states is zeroed, no more
        stated = int(p['spb']) - 1
        pieces[1]['spb'] = stated
        want[lo:lo + n] = SENTINEL
        want[lo:lo + 60 * stated] = 0
    elif case == 'codec_0':
        pieces[1]['codec'] = 0
        want[lo:lo + n] = 0
    else:                                   # 3 channels are no ADPCM geometry; 20 blocks x 3 channels state the same range
        pieces[1]['channels'], pieces[1]['n_blocks'] = 3, 20
        want[lo:lo + n] = 0
    assert nafp._lib.load().nafp_codec_check_pieces_host(pieces.ctypes.data_as(ctypes.c_void_p), 3, raw_size, out_samples) in (1, 2)
    out = torch.full((len(want),), SENTINEL, dtype=torch.int16, device='cuda')
    _launch(nafp, torch.from_numpy(raw).cuda(), raw_size, pieces, out, out_samples)
    got = out.cpu().numpy()
    assert np.array_equal(got[out_samples:], want[out_samples:])
    assert np.array_equal(got, want)
    assert np.abs(got[:lo].astype(int)).max() > 1000 and (got[lo + n + 8:out_samples - 8] != SENTINEL).any()


def test_pieces_and_launches_do_not_matter(nafp):
    """The same four files cut into different pieces and split over 1, 2 and 5 launches: the same bytes per file."""
    files = [('ima4', 2, 1024, _noise(140 * 1024, 11)), ('ms4', 2, 256, _noise(333 * 256, 12)), ('alaw', 3, 3, _noise(9001 * 3, 13)),
             ('ima4', 1, 4096, _noise(9 * 4096, 14))]
    whole = [_host_decode(nafp, *f) for f in files]
    rng = np.random.default_rng(15)
    for launches, n_cuts in ((1, 0), (1, 6), (2, 3), (5, 9)):
        items, owner = [], []
        for i, (codec, ch, align, data) in enumerate(files):
            n_blocks = len(data) // align
            cuts = sorted(set([0, n_blocks] + list(rng.integers(0, n_blocks + 1, size=n_cuts))))
            for lo, hi in zip(cuts, cuts[1:]):
                items.append((codec, ch, align, data[lo * align:hi * align]))
                owner.append((i, lo))
        order = rng.permutation(len(items))
        raw, pieces, want = _layout(nafp, [items[k] for k in order], seed=launches)
        out = torch.full((len(want),), SENTINEL, dtype=torch.int16, device='cuda')
        d_raw = torch.from_numpy(raw).cuda()
        for part in np.array_split(np.arange(len(pieces)), launches):
            _launch(nafp, d_raw, len(raw), pieces[part], out, len(want))
        got = out.cpu().numpy()
        assert np.array_equal(got, want)
        back = [np.zeros_like(w) for w in whole]
        for p, k in zip(pieces, order):
            i, lo = owner[k]
            per = int(p['spb'] * p['channels'])
            back[i][lo * per:(lo + int(p['n_blocks'])) * per] = got[p['out_off']:p['out_off'] + int(p['n_blocks']) * per]
        for b, w in zip(back, whole):
            assert b.tobytes() == w.tobytes()


def _codec_file(codec, ch, align, fs, seconds, seed, fact=None):
    """(wav bytes, the file's frames (n, ch) int16 by the restatement)."""
    spb = cref.samples_per_block(codec, ch, align)
    body = cref.encode(codec, cref.music(int(seconds * fs), fs, ch, seed), ch, align)
    n_frames = fact if fact is not None else len(body) // align * spb
    return cref.wav_bytes(codec, body, fs, ch, align, fact=fact), cref.decode_file(codec, ch, align, body, n_frames)


def _windows(src, rows_per_launch):
    """Every segment of a SegmentSource through iter_windows and the launch's device work: (n_samples, seg_len) int16."""
    out = np.zeros((src.n_samples, src.seg_len), np.int16)
    for start, n, arena, used, off, valid, *work in src.iter_windows(0, src.n_samples, rows_per_launch):
        pcm = torch.from_numpy(arena[:max(used, 1)]).cuda()
        if work and work[0] is not None:
            pcm = work[0].run(pcm)
        pcm = pcm.cpu().numpy()
        for i in range(n):
            out[start + i, :valid[i]] = pcm[off[i]:off[i] + valid[i]]
    return out


@pytest.mark.parametrize('codec,align', [('alaw', 1), ('ulaw', 1), ('ima4', 256), ('ms4', 512)])
def test_eight_khz_mono_is_the_identity(nafp, tmp_path, monkeypatch, codec, align):
    """A codec file at 8 kHz mono through the pre-pass and the ingest (never "native"): the segments hold the restatement-decoded
    PCM itself -- the ingest's identity geometry copies it."""
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource, file_segments
    monkeypatch.setenv('NAFP_INGEST_CODECS', '1')
    spb = cref.samples_per_block(codec, 1, align)
    data, pcm = _codec_file(codec, 1, align, 8000, 3.3, seed=3, fact=None if spb == 1 else 26000 // spb * spb - spb // 2)
    (tmp_path / 'x.wav').write_bytes(data)
    src = SegmentSource([str(tmp_path / 'x.wav')], bsz=4)
    assert src.resampled == [True] and src.n_frames == [len(pcm)] and np.abs(pcm.astype(int)).max() > 3000
    want = file_segments(pcm[:, 0], 8000, 1., .5)
    for rows in (2, 100):
        assert np.array_equal(_windows(src, rows), want)


@pytest.mark.parametrize('codec,ch,align,fs_in,fs_out', [('ima4', 2, 1024, 22050, 8000), ('ms4', 1, 256, 11025, 16000)])
def test_rate_conversion_equals_the_ingest_of_the_decoded_pcm(nafp, tmp_path, monkeypatch, codec, ch, align, fs_in, fs_out):
    """Codec file -> pre-pass -> nafp_ingest_i16 == nafp_ingest_i16 on the restatement-decoded 16-bit PCM of the same file."""
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    data, pcm = _codec_file(codec, ch, align, fs_in, 2.7, seed=5)
    (tmp_path / 'x.wav').write_bytes(data)
    (tmp_path / 'y.wav').write_bytes(cref.pcm16_wav(pcm, fs_in, ch))
    monkeypatch.setenv('NAFP_INGEST_CODECS', '1')
    got = _windows(SegmentSource([str(tmp_path / 'x.wav')], bsz=4, fs=fs_out), 3)
    monkeypatch.delenv('NAFP_INGEST_CODECS')
    monkeypatch.setenv('NAFP_INGEST_ANY', '1')
    want = _windows(SegmentSource([str(tmp_path / 'y.wav')], bsz=4, fs=fs_out), 3)
    assert got.shape == want.shape and got.shape[0] >= 4 and np.abs(want.astype(int)).max() > 3000
    assert got.tobytes() == want.tobytes()


def _tree(src_dir, conv_dir):
    """Native files next to all four codecs at several rates and channel counts; `conv_dir`: the same tree converted to 16-bit PCM
    (same rate, same channels) by the restatement.  One file's fact count ends mid-block."""
    import wave
    tree = [('a', 'alaw', 1, 1, 8000, 2.2, None), ('b', 'ulaw', 2, 2, 16000, 2.0, None), ('c', 'ima4', 2, 1024, 22050, 2.6, None),
            ('d', 'ima4', 1, 256, 8000, 2.3, 17000), ('e', 'ms4', 1, 256, 11025, 2.1, None), ('f', 'ms4', 2, 2048, 44100, 2.4, None)]
    names = []
    for name, codec, ch, align, fs, seconds, fact in tree:
        data, pcm = _codec_file(codec, ch, align, fs, seconds, seed=ord(name), fact=fact)
        (src_dir / f'{name}.wav').write_bytes(data)
        (conv_dir / f'{name}.wav').write_bytes(cref.pcm16_wav(pcm, fs, ch))
        names.append(name)
    native = cref.music(17000, 8000, 1, 77).astype('<i2')
    s24 = iref.wav_bytes('s24', iref.encode('s24', cref.music(2 * 48000, 48000, 2, 78).reshape(-1) * 256), 48000, 2, extensible=True)
    for d in (src_dir, conv_dir):
        with wave.open(str(d / 'g.wav'), 'w') as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(8000)
            w.writeframes(native.tobytes())
        (d / 'h.wav').write_bytes(s24)
    return names + ['g', 'h']


def test_generate_end_to_end(nafp, cfg, tmp_path, monkeypatch):
    """`run.py generate -s DIR` with NAFP_INGEST_CODECS=1 on a tree mixing native files with all four codecs vs the same tree
    converted beforehand to 16-bit PCM by the restatement and generated with NAFP_INGEST_ANY=1: the .mm files are byte-identical,
    at two launch sizes too; source_rates.json names the codecs."""
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
    names = _tree(src_dir, conv_dir)
    paths = lambda d: [str(d / f'{name}.wav') for name in names]
    m_pre, m_fp = g.build_fp(c)
    g.save_checkpoint(c['DIR']['LOG_ROOT_DIR'] + 'checkpoint/', 'exp', 3, m_fp)

    def run(files, launch_rows):
        src = SegmentSource(files, bsz=5)
        arr = np.zeros((src.n_samples, 128), np.float32)
        g.write_fingerprints(src, g.StreamedEmbedder(m_pre, m_fp), arr, group=5, launch_rows=launch_rows)
        return arr

    for env in ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS'):
        monkeypatch.delenv(env, raising=False)
    monkeypatch.setenv('NAFP_INGEST_ANY', '1')
    plain = run(paths(conv_dir), 10)
    assert plain.shape[0] == 3 + 3 + 4 + 3 + 3 + 3 + 3 + 3 and np.abs(plain).sum() > 0
    monkeypatch.delenv('NAFP_INGEST_ANY')
    monkeypatch.setenv('NAFP_INGEST_CODECS', '1')
    small, large = run(paths(src_dir), 5), run(paths(src_dir), 15)
    assert small.tobytes() == plain.tobytes()
    assert large.tobytes() == plain.tobytes()
    env = {k: v for k, v in os.environ.items() if k not in ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY')}
    env['NAFP_INGEST_CODECS'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), 'generate', 'exp', '-c', 'tiny', '-s', str(src_dir), '--skip_dummy'],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert '7 of 8 files are decoded' in r.stdout
    out_dir = c['DIR']['OUTPUT_ROOT_DIR'] + '/exp/3/'
    got = np.asarray(np.memmap(out_dir + 'custom_source.mm', dtype='float32', mode='r', shape=plain.shape))
    assert got.tobytes() == plain.tobytes()
    rates = json.load(open(out_dir + 'source_rates.json'))['custom_source']
    assert rates == {'files': 8, 'resampled': 7, 'rates': {'8000x1xalaw': 1, '16000x2xulaw': 1, '22050x2xima4': 1, '8000x1xima4': 1,
                                                          '11025x1xms4': 1, '44100x2xms4': 1, '8000x1xs16': 1, '48000x2xs24': 1}}


def test_train_arena(nafp, tmp_path, monkeypatch):
    """PcmArena.device() of the codec tree == that of the converted tree (NAFP_INGEST_ANY=1), also when the blocks pass the staging
    buffer in several runs; .host() raises."""
    from neural_audio_fp_amd.model.utils.dataloader_keras import PcmStore, PcmArena
    src_dir, conv_dir = tmp_path / 'src', tmp_path / 'conv'
    src_dir.mkdir(); conv_dir.mkdir()
    names = _tree(src_dir, conv_dir)
    for env in ('NAFP_RESAMPLE', 'NAFP_INGEST_CODECS'):
        monkeypatch.delenv(env, raising=False)
    monkeypatch.setenv('NAFP_INGEST_ANY', '1')
    conv = PcmStore([str(conv_dir / f'{n}.wav') for n in names], 8000, base=16)
    want = PcmArena([conv]).device().cpu().numpy()
    monkeypatch.delenv('NAFP_INGEST_ANY')
    monkeypatch.setenv('NAFP_INGEST_CODECS', '1')
    store = PcmStore([str(src_dir / f'{n}.wav') for n in names], 8000, base=16)
    assert list(store.n_frames) == list(conv.n_frames) and list(store.start) == list(conv.start)
    assert store.format[:6] == ['alaw', 'ulaw', 'ima4', 'ima4', 'ms4', 'ms4'] and store.n_in[3] == 17000
    arena = PcmArena([store])
    assert np.abs(want.astype(int)).max() > 3000
    assert arena.device().cpu().numpy().tobytes() == want.tobytes()
    assert arena.device(piece=1 << 15).cpu().numpy().tobytes() == want.tobytes()      # several runs per file
    with pytest.raises(NotImplementedError):
        arena.host()
