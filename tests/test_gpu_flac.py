"""GPU: the FLAC pre-pass (csrc/flac.hip) writes the bytes and statuses of nafp_flac_decode_host -- the same functions compiled for
the host, themselves held to the writer's samples by tests/test_flac_host.py -- for every variant of the host grid in one launch,
for any cut of frames into launches and any order; corrupt frames are zeroed with a status and their neighbours untouched; and the
consumers (generate, the training arena) deliver for FLAC files the bytes they deliver for the same samples as PCM WAV.  No
tolerance anywhere."""
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
import _flac_ref as fr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p
CANARY = 0x5a


def _layout(nafp, streams, seed=0):
    """streams: [bytes].  Every stream's bytes go into one raw arena at odd offsets, every frame of its index gets a record whose
    output range starts 1 to 4 canary bytes behind the previous one (any alignment).  -> (raw, records, scratch size, owner of each
    record: (stream, frame))."""
    from neural_audio_fp_amd.model.utils import flac as fl
    raw_parts, rows, owner, raw_pos, out_pos = [], [], [], 0, 3
    for s, data in enumerate(streams):
        info, index = fl.scan(data)
        assert info['refusal'] == 0 and len(index)
        idx = fl.Index(index, info['channels'], info['bps'], info['rate'])
        raw_pos += 1 + s % 3
        raw_parts.append((raw_pos, data))
        for k in range(len(idx)):
            r, _, n_pcm = fl.records(idx, k, k + 1, raw_pos + int(idx.offset[k]), out_pos)
            rows.append(r)
            owner.append((s, k))
            out_pos += n_pcm + 1 + (len(rows) % 4)
        raw_pos += len(data)
    raw = np.random.default_rng(seed).integers(0, 256, size=raw_pos + 16, dtype=np.uint8)
    for at, data in raw_parts:
        raw[at:at + len(data)] = np.frombuffer(data, np.uint8)
    return raw, np.concatenate(rows), out_pos + 8, owner


def _host(nafp, raw, raw_size, rows, scratch_size, total=None):
    out = np.full(total or scratch_size, CANARY, np.uint8)
    status = np.full(len(rows), -1, np.int32)
    rows = np.ascontiguousarray(rows)
    assert nafp._lib.load().nafp_flac_decode_host(raw.ctypes.data_as(VP), raw_size, rows.ctypes.data_as(VP), len(rows), out.ctypes.data_as(VP),
                                                  scratch_size, status.ctypes.data_as(VP)) == 0
    return out, status


def _launch(nafp, d_raw, raw_size, rows, d_out, scratch_size, with_status=True):
    """The library entry point itself (no host-side record check in the way)."""
    d_rows = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy()).cuda()
    d_status = torch.full((len(rows),), -1, dtype=torch.int32, device='cuda') if with_status else None
    st = nafp._lib.load().nafp_flac_decode(nafp._lib.ptr(d_raw), raw_size, nafp._lib.ptr(d_rows), len(rows), nafp._lib.ptr(d_out), scratch_size,
                                           nafp._lib.ptr(d_status), nafp._lib.current_stream())
    assert st == 0
    torch.cuda.synchronize()
    return d_status.cpu().numpy() if with_status else None


def test_device_equals_host_in_one_mixed_launch(nafp):
    """Every variant of the host grid, all frames in ONE launch in a random order: scratch bytes (canary bytes between the frames
    included) and statuses equal the host's, and the frames hold the writer's samples."""
    grid = fr.variant_grid()
    raw, rows, size, owner = _layout(nafp, [g[1].data for g in grid])
    order = np.random.default_rng(1).permutation(len(rows))
    rows = rows[order]
    want, want_status = _host(nafp, raw, len(raw), rows, size)
    assert (want_status == 0).all()
    out = torch.full((size,), CANARY, dtype=torch.uint8, device='cuda')
    status = _launch(nafp, torch.from_numpy(raw).cuda(), len(raw), rows, out, size)
    got = out.cpu().numpy()
    assert np.array_equal(status, want_status)
    if not np.array_equal(got, want):
        bad = [grid[owner[order[i]][0]][0] for i, r in enumerate(rows) if not np.array_equal(
            got[r['scratch_off'] - 1:r['scratch_off'] + r['block_size'] * r['channels'] * 3 + 1],
            want[r['scratch_off'] - 1:r['scratch_off'] + r['block_size'] * r['channels'] * 3 + 1])]
        raise AssertionError(f'{len(bad)} frames differ, e.g. {bad[:5]}')
    for i, r in enumerate(rows):                              # the ground truth: the samples handed to the writer
        s, k = owner[order[i]]
        name, stream, x, bps = grid[s]
        first = sum(f[3] for f in stream.frames[:k])
        ref = fr.justified(x[first:first + int(r['block_size'])], bps)
        assert got[r['scratch_off']:r['scratch_off'] + len(ref)].tobytes() == ref.tobytes(), name
    assert (got == CANARY).sum() >= len(rows)


def test_launches_and_order_do_not_matter(nafp):
    """The frames of several files cut into launches of 1, 3 and all frames, permuted within a launch; launches without a status
    array too: every cut gives the same scratch bytes, and the canary bytes outside the frames' ranges stay."""
    grid = {g[0]: g for g in fr.variant_grid()}
    streams = [s.data for s in fr.golden_streams()] + [grid[n][1].data for n in ('short_last', 'lpc32', 'stereo10x24', 'depth20x5')]
    raw, rows, size, _ = _layout(nafp, streams, seed=2)
    want, _ = _host(nafp, raw, len(raw), rows, size)
    d_raw = torch.from_numpy(raw).cuda()
    rng = np.random.default_rng(3)
    taken = np.zeros(size, bool)
    for r in rows:
        taken[r['scratch_off']:r['scratch_off'] + r['block_size'] * r['channels'] * (2 if r['bps'] <= 16 else 3)] = True
    assert (~taken).sum() > len(rows) and (want[~taken] == CANARY).all()
    for per_launch in (1, 3, len(rows)):
        out = torch.full((size,), CANARY, dtype=torch.uint8, device='cuda')
        order = rng.permutation(len(rows))
        for a in range(0, len(rows), per_launch):
            _launch(nafp, d_raw, len(raw), rows[order[a:a + per_launch]], out, size, with_status=per_launch != 3)
        assert out.cpu().numpy().tobytes() == want.tobytes(), per_launch


def test_corrupt_frames_are_zeroed_and_their_neighbours_untouched(nafp):
    """A launch holds the valid frames of golden stream 0 next to the six named mutations of its frame 1 -- each run under the
    sanitizers by tools/flac_host_check.cpp first, same definitions -- and a record that states no range of the scratch arena.
    raw_size / scratch_size are passed SMALLER than the tensors allocated, so every access stays inside allocated memory whatever
    the kernel does and the check is read from the bytes."""
    from neural_audio_fp_amd.model.utils import flac as fl
    stream = fr.golden_streams()[0]
    x = fr.music(16 * 6, 8000, 2, 16, 1, .9)
    mutations = fr.named_mutations(stream)
    names = list(mutations)
    raw, rows, size, owner = _layout(nafp, [stream.data] + [mutations[n][0] for n in names], seed=4)
    keep, kinds = [], []
    for i, (s, k) in enumerate(owner):
        if s == 0 or k == 1:                                  # the valid stream whole, frame 1 of every mutated copy
            keep.append(i)
            kinds.append(None if s == 0 else names[s - 1])
    rows = rows[keep].copy()
    raw_size = len(raw)
    for i, name in enumerate(kinds):
        for field, value in (mutations[name][1] if name else {}).items():
            # (the inconsistent record: its frame ends one byte past the raw arena, wherever the arena ends)
            rows[i][field] = raw_size - stream.frames[1][1] + 1 if field == 'raw_off' else value
    nowhere = rows[0].copy()
    nowhere['scratch_off'] = size - 1
    rows = np.concatenate([rows, nowhere[None]])
    kinds.append('no_range')
    raw = np.concatenate([raw, np.random.default_rng(5).integers(0, 256, size=1 << 16, dtype=np.uint8)])
    total = size + (1 << 16)
    want, want_status = _host(nafp, raw, raw_size, rows, size, total)
    out = torch.full((total,), CANARY, dtype=torch.uint8, device='cuda')
    status = _launch(nafp, torch.from_numpy(raw).cuda(), raw_size, rows, out, size)
    got = out.cpu().numpy()
    assert np.array_equal(status, want_status) and got.tobytes() == want.tobytes()
    assert (got[size:] == CANARY).all()
    for r, kind, st in zip(rows, kinds, status):
        lo, n = int(r['scratch_off']), int(r['block_size']) * 4
        if kind is None:
            assert st == 0
        elif kind == 'no_range':
            assert st == 8 and (got[lo:size] == CANARY).all()
        else:
            assert st != 0 and not got[lo:lo + n].any(), kind
            assert got[lo - 1] == CANARY and got[lo + n] == CANARY
    valid = [i for i, kind in enumerate(kinds) if kind is None]
    assert len(valid) == 6
    for k, i in enumerate(valid):                             # the valid frames: the writer's samples
        lo = int(rows[i]['scratch_off'])
        assert got[lo:lo + 64].tobytes() == fr.justified(x[16 * k:16 * k + 16], 16).tobytes()
    assert fl.FRAME_DTYPE.itemsize == 40


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


def _clear(monkeypatch):
    for env in ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS', 'NAFP_INGEST_FLAC'):
        monkeypatch.delenv(env, raising=False)


@pytest.mark.parametrize('fs_in,ch,bps,block,fs_out', [(44100, 2, 16, 4096, 8000), (48000, 1, 24, 1152, 8000), (11025, 1, 16, 576, 16000)])
def test_rate_conversion_equals_the_ingest_of_the_pcm_wav(nafp, tmp_path, monkeypatch, fs_in, ch, bps, block, fs_out):
    """FLAC file -> pre-pass -> nafp_ingest_i16 == nafp_ingest_i16 on the PCM WAV written from the source samples."""
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    x = fr.music(int(2.7 * fs_in), fs_in, ch, bps, seed=bps + ch)
    sub = fr.lpc_recipe(x[:, 0], 4, 12, porder=2, method=1 if bps > 16 else 0)
    (tmp_path / 'x.flac').write_bytes(fr.write_stream(x, bps, fs_in, block=block, sub=sub, frames=None).data)
    (tmp_path / 'y.wav').write_bytes(fr.pcm_wav(x, bps, fs_in))
    _clear(monkeypatch)
    monkeypatch.setenv('NAFP_INGEST_FLAC', '1')
    src = SegmentSource([str(tmp_path / 'x.flac')], bsz=4, fs=fs_out)
    got = _windows(src, 3)
    assert src.flac_failed.count() == 0
    monkeypatch.delenv('NAFP_INGEST_FLAC')
    monkeypatch.setenv('NAFP_INGEST_ANY', '1')
    want = _windows(SegmentSource([str(tmp_path / 'y.wav')], bsz=4, fs=fs_out), 3)
    assert got.shape == want.shape and got.shape[0] >= 4 and np.abs(want.astype(int)).max() > 3000
    assert got.tobytes() == want.tobytes()


def test_eight_khz_mono_16_bit_is_the_identity(nafp, tmp_path, monkeypatch):
    """An 8 kHz mono 16-bit FLAC file through the pre-pass and the ingest (never "native"): the segments hold the writer's samples,
    as those of the same samples in a plain WAV do."""
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource, file_segments
    x = fr.music(26500, 8000, 1, 16, seed=3)
    (tmp_path / 'x.flac').write_bytes(fr.write_stream(x, 16, 8000, block=1152, sub={'type': 'fixed', 'order': 2, 'porder': 3}).data)
    (tmp_path / 'y.wav').write_bytes(fr.pcm_wav(x, 16, 8000))
    _clear(monkeypatch)
    plain = SegmentSource([str(tmp_path / 'y.wav')], bsz=4)
    want = file_segments(x[:, 0].astype(np.int16), 8000, 1., .5)
    assert np.array_equal(plain.read_rows(0, plain.n_samples)[:, 0], want)
    monkeypatch.setenv('NAFP_INGEST_FLAC', '1')
    src = SegmentSource([str(tmp_path / 'x.flac')], bsz=4)
    assert src.resampled == [True] and src.n_frames == [26500] and np.abs(want.astype(int)).max() > 3000
    for rows in (2, 100):
        assert np.array_equal(_windows(src, rows), want)


def _tree(src_dir, conv_dir):
    """PCM and codec WAVs next to FLAC files of two depths, mono and stereo, two rates, one with a corrupted frame; `conv_dir`: the
    same tree converted beforehand to PCM WAV (the corrupted frame as zeros)."""
    import wave
    native = cref.music(17000, 8000, 1, 77).astype('<i2')
    for d in (src_dir, conv_dir):
        with wave.open(str(d / 'a.wav'), 'w') as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(8000)
            w.writeframes(native.tobytes())
    body = cref.encode('alaw', cref.music(2 * 16000, 16000, 2, 5), 2, 2)
    (src_dir / 'b.wav').write_bytes(cref.wav_bytes('alaw', body, 16000, 2, 2))
    (conv_dir / 'b.wav').write_bytes(cref.pcm16_wav(cref.decode_file('alaw', 2, 2, body, len(body) // 2), 16000, 2))
    for name, fs, ch, bps, block, seconds, corrupt in (('c', 8000, 1, 16, 1152, 2.3, None), ('d', 48000, 2, 24, 4096, 2.1, None),
                                                       ('e', 44100, 2, 16, 4096, 2.4, 11), ('f', 8000, 1, 24, 576, 2.2, None)):
        x = fr.music(int(seconds * fs), fs, ch, bps, seed=ord(name))
        stream = fr.write_stream(x, bps, fs, block=block, sub=fr.lpc_recipe(x[:, 0], 6, 12, porder=3, method=1 if bps > 16 else 0))
        data = bytearray(stream.data)
        if corrupt is not None:                              # one bit of one frame's body: its CRC-16 fails, the frame is zeros
            off, nb, first, size = stream.frames[corrupt]
            data[off + nb // 2] ^= 0x04
            x = x.copy()
            x[corrupt * block:corrupt * block + size] = 0
        (src_dir / f'{name}.flac').write_bytes(bytes(data))
        (conv_dir / f'{name}.wav').write_bytes(fr.pcm_wav(x, bps, fs))
    return ['a.wav', 'b.wav', 'c.flac', 'd.flac', 'e.flac', 'f.flac']


def test_generate_end_to_end(nafp, cfg, tmp_path, monkeypatch):
    """`run.py generate -s DIR` with NAFP_INGEST_FLAC=1 on a tree mixing PCM and codec WAVs with FLAC files vs the same tree
    converted beforehand to PCM WAV and generated with NAFP_INGEST_ANY=1: the .mm files are byte-identical, at two launch sizes
    too; the corrupted frame is converted as zeros; source_rates.json names the classes and counts the failed frame once."""
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
    m_pre, m_fp = g.build_fp(c)
    g.save_checkpoint(c['DIR']['LOG_ROOT_DIR'] + 'checkpoint/', 'exp', 3, m_fp)

    def run(files, launch_rows):
        src = SegmentSource(files, bsz=5)
        arr = np.zeros((src.n_samples, 128), np.float32)
        g.write_fingerprints(src, g.StreamedEmbedder(m_pre, m_fp), arr, group=5, launch_rows=launch_rows)
        return arr, src

    _clear(monkeypatch)
    monkeypatch.setenv('NAFP_INGEST_ANY', '1')
    plain, _ = run([str(conv_dir / (n[:2] + 'wav')) for n in names], 10)
    assert plain.shape[0] == 3 + 3 + 3 + 3 + 3 + 3 and np.abs(plain).sum() > 0
    monkeypatch.delenv('NAFP_INGEST_ANY')
    monkeypatch.setenv('NAFP_INGEST_FLAC', '1')
    for rows in (5, 15):
        got, src = run([str(src_dir / n) for n in names], rows)
        assert got.tobytes() == plain.tobytes(), rows
        assert src.flac_failed.count() == 1, rows            # a frame that two launches decode is still one frame
    env = {k: v for k, v in os.environ.items() if k not in ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS')}
    env['NAFP_INGEST_FLAC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), 'generate', 'exp', '-c', 'tiny', '-s', str(src_dir), '--skip_dummy'],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert '5 of 6 files are decoded' in r.stdout and '4 FLAC files, 1 frames failed their checks' in r.stdout
    out_dir = c['DIR']['OUTPUT_ROOT_DIR'] + '/exp/3/'
    got = np.asarray(np.memmap(out_dir + 'custom_source.mm', dtype='float32', mode='r', shape=plain.shape))
    assert got.tobytes() == plain.tobytes()
    rates = json.load(open(out_dir + 'source_rates.json'))['custom_source']
    assert rates == {'files': 6, 'resampled': 5, 'flac_files': 4, 'flac_failed_frames': 1,
                     'rates': {'8000x1xs16': 1, '16000x2xalaw': 1, '8000x1xflac16': 1, '48000x2xflac24': 1, '44100x2xflac16': 1,
                               '8000x1xflac24': 1}}


def test_train_arena(nafp, tmp_path, monkeypatch):
    """PcmArena.device() of the mixed tree == that of the converted tree (NAFP_INGEST_ANY=1), also when the frames pass the staging
    buffer in several runs; the failed frame is counted once; .host() raises."""
    from neural_audio_fp_amd.model.utils.dataloader_keras import PcmStore, PcmArena
    src_dir, conv_dir = tmp_path / 'src', tmp_path / 'conv'
    src_dir.mkdir(); conv_dir.mkdir()
    names = _tree(src_dir, conv_dir)
    _clear(monkeypatch)
    monkeypatch.setenv('NAFP_INGEST_ANY', '1')
    conv = PcmStore([str(conv_dir / (n[:2] + 'wav')) for n in names], 8000, base=16)
    want = PcmArena([conv]).device().cpu().numpy()
    monkeypatch.delenv('NAFP_INGEST_ANY')
    monkeypatch.setenv('NAFP_INGEST_FLAC', '1')
    for piece in (1 << 25, 1 << 16):                         # the second: several runs per file
        store = PcmStore([str(src_dir / n) for n in names], 8000, base=16)
        assert list(store.n_frames) == list(conv.n_frames) and list(store.start) == list(conv.start)
        assert store.format == ['s16', 'alaw', 'flac16', 'flac24', 'flac16', 'flac24']
        arena = PcmArena([store])
        assert arena.device(piece=piece).cpu().numpy().tobytes() == want.tobytes(), piece
        assert arena.flac_failed_frames() == 1, piece
    assert np.abs(want.astype(int)).max() > 3000
    with pytest.raises(NotImplementedError):
        arena.host()
