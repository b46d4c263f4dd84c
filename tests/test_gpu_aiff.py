"""GPU: what NAFP_INGEST_AIFF=1 adds on the device.  The ingest kernel (csrc/ingest.hip) on big-endian and signed 8-bit pieces
writes the bytes it writes for the byte-reversed little-endian twin in the same launch, and the restatement's; the codec pre-pass
(csrc/codec.hip) on Apple IMA4 packets writes the bytes of nafp_codec_decode_host -- the same function compiled for the host, held
to the numpy restatement and to `audioop` by tests/test_aiff_host.py -- for piece sizes around the workgroup's block group, odd
offsets, any cut into pieces or launches, next to the four older codecs, whose bytes do not move; inconsistent pieces are zeroed
or left alone as the contract says; and the consumers (SegmentSource, `generate`, the training arena, `identify`) deliver for
AIFF / AIFF-C / AU files the bytes they deliver for the PCM WAV twin of each file (tests/_aiff_ref.to_wav).  No tolerance anywhere."""
import copy
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _aiff_ref as aref
import _codec_ref as cref
import _flac_ref as fr
import _ingest_ref as iref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5555
SWITCHES = ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS', 'NAFP_INGEST_FLAC', 'NAFP_INGEST_AIFF')
QT = 6


def _clear(monkeypatch):
    for k in SWITCHES + ('NAFP_TRACK_TABLE',):
        monkeypatch.delenv(k, raising=False)


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


# ---- the ingest kernel: big-endian == byte-reversed little-endian ---------------------------------------------------------------
@pytest.mark.parametrize('fs_in,fs_out', [(44100, 8000), (11025, 16000)])
def test_big_endian_equals_reversed_little_endian(nafp, fs_in, fs_out):
    """One launch: every new code x {1, 2, 3, 8} channels, about 1,000 outputs a piece, each next to its little-endian twin (for s8
    the u8 file of x + 128), once at a 16-byte boundary (one load per sample where the width allows) and once a byte past it (byte
    by byte: both paths of ig_load).  The twins' output ranges are byte-identical and equal the restatement on the library's table."""
    from neural_audio_fp_amd.model.utils import ingest as ig
    L, M, half, T = iref.geometry(fs_in, fs_out)
    tab = np.zeros((L, T), np.int32)
    assert nafp._lib.load().nafp_ingest_table_host(fs_in, fs_out, tab.ctypes.data_as(ctypes.c_void_p)) == 0
    n_frames = -(-1000 * M // L) + 3
    n_out = iref.n_out(n_frames, fs_in, fs_out)
    rows, chunks, want, raw_pos, out_pos = [], [], [], 0, 3
    for k, (fmt, (code, width, le)) in enumerate(aref.FORMATS.items()):
        for ch in (1, 2, 3, 8):
            body = _noise(n_frames * ch * width, 10 * k + ch).tobytes()
            if fmt in ('f32be', 'f64be'):                        # random bytes are mostly huge or tiny floats: audio-range values
                body = aref.encode(fmt, np.random.default_rng(10 * k + ch).integers(-2 ** 23, 2 ** 23, size=n_frames * ch))
            twin = aref.reverse(body, width) if le else bytes((b + 128) & 255 for b in body)
            twin_code = iref.FORMATS[le or 'u8'][0]
            y = iref.ingest(le or 'u8', twin, ch, fs_in, fs_out, tab=tab)
            assert np.array_equal(aref.decode(fmt, body), iref.decode(le or 'u8', twin)) and len(y) == n_out
            for skew in (0, 1):
                for data, c in ((body, code), (twin, twin_code)):
                    raw_pos = (raw_pos + 15) // 16 * 16 + skew
                    rows.append((raw_pos, 0, n_frames, n_frames, 0, out_pos, n_out, ch, c, 0))
                    chunks.append((raw_pos, data))
                    want.append((out_pos, y, fmt, ch, skew))
                    raw_pos += len(data)
                    out_pos += n_out + 5
    raw = np.full(raw_pos + 16, 0xA5, np.uint8)
    for pos, data in chunks:
        raw[pos:pos + len(data)] = np.frombuffer(data, np.uint8)
    pieces = np.array(rows, dtype=ig.PIECE_DTYPE)
    out = torch.full((out_pos + 8,), SENTINEL, dtype=torch.int16, device='cuda')
    ig.plan_for(fs_in, fs_out).run(torch.from_numpy(raw).cuda(), pieces, out)
    got = out.cpu().numpy()
    expect = np.full(len(got), SENTINEL, np.int16)
    for pos, y, *_ in want:
        expect[pos:pos + len(y)] = y
    for (pos, y, fmt, ch, skew), (pos2, *_) in zip(want[0::2], want[1::2]):
        assert got[pos:pos + n_out].tobytes() == got[pos2:pos2 + n_out].tobytes(), (fmt, ch, skew)
        assert np.array_equal(got[pos:pos + n_out], y), (fmt, ch, skew)
    assert np.array_equal(got, expect)                           # the guards too
    assert all(np.abs(y.astype(int)).max() > 1000 for _, y, *_ in want)


# ---- the codec pre-pass: Apple IMA4 ------------------------------------------------------------------------------------------
def _spb(codec, ch, align):
    return aref.QT_SPB if codec == 'qtima4' else cref.samples_per_block(codec, ch, align)


def _code(codec):
    return QT if codec == 'qtima4' else cref.CODECS[codec]


def _host_decode(nafp, codec, ch, align, data):
    spb, n_blocks = _spb(codec, ch, align), len(data) // align
    buf = np.ascontiguousarray(data)
    out = np.zeros(max(n_blocks * spb * ch, 1), np.int16)
    assert nafp._lib.load().nafp_codec_decode_host(_code(codec), ch, align, buf.ctypes.data_as(ctypes.c_void_p), n_blocks,
                                                   out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out[:n_blocks * spb * ch]


def _layout(nafp, items, seed=0, skews=(0, 1, 2, 7, 15, 16 - 2, 4, 9)):
    """items: (codec, channels, block_align, uint8 bytes of whole blocks).  Pieces at byte offsets that are skews[i % 8] past a
    16-byte boundary in turn (odd ones among them) and at int16 offsets of alternating parity, 3 or 4 guard samples apart.
    -> (raw, piece array, expected arena)."""
    dt = np.dtype(nafp._lib.CODEC_PIECE_DTYPE)
    rows, chunks, raw_pos, out_pos = [], [], 0, 5
    for i, (codec, ch, align, data) in enumerate(items):
        spb, n_blocks = _spb(codec, ch, align), len(data) // align
        raw_pos = (raw_pos + 15) // 16 * 16 + skews[i % len(skews)]
        rows.append((raw_pos, n_blocks, out_pos, _code(codec), ch, align, spb))
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


def _span(p):
    return int(p['out_off']), int(p['n_blocks']) * int(p['spb']) * int(p['channels'])


def test_qt_device_equals_host_in_one_mixed_launch(nafp):
    """Both channel counts x n_blocks = 0, 1, g - 1, g, g + 1, 2 g + 3 for the reported group g, random-byte packets, every raw
    offset class (odd ones too) and both parities of out_off, IN ONE LAUNCH with pieces of all four older codecs: the whole arena,
    guards included, equals the host's; and the older codecs' ranges equal what a launch of theirs alone writes."""
    lib = nafp._lib.load()
    old = [('alaw', 3, 3, _noise(3 * 2500, 1)), ('ulaw', 1, 1, _noise(4099, 2)), ('ima4', 2, 256, _noise(256 * 70, 3)),
           ('ms4', 1, 37, _noise(37 * 300, 4)), ('ima4', 1, 1024, _noise(1024 * 21, 5)), ('ms4', 2, 512, _noise(512 * 33, 6))]
    items = list(old)
    for ch in (1, 2):
        g = lib.nafp_codec_blocks_per_group(QT, ch, 34 * ch)
        assert g >= 1
        for k, n_blocks in enumerate((0, 1, g - 1, g, g + 1, 2 * g + 3, 1, g + 1)):       # the last two: other offset classes
            items.append(('qtima4', ch, 34 * ch, _noise(n_blocks * 34 * ch, 100 * ch + k)))
    order = np.random.default_rng(1).permutation(len(items))
    raw, pieces, want = _layout(nafp, [items[i] for i in order])
    assert {int(p['raw_off']) % 2 for p in pieces if p['codec'] == QT} == {0, 1} == {int(p['out_off']) % 2 for p in pieces if p['codec'] == QT}
    assert lib.nafp_codec_check_pieces_host(pieces.ctypes.data_as(ctypes.c_void_p), len(pieces), len(raw), len(want)) == 0
    d_raw = torch.from_numpy(raw).cuda()
    out = torch.full((len(want),), SENTINEL, dtype=torch.int16, device='cuda')
    _launch(nafp, d_raw, len(raw), pieces, out, len(want))
    got = out.cpu().numpy()
    bad = [tuple(p) for p in pieces if not np.array_equal(got[_span(p)[0] - 3:sum(_span(p)) + 3], want[_span(p)[0] - 3:sum(_span(p)) + 3])]
    assert not bad and np.array_equal(got, want), f'{len(bad)} pieces differ, e.g. {bad[:5]}'
    assert (want == 32767).any() and (want == -32768).any()
    alone = torch.full((len(want),), SENTINEL, dtype=torch.int16, device='cuda')
    olds = pieces[pieces['codec'] != QT]
    _launch(nafp, d_raw, len(raw), olds, alone, len(want))
    alone = alone.cpu().numpy()
    for p in olds:
        lo, n = _span(p)
        assert alone[lo:lo + n].tobytes() == got[lo:lo + n].tobytes()
    for p in pieces[pieces['codec'] == QT]:
        lo, n = _span(p)
        assert np.all(alone[lo:lo + n] == SENTINEL)


def test_qt_pieces_and_launches_do_not_matter(nafp):
    """The same files cut into different pieces and split over 1, 2 and 5 launches: the same bytes per file."""
    files = [('qtima4', 2, 68, _noise(700 * 68, 11)), ('qtima4', 1, 34, _noise(1111 * 34, 12)), ('ima4', 2, 256, _noise(90 * 256, 13))]
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


@pytest.mark.parametrize('case', ['raw_past_end', 'out_past_end', 'spb', 'align_33', 'three_channels'])
def test_qt_inconsistent_piece(nafp, case):
    """The cases of test_gpu_codec.py::test_inconsistent_piece for code 6.  Three pieces, the middle one inconsistent.  raw_size /
    out_samples are passed SMALLER than the tensors allocated, so every access stays inside allocated memory whatever the kernel
    does and the check is read from the bytes: the piece's stated output range is zeroed (left untouched where it leaves the
    arena), everything past the stated sizes is untouched, the neighbours are decoded."""
    a = ('qtima4', 1, 34, _noise(300 * 34, 1))
    b = ('qtima4', 2, 68, _noise(600 * 68, 2))
    c = ('ima4', 2, 256, _noise(7 * 256, 3))
    raw, pieces, want = _layout(nafp, [a, b, c])
    raw_size, out_samples = len(raw), len(want)
    raw = np.concatenate([raw, _noise(1 << 16, 4)])
    want = np.concatenate([want, np.full(1 << 17, SENTINEL, np.int16)])
    lo, n = _span(pieces[1])
    if case == 'raw_past_end':              # its last block ends one byte past raw_size
        pieces[1]['raw_off'] = raw_size - 600 * 68 + 1
        want[lo:lo + n] = 0
    elif case == 'out_past_end':            # its last sample is one past out_samples: nothing is written
        pieces[1]['out_off'] = out_samples - n + 1
        want[lo:lo + n] = SENTINEL
    elif case == 'spb':                     # states 63 frames per block: the range it states is zeroed, no more
        pieces[1]['spb'] = 63
        want[lo:lo + n] = SENTINEL
        want[lo:lo + 600 * 63 * 2] = 0
    elif case == 'align_33':                # 33 bytes are no packet
        pieces[1]['block_align'], pieces[1]['channels'], pieces[1]['n_blocks'] = 33, 1, 1200
        want[lo:lo + n] = 0
    else:                                   # 3 channels are no Apple IMA4 geometry; 400 blocks x 3 channels state the same range
        pieces[1]['channels'], pieces[1]['block_align'], pieces[1]['n_blocks'] = 3, 102, 400
        want[lo:lo + n] = 0
    assert nafp._lib.load().nafp_codec_check_pieces_host(pieces.ctypes.data_as(ctypes.c_void_p), 3, raw_size, out_samples) in (1, 2)
    out = torch.full((len(want),), SENTINEL, dtype=torch.int16, device='cuda')
    _launch(nafp, torch.from_numpy(raw).cuda(), raw_size, pieces, out, out_samples)
    got = out.cpu().numpy()
    assert np.array_equal(got[out_samples:], want[out_samples:])
    assert np.array_equal(got, want)
    assert np.abs(got[:lo].astype(int)).max() > 1000 and (got[lo + n + 8:out_samples - 8] != SENTINEL).any()


# ---- the consumers ---------------------------------------------------------------------------------------------------------
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


def _be16(x):
    return np.asarray(x).astype('>i2').tobytes()


def test_eight_khz_mono_sixteen_bit_is_the_wav_twin(nafp, tmp_path, monkeypatch):
    """An 8 kHz mono s16be AIFF, a `sowt` AIFC and a 16-bit AU of 2.7 s of noise: the segments are the samples themselves, the
    segments of the WAV twin read natively, in launches of 3 and of 64 rows."""
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource, file_segments
    x = np.random.default_rng(3).integers(-32768, 32768, size=21600).astype(np.int16)
    files = {'a.aiff': aref.aiff_bytes(_be16(x), 8000, 1, 16, junk=((b'NAME', b'odd'),)),
             'b.aifc': aref.aifc_bytes(b'sowt', x.astype('<i2').tobytes(), 8000, 1, 16, ssnd_first=True, ssnd_offset=3),
             'c.au': aref.au_bytes('s16be', _be16(x), 8000, 1, header=29)}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        assert aref.to_wav(data) == iref.wav_bytes('s16', x.astype('<i2').tobytes(), 8000, 1)
    (tmp_path / 'twin.wav').write_bytes(aref.to_wav(files['a.aiff']))
    _clear(monkeypatch)
    twin = SegmentSource([str(tmp_path / 'twin.wav')] * 3, bsz=4)
    want = twin.read_rows(0, twin.n_samples)[:, 0]
    assert np.array_equal(want[:twin.n_samples // 3], file_segments(x, 8000, 1., .5))
    monkeypatch.setenv('NAFP_INGEST_AIFF', '1')
    src = SegmentSource([str(tmp_path / n) for n in files], bsz=4)
    assert src.format == ['s16be', 's16', 's16be'] and all(src.resampled) and src.n_frames == [21600] * 3
    for rows in (3, 64):
        assert np.array_equal(_windows(src, rows), want), rows


@pytest.mark.parametrize('kind,ch,fs_in,fs_out', [('qtima4', 2, 22050, 8000), ('f32be', 1, 11025, 16000)])
def test_rate_conversion_equals_the_ingest_of_the_wav_twin(nafp, tmp_path, monkeypatch, kind, ch, fs_in, fs_out):
    """22.05 kHz stereo `ima4` and 11.025 -> 16 kHz `fl32`, 2.7 s: the segments equal those of to_wav's file under NAFP_INGEST_ANY=1."""
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    x = cref.music(int(2.7 * fs_in), fs_in, ch, 5)
    if kind == 'qtima4':
        data = aref.aifc_bytes(b'ima4', aref.qt_encode(x, ch), fs_in, ch, 16, n_frames=len(x) // 64)       # the stated count wins
    else:
        data = aref.aifc_bytes(b'fl32', (x / 32768.0).astype('>f4').tobytes(), fs_in, ch, 32)
    (tmp_path / 'x.aifc').write_bytes(data)
    (tmp_path / 'y.wav').write_bytes(aref.to_wav(data))
    _clear(monkeypatch)
    monkeypatch.setenv('NAFP_INGEST_ANY', '1')
    want3, want64 = (_windows(SegmentSource([str(tmp_path / 'y.wav')], bsz=4, fs=fs_out), rows) for rows in (3, 64))
    monkeypatch.delenv('NAFP_INGEST_ANY')
    monkeypatch.setenv('NAFP_INGEST_AIFF', '1')
    src = SegmentSource([str(tmp_path / 'x.aifc')], bsz=4, fs=fs_out)
    assert src.format == [kind] and src.n_in == [len(x) // 64 * 64 if kind == 'qtima4' else len(x)]
    assert want3.shape[0] >= 4 and np.abs(want3.astype(int)).max() > 3000 and want3.tobytes() == want64.tobytes()
    for rows in (3, 64):
        assert _windows(src, rows).tobytes() == want3.tobytes(), rows


def _tree(src_dir, conv_dir):
    """A native WAV and a FLAC file next to `.aif` (16- and 24-bit), `.aifc` (sowt, fl32, ulaw, ima4), `.au` (mu-law, 16-bit) and an
    upper-case `.SND`, 2 to 3 s each; `conv_dir`: the same tree converted beforehand by to_wav.  -> the names, sorted as the glob sorts."""
    import wave
    native = cref.music(17000, 8000, 1, 77).astype('<i2')
    for d in (src_dir, conv_dir):
        with wave.open(str(d / 'a.wav'), 'w') as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(8000)
            w.writeframes(native.tobytes())
    xf = fr.music(int(2.3 * 8000), 8000, 1, 16, seed=ord('b'))
    (src_dir / 'b.flac').write_bytes(bytes(fr.write_stream(xf, 16, 8000, block=1152, sub=fr.lpc_recipe(xf[:, 0], 6, 12, porder=3)).data))
    (conv_dir / 'b.wav').write_bytes(fr.pcm_wav(xf, 16, 8000))
    m = lambda seconds, fs, ch, seed: cref.music(int(seconds * fs), fs, ch, seed)
    files = {
        'c.aif': aref.aiff_bytes(_be16(m(2.6, 8000, 1, 1)), 8000, 1, 16),
        'd.aif': aref.aiff_bytes(aref.encode('s24be', m(2.2, 44100, 2, 2).reshape(-1) * 256 + 77), 44100, 2, 24, ssnd_first=True),
        'e.aifc': aref.aifc_bytes(b'sowt', m(2.1, 16000, 2, 3).astype('<i2').tobytes(), 16000, 2, 16, junk=((b'ANNO', b'x'),)),
        'f.aifc': aref.aifc_bytes(b'fl32', (m(2.4, 48000, 1, 4) / 32768.0).astype('>f4').tobytes(), 48000, 1, 32),
        'g.aifc': aref.aifc_bytes(b'ulaw', cref.encode('ulaw', m(2.5, 8000, 1, 5), 1, 1), 8000, 1, 16),
        'h.aifc': aref.aifc_bytes(b'ima4', aref.qt_encode(m(2.3, 44100, 2, 6), 2), 44100, 2, 16),
        'i.au': aref.au_bytes('ulaw', cref.encode('ulaw', m(2.2, 8000, 2, 7), 2, 2), 8000, 2, size=0xffffffff),
        'j.au': aref.au_bytes('s16be', _be16(m(2.0, 22050, 1, 8)), 22050, 1, header=32),
        'k.SND': aref.au_bytes('s8', aref.encode('s8', m(2.1, 11025, 1, 9).reshape(-1) * 256), 11025, 1)}
    for name, data in files.items():
        (src_dir / name).write_bytes(data)
        (conv_dir / (name[:2] + 'wav')).write_bytes(aref.to_wav(data))
    return ['a.wav', 'b.flac'] + list(files)


RATES = {'files': 11, 'resampled': 10, 'flac_files': 1, 'flac_failed_frames': 0,
         'rates': {'8000x1xs16': 1, '8000x1xflac16': 1, '8000x1xs16be': 1, '44100x2xs24be': 1, '16000x2xs16': 1, '48000x1xf32be': 1,
                   '8000x1xulaw': 1, '44100x2xqtima4': 1, '8000x2xulaw': 1, '22050x1xs16be': 1, '11025x1xs8': 1}}


def test_generate_and_identify_end_to_end(nafp, cfg, tmp_path, monkeypatch):
    """`run.py generate -s DIR` with NAFP_INGEST_AIFF=1 on the mixed tree vs the same tree converted beforehand by to_wav and
    generated with NAFP_INGEST_ANY=1: byte-identical .mm, at two launch sizes and at another TS_BATCH_SZ too; source_rates.json
    names the new classes.  Then `run.py identify` on an `.aif` recording (a library track) and on its WAV twin: the same matches.
    One test, because the second command needs what the first one wrote."""
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

    def run(files, bsz, launch_rows):
        src = SegmentSource(files, bsz=bsz)
        arr = np.zeros((src.n_samples, 128), np.float32)
        g.write_fingerprints(src, g.StreamedEmbedder(m_pre, m_fp), arr, group=bsz, launch_rows=launch_rows)
        return arr

    _clear(monkeypatch)
    monkeypatch.setenv('NAFP_INGEST_ANY', '1')
    conv = [str(conv_dir / (n[:2] + 'wav')) for n in names]
    plain5, plain7 = run(conv, 5, 10), run(conv, 7, 14)
    assert plain5.shape[0] == 3 + 3 + 4 + 3 + 3 + 3 + 4 + 3 + 3 + 3 + 3 and np.abs(plain5).sum() > 0
    monkeypatch.delenv('NAFP_INGEST_ANY')
    monkeypatch.setenv('NAFP_INGEST_AIFF', '1')
    mixed = [str(src_dir / n) for n in names]
    for rows in (5, 15):
        assert run(mixed, 5, rows).tobytes() == plain5.tobytes(), rows
    assert run(mixed, 7, 7).tobytes() == plain7.tobytes()
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(NAFP_INGEST_AIFF='1', NAFP_TRACK_TABLE='1', PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), 'generate', 'exp', '-c', 'tiny', '-s', str(src_dir), '--skip_dummy'],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert '10 of 11 files are decoded' in r.stdout
    out_dir = c['DIR']['OUTPUT_ROOT_DIR'] + '/exp/3/'
    got = np.asarray(np.memmap(out_dir + 'custom_source.mm', dtype='float32', mode='r', shape=plain5.shape))
    assert got.tobytes() == plain5.tobytes()
    assert json.load(open(out_dir + 'source_rates.json'))['custom_source'] == RATES
    assert json.load(open(out_dir + 'custom_source_tracks.json'))['files'] == mixed

    # identify: library track c.aif as the recording, once as it is and once as its WAV twin
    rec = tmp_path / 'rec'
    rec.mkdir()
    (rec / 'r.aif').write_bytes((src_dir / 'c.aif').read_bytes())
    (rec / 'r.wav').write_bytes((conv_dir / 'c.wav').read_bytes())
    matches = {}
    for name in ('r.aif', 'r.wav'):
        out = str(tmp_path / (name + '.json'))
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), 'identify', 'exp', '3', str(rec / name), '-c', 'tiny', '-i', 'L2',
                            '--window', '4', '--window_hop', '2', '--min_overlap', '3', '--output', out],
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        matches[name] = [{k: v for k, v in m.items() if k != 'recording'} for m in json.load(open(out))['matches']]
    assert matches['r.aif'] and matches['r.aif'][0]['track'] == str(src_dir / 'c.aif') and matches['r.aif'][0]['track_position_s'] == 0.0
    assert matches['r.aif'] == matches['r.wav']


def test_train_arena(nafp, tmp_path, monkeypatch):
    """PcmArena.device() of the mixed tree == that of the converted tree (NAFP_INGEST_ANY=1), also when the files pass the staging
    buffer in several runs; .host() raises."""
    from neural_audio_fp_amd.model.utils.dataloader_keras import PcmStore, PcmArena
    src_dir, conv_dir = tmp_path / 'src', tmp_path / 'conv'
    src_dir.mkdir(); conv_dir.mkdir()
    names = _tree(src_dir, conv_dir)
    _clear(monkeypatch)
    monkeypatch.setenv('NAFP_INGEST_ANY', '1')
    conv = PcmStore([str(conv_dir / (n[:2] + 'wav')) for n in names], 8000, base=16)
    want = PcmArena([conv]).device().cpu().numpy()
    monkeypatch.delenv('NAFP_INGEST_ANY')
    monkeypatch.setenv('NAFP_INGEST_AIFF', '1')
    for piece in (1 << 25, 1 << 15):                         # the second: several runs per file
        store = PcmStore([str(src_dir / n) for n in names], 8000, base=16)
        assert list(store.n_frames) == list(conv.n_frames) and list(store.start) == list(conv.start)
        assert store.format == ['s16', 'flac16', 's16be', 's24be', 's16', 'f32be', 'ulaw', 'qtima4', 'ulaw', 's16be', 's8']
        arena = PcmArena([store])
        assert arena.device(piece=piece).cpu().numpy().tobytes() == want.tobytes(), piece
    assert np.abs(want.astype(int)).max() > 3000
    with pytest.raises(NotImplementedError):
        arena.host()
