"""CPU: FLAC on the host (include/nafp.h `nafp_flac_*`, csrc/flac_decode.h) -- nafp_flac_decode_host, the function the kernels
decode with compiled for the host, and the bit-level restatement of tests/_flac_ref.py both return THE SAMPLES HANDED TO THE
WRITER over every depth, channel count, stereo mode, subframe, residual and block-size variant; the MD5 of the decode is
STREAMINFO's; nafp_flac_index_host agrees with the restatement's index; refusals are by name; nothing changes without the switch."""
import ctypes
import glob
import hashlib
import os
import struct

import numpy as np
import pytest

import _flac_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p


def _scan(nafp, data):
    from neural_audio_fp_amd.model.utils import flac as fl
    info, index = fl.scan(data)
    return fl, info, index


def host_decode(nafp, data, guard=8):
    """(info, index, scratch bytes, statuses) of the whole stream through nafp_flac_index_host / nafp_flac_decode_host."""
    fl, info, index = _scan(nafp, data)
    assert info['refusal'] == 0
    idx = fl.Index(index, info['channels'], info['bps'], info['rate'])
    rows, _, n_pcm = fl.records(idx, 0, len(idx), int(idx.offset[0]) if len(idx) else 0, 0)
    raw = np.frombuffer(data, np.uint8)
    out = np.full(n_pcm + guard, 0x5a, np.uint8)
    status = np.full(len(rows), -1, np.int32)
    assert nafp._lib.load().nafp_flac_decode_host(raw.ctypes.data_as(VP), len(raw), rows.ctypes.data_as(VP), len(rows), out.ctypes.data_as(VP),
                                                  n_pcm, status.ctypes.data_as(VP)) == 0
    assert (out[n_pcm:] == 0x5a).all()
    return info, index, out[:n_pcm], status


def unjustify(pcm, bps, channels):
    """Scratch bytes -> (n, ch) samples."""
    if bps <= 16:
        return (pcm.view('<i2').astype(np.int64) >> (16 - bps)).reshape(-1, channels)
    b = pcm.reshape(-1, 3).astype(np.int64)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    return ((v ^ (1 << 23)) - (1 << 23) >> (24 - bps)).reshape(-1, channels)


def _index_tuples(index):
    return [(int(e['offset']), int(e['n_bytes']), int(e['first_sample']), int(e['block_size'])) for e in index]


@pytest.mark.parametrize('part', range(4))
def test_host_decode_and_restatement_return_the_writers_samples(nafp, part):
    grid = fr.variant_grid()
    names = [g[0] for g in grid]
    for want in ['depth8x1', 'depth24x8', 'stereo10x24', 'constant', 'verbatim', 'fixed0', 'fixed4', 'lpc1', 'lpc2', 'lpc12', 'lpc32',
                 'precision1', 'precision15_shift14', 'shift0', 'sum_above_32_bits', 'rice0', 'rice14', 'rice30', 'escape0', 'escape1', 'escape25',
                 'porder_largest', 'wasted1', 'wasted7', 'block_8bit16', 'block_code192', 'block_code4096', 'block_code16384', 'short_last']:
        assert want in names
    for name, stream, x, bps in grid[part::4]:
        info, index, pcm, status = host_decode(nafp, stream.data)
        assert (status == 0).all(), (name, status)
        assert pcm.tobytes() == fr.justified(x, bps).tobytes(), name
        assert np.array_equal(unjustify(pcm, bps, x.shape[1]), x), name
        width = (bps + 7) // 8            # STREAMINFO's MD5: the samples interleaved, little-endian, sign-extended to whole bytes, not justified
        packed = unjustify(pcm, bps, x.shape[1]).reshape(-1, 1) >> (8 * np.arange(width)) & 0xff
        assert hashlib.md5(packed.astype(np.uint8).tobytes()).digest() == bytes(info['md5']), name
        assert _index_tuples(index) == stream.frames, name
        r_info, r_frames, y, failed = fr.read_stream(stream.data)
        assert np.array_equal(y, x) and not any(failed), name
        assert r_frames == stream.frames and r_info['md5'] == bytes(info['md5']) == fr.md5_of(x, bps), name
        assert (r_info['rate'], r_info['channels'], r_info['bps']) == (int(info['rate']), int(info['channels']), int(info['bps'])), name


def test_the_grid_reaches_its_edges():
    """The cases are what they say: full scale of both signs, a 25-bit side channel, a prediction sum above 32 bits."""
    grid = {g[0]: g for g in fr.variant_grid()}
    x = grid['stereo8x24'][2]
    assert x.max() == (1 << 23) - 1 and x.min() == -(1 << 23) and np.abs(x[:, 0] - x[:, 1]).max() >= (1 << 24) - 1
    x = grid['sum_above_32_bits'][2][:, 0]
    assert abs(sum(16383 * int(v) for v in x[:32])) > 1 << 40
    assert grid['escape25'][2].max() == (1 << 23) - 1


def test_index_fixed_stream_with_1_2_and_3_byte_frame_numbers(nafp):
    x = fr.music(2100 * 16, 8000, 1, 8, 1)
    stream = fr.write_stream(x, 8, 8000, block=16, sub={'type': 'fixed', 'order': 1})
    assert len(stream.frames) == 2100 and {len(fr._utf8(k)) for k in (0, 127, 128, 2047, 2048, 2099)} == {1, 2, 3}
    fl, info, index = _scan(nafp, stream.data)
    assert _index_tuples(index) == stream.frames == fr.read_index(stream.data)[1]
    assert int(info['n_indexed']) == 2100 and int(info['indexed_samples']) == 2100 * 16
    # a cap below the count: the count is still reported, the entries written are the first ones
    lib, buf = nafp._lib.load(), np.frombuffer(stream.data, np.uint8)
    few, inf2 = np.zeros(10, fl.INDEX_DTYPE), np.zeros(1, fl.INFO_DTYPE)
    assert lib.nafp_flac_index_host(buf.ctypes.data_as(VP), len(buf), inf2.ctypes.data_as(VP), few.ctypes.data_as(VP), 10) == 0
    assert int(inf2[0]['n_indexed']) == 2100 and _index_tuples(few) == stream.frames[:10]


def test_index_variable_stream_first_number_id3_and_totals(nafp):
    x = fr.music(1000, 44100, 2, 16, 2)
    frames = [{'block': b, 'subframes': {'type': 'fixed', 'order': 2}} for b in (300, 100, 17, 583)]
    for kw in ({'variable': True, 'frames': frames}, {'variable': True, 'frames': frames, 'first_number': 60000000000},
               {'block': 250, 'first_number': 70000}, {'block': 250, 'id3': 777}, {'block': 250, 'total': 0}, {'block': 250, 'total': 900},
               {'block': 250, 'total': 5000}):
        stream = fr.write_stream(x, 16, 44100, **kw)
        fl, info, index = _scan(nafp, stream.data)
        r_info, r_frames = fr.read_index(stream.data)
        assert _index_tuples(index) == stream.frames == r_frames, kw
        assert int(info['audio_off']) == stream.audio_off == r_info['audio_off']
        _, _, pcm, status = host_decode(nafp, stream.data)
        assert (status == 0).all() and pcm.tobytes() == fr.justified(x, 16).tobytes()
        total = kw.get('total')
        want = 900 if total == 900 else 1000                   # 0 and 5000 (above the indexed sum) fall back to the indexed sum
        assert fr.n_frames_of(r_info, r_frames) == want
        t, s = int(info['total_samples']), int(info['indexed_samples'])
        assert (t if 0 < t <= s else s) == want


def test_index_truncated_last_frame_is_left_out(nafp):
    x = fr.music(768, 22050, 1, 16, 3)
    stream = fr.write_stream(x, 16, 22050, block=256)
    for cut in (1, 2, 40, stream.frames[-1][1] - 7):
        data = stream.data[:-cut]
        fl, info, index = _scan(nafp, data)
        assert _index_tuples(index) == stream.frames[:2] == fr.read_index(data)[1]
        assert int(info['indexed_samples']) == 512
    data = stream.data + bytes(128)                           # trailing bytes behind a whole last frame do not hurt it
    _, _, pcm, status = host_decode(nafp, data)
    assert (status == 0).all() and pcm.tobytes() == fr.justified(x, 16).tobytes()


@pytest.mark.parametrize('continues', [False, True])
def test_planted_sync_with_valid_crc8_is_dropped_or_fails(nafp, continues):
    """A complete frame header (sync, valid codes, valid CRC-8) sits inside a verbatim subframe.  With a number that breaks
    continuity it is dropped and every frame decodes; with the number that continues the chain it is taken, its predecessor ends
    early and both FAIL -- zeros, never other samples."""
    rate, block = 16000, 64
    x = fr.music(3 * block, rate, 1, 16, 4)
    head = bytes([0xff, 0xf8, (6 << 4) | 0, (0 << 4) | 0]) + fr._utf8(2 if continues else 9) + bytes([block - 1])
    head += bytes([fr.crc8(head)])
    assert len(head) == 7
    planted = np.frombuffer(head + b'\x00', '>i2').astype(np.int64)       # four verbatim 16-bit samples of frame 1
    x[block + 10:block + 14, 0] = planted
    stream = fr.write_stream(x, 16, rate, block=block, sub={'type': 'verbatim'})
    at = stream.data.find(head, stream.frames[1][0])
    assert stream.frames[1][0] < at < stream.frames[2][0]
    info, index, pcm, status = host_decode(nafp, stream.data)
    got = unjustify(pcm, 16, 1)
    r_info, r_frames, y, failed = fr.read_stream(stream.data)
    assert _index_tuples(index) == r_frames
    if not continues:
        assert _index_tuples(index) == stream.frames and (status == 0).all() and np.array_equal(got, x) and np.array_equal(y, x)
        return
    assert [f[0] for f in r_frames] == [stream.frames[0][0], stream.frames[1][0], at]       # the true frame 2 no longer continues
    assert status[0] == 0 and status[1] != 0 and status[2] != 0 and failed == [False, True, True]
    assert np.array_equal(got[:block], x[:block]) and not got[block:].any() and np.array_equal(got, y)


def _streaminfo_patch(data, **kw):
    """The stream with STREAMINFO fields overwritten: bps, max_block."""
    b = bytearray(data)
    at = data.index(b'fLaC') + 8
    word = int.from_bytes(b[at + 10:at + 18], 'big')
    if 'bps' in kw:
        word = (word & ~(31 << 36)) | ((kw['bps'] - 1) << 36)
    b[at + 10:at + 18] = word.to_bytes(8, 'big')
    if 'max_block' in kw:
        b[at + 2:at + 4] = struct.pack('>H', kw['max_block'])
    return bytes(b)


def test_flac_scan_refuses_by_name(nafp, tmp_path, monkeypatch):
    from neural_audio_fp_amd.model.utils.audio_utils import flac_scan
    monkeypatch.setenv('NAFP_INGEST_FLAC', '1')
    good = fr.write_stream(fr.music(512, 8000, 1, 16, 5), 16, 8000, block=256).data
    at = good.index(b'fLaC')
    cases = {'ogg': (b'OggS' + good[4:], 'Ogg'), 'marker': (b'RIFF' + good[4:], 'fLaC marker'),
             'streaminfo_type': (good[:at + 4] + b'\x04' + good[at + 5:], 'STREAMINFO'),
             'streaminfo_len': (good[:at + 7] + b'\x21' + good[at + 8:], 'STREAMINFO'),
             'bits32': (_streaminfo_patch(good, bps=32), '32-bit'), 'bits17': (_streaminfo_patch(good, bps=17), '17-bit'),
             'block': (_streaminfo_patch(good, max_block=16385), 'block size 16385'),
             'no_frame': (good[:fr.read_streaminfo(good)['audio_off']] + bytes(300), 'no valid FLAC frame'),
             'rate': (fr.write_stream(fr.music(512, 7999, 1, 16, 5), 16, 7999, block=256).data, 'Sample rate should be 8000 but got 7999')}
    for name, (data, word) in cases.items():
        path = tmp_path / f'{name}.flac'
        path.write_bytes(data)
        with pytest.raises(ValueError, match=word):
            flac_scan(str(path), 8000)
        if name not in ('no_frame', 'rate'):
            with pytest.raises(fr.Refused):
                fr.read_streaminfo(data)
    (tmp_path / 'good.flac').write_bytes(good)
    info = flac_scan(str(tmp_path / 'good.flac'), 8000)
    assert (info['rate'], info['channels'], info['format'], info['n_frames'], info['codec']) == (8000, 1, 'flac16', 512, 'flac')
    assert len(info['frames']) == 2 and list(info['index'].start) == [0, 256, 512]


def _records(nafp, stream):
    fl, info, index = _scan(nafp, stream.data)
    idx = fl.Index(index, info['channels'], info['bps'], info['rate'])
    rows, _, n_pcm = fl.records(idx, 0, len(idx), int(idx.offset[0]), 0)
    return fl, rows, n_pcm


def test_check_frames_is_the_kernels_check(nafp):
    """nafp_flac_check_frames_host rejects exactly the records that nafp_flac_decode_host gives status 1 (range zeroed) or 8
    (nothing written)."""
    lib = nafp._lib.load()
    stream = fr.golden_streams()[0]
    fl, rows, n_pcm = _records(nafp, stream)
    raw = np.frombuffer(stream.data, np.uint8)
    assert lib.nafp_flac_check_frames_host(rows.ctypes.data_as(VP), len(rows), len(raw), n_pcm) == 0
    changes = [('raw_off', len(raw) - int(rows[1]['n_bytes']) + 1, 1), ('raw_off', -1, 1), ('n_bytes', 0, 1), ('bps', 17, 1), ('bps', 32, 8),
               ('bps', 0, 8), ('rate', 0, 1), ('rate', 655351, 1), ('channels', 0, 8), ('channels', 9, 8), ('block_size', 0, 8),
               ('block_size', 16385, 8), ('scratch_off', -1, 8), ('scratch_off', n_pcm - int(rows[1]['block_size']) * 4 + 1, 8)]
    for field, value, want in changes:
        bad = rows.copy()
        bad[1][field] = value
        assert lib.nafp_flac_check_frames_host(bad.ctypes.data_as(VP), len(bad), len(raw), n_pcm) == 1, (field, value)
        out = np.full(n_pcm, 0x5a, np.uint8)
        status = np.zeros(len(bad), np.int32)
        assert lib.nafp_flac_decode_host(raw.ctypes.data_as(VP), len(raw), bad.ctypes.data_as(VP), len(bad), out.ctypes.data_as(VP), n_pcm,
                                         status.ctypes.data_as(VP)) == 0
        assert status[1] == want and status[0] == 0 and status[2] == 0, (field, value, status)
    # a record the checks accept whose frame header disagrees with it (the file's STREAMINFO) fails as a mismatch; golden stream 2
    # codes depth and rate in its second frame's header
    for k, field, value in ((0, 'block_size', 32), (0, 'channels', 1), (2, 'bps', 20), (2, 'rate', 44100)):
        stream = fr.golden_streams()[k]
        fl, rows, n_pcm = _records(nafp, stream)
        raw = np.frombuffer(stream.data, np.uint8)
        bad = rows.copy()
        bad[1][field] = value
        if field == 'channels':
            bad[1]['block_size'] = 32
        out, status = np.zeros(n_pcm + 4096, np.uint8), np.zeros(len(bad), np.int32)
        assert lib.nafp_flac_check_frames_host(bad.ctypes.data_as(VP), len(bad), len(raw), len(out)) == 0
        assert lib.nafp_flac_decode_host(raw.ctypes.data_as(VP), len(raw), bad.ctypes.data_as(VP), len(bad), out.ctypes.data_as(VP), len(out),
                                         status.ctypes.data_as(VP)) == 0
        assert status[1] == 3 and status[0] == 0, (field, status)


def test_named_mutations_fail_on_the_host(nafp):
    """The corrupt-input cases the GPU test launches, here through nafp_flac_decode_host: frame 1 fails and is zero, the others are
    the writer's samples, the guard bytes stay."""
    lib = nafp._lib.load()
    stream = fr.golden_streams()[0]
    fl, rows, n_pcm = _records(nafp, stream)
    x = fr.music(16 * 6, 8000, 2, 16, 1, .9)
    want = fr.justified(x, 16).copy()
    want[64:128] = 0
    reasons = {}
    for name, (data, rec) in fr.named_mutations(stream).items():
        raw = np.frombuffer(data, np.uint8)
        bad = rows.copy()
        for k, v in rec.items():
            bad[1][k] = v
        out, status = np.full(n_pcm + 8, 0x5a, np.uint8), np.zeros(len(bad), np.int32)
        assert lib.nafp_flac_decode_host(raw.ctypes.data_as(VP), len(raw), bad.ctypes.data_as(VP), len(bad), out.ctypes.data_as(VP), n_pcm,
                                         status.ctypes.data_as(VP)) == 0
        assert status[1] != 0 and (np.delete(status, 1) == 0).all(), (name, status)
        assert out[:n_pcm].tobytes() == want.tobytes() and (out[n_pcm:] == 0x5a).all(), name
        reasons[name] = int(status[1])
    assert reasons == {'bit_flip': 7, 'truncation': 4, 'unary_run': 4, 'lpc_order_above_block': 5, 'reserved_subframe_type': 5,
                       'inconsistent_record': 1}


def test_golden_streams_are_the_writers(nafp):
    """tests/golden/flac_streams_v1.bin, the seed file of tools/flac_host_check.cpp, is what golden_streams() writes today."""
    streams = fr.golden_streams()
    blob = b'NAFPFLAC' + struct.pack('<I', len(streams)) + b''.join(struct.pack('<I', len(s.data)) + s.data for s in streams)
    assert open(os.path.join(ROOT, 'tests', 'golden', 'flac_streams_v1.bin'), 'rb').read() == blob
    for s in streams:
        _, _, _, status = host_decode(nafp, s.data)
        assert len(status) == len(s.frames) and (status == 0).all()


def test_null_and_negative_arguments(nafp):
    lib = nafp._lib.load()
    buf, info = np.zeros(64, np.uint8), np.zeros(72, np.uint8)
    p, i = buf.ctypes.data_as(VP), info.ctypes.data_as(VP)
    assert lib.nafp_flac_streaminfo_host(None, 64, i) == 1 and lib.nafp_flac_streaminfo_host(p, -1, i) == 1
    assert lib.nafp_flac_streaminfo_host(p, 64, None) == 1 and lib.nafp_flac_streaminfo_host(p, 64, i) == 0
    assert lib.nafp_flac_index_host(None, 64, i, None, 0) == 1 and lib.nafp_flac_index_host(p, 64, i, None, 4) == 1
    assert lib.nafp_flac_index_host(p, 64, i, None, -1) == 1 and lib.nafp_flac_index_host(p, -1, i, None, 0) == 1
    assert lib.nafp_flac_decode_host(None, 64, p, 1, p, 64, None) == 1 and lib.nafp_flac_decode_host(p, 64, None, 1, p, 64, None) == 1
    assert lib.nafp_flac_decode_host(p, 64, p, -1, p, 64, None) == 1 and lib.nafp_flac_decode_host(p, 64, p, 1, None, 64, None) == 1
    assert lib.nafp_flac_decode_host(p, -1, p, 1, p, 64, None) == 1 and lib.nafp_flac_decode_host(p, 64, p, 1, p, -1, None) == 1
    assert lib.nafp_flac_decode_host(p, 64, None, 0, p, 64, None) == 0
    assert lib.nafp_flac_check_frames_host(None, 1, 64, 64) == 1 and lib.nafp_flac_check_frames_host(p, -1, 64, 64) == 1
    assert lib.nafp_flac_check_frames_host(p, 1, -1, 64) == 1 and lib.nafp_flac_check_frames_host(None, 0, 64, 64) == 0
    assert lib.nafp_flac_decode(None, 64, p, 1, p, 64, None, None) == 1 and lib.nafp_flac_decode(p, 64, None, 1, p, 64, None, None) == 1
    assert lib.nafp_flac_decode(p, 64, p, 1, None, 64, None, None) == 1 and lib.nafp_flac_decode(p, 64, p, -1, p, 64, None, None) == 1
    assert lib.nafp_flac_decode(p, -1, p, 1, p, 64, None, None) == 1 and lib.nafp_flac_decode(p, 64, p, 1, p, -1, None, None) == 1


@pytest.mark.parametrize('env', [{}, {'NAFP_INGEST_CODECS': '1'}, {'NAFP_INGEST_ANY': '1'}, {'NAFP_RESAMPLE': '1'}])
def test_flac_names_are_refused_without_the_switch(nafp, tmp_path, monkeypatch, env):
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource, wav_info
    from neural_audio_fp_amd.model.utils.dataloader_keras import PcmStore
    for k in ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS', 'NAFP_INGEST_FLAC'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    path = tmp_path / 'a.flac'
    path.write_bytes(fr.write_stream(fr.music(9000, 8000, 1, 16, 6), 16, 8000, block=1024).data)
    for name in (str(path), str(tmp_path / 'b.FLAC')):
        for make in (lambda: SegmentSource([name], bsz=4), lambda: PcmStore([name], 8000), lambda: wav_info(name, 8000)):
            with pytest.raises(NotImplementedError) as e:
                make()
            assert e.value.args == (name[-3:],) and name[-3:] in ('lac', 'LAC')


def test_with_the_switch_the_sources_take_flac_and_have_no_cpu_path(nafp, tmp_path, monkeypatch):
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    from neural_audio_fp_amd.model.utils.dataloader_keras import PcmStore, PcmArena
    from neural_audio_fp_amd.model.utils.ingest import rates_summary
    from neural_audio_fp_amd.model import dataset
    for k in ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('NAFP_INGEST_FLAC', '1')
    (tmp_path / 'b.FLAC').write_bytes(fr.write_stream(fr.music(20000, 44100, 2, 16, 7), 16, 44100, block=4096).data)
    (tmp_path / 'a.flac').write_bytes(fr.write_stream(fr.music(9000, 8000, 1, 24, 8), 24, 8000, block=1024).data)
    (tmp_path / 'c.wav').write_bytes(fr.pcm_wav(fr.music(9000, 8000, 1, 16, 9), 16, 8000))
    (tmp_path / 'd.txt').write_bytes(b'x')
    files = dataset._audio_files(str(tmp_path) + '/**/')
    assert [os.path.basename(f) for f in files] == ['a.flac', 'b.FLAC', 'c.wav']
    monkeypatch.delenv('NAFP_INGEST_FLAC')
    assert [os.path.basename(f) for f in dataset._audio_files(str(tmp_path) + '/**/')] == ['c.wav']
    monkeypatch.setenv('NAFP_INGEST_FLAC', '1')
    src = SegmentSource(files, bsz=4)
    assert src.ingest and src.codecs and src.resample and src.resampled == [True, True, False]
    assert src.n_in == [9000, 20000, 9000] and src.format == ['flac24', 'flac16', 's16']
    assert rates_summary(src)['rates'] == {'8000x1xflac24': 1, '44100x2xflac16': 1, '8000x1xs16': 1}
    with pytest.raises(NotImplementedError):
        src.read_rows(0, 1)
    with pytest.raises(NotImplementedError):
        next(src.iter_rows(0, 2, 2))
    store = PcmStore(files, 8000)
    assert list(store.n_frames) == src.n_frames and sorted(store.flac_index) == [0, 1]
    with pytest.raises(NotImplementedError):
        PcmArena([store]).host()


@pytest.mark.skipif(not os.path.isdir(os.environ.get('NAFP_FLAC_SAMPLES', '')), reason='NAFP_FLAC_SAMPLES names no directory of FLAC files')
def test_md5_of_real_files(nafp):
    """The recipe that pins parity with real encoders: every .flac under $NAFP_FLAC_SAMPLES is decoded on the host and the MD5 of
    its samples compared with the one its encoder wrote into STREAMINFO."""
    paths = [p for p in glob.glob(os.path.join(os.environ['NAFP_FLAC_SAMPLES'], '**', '*'), recursive=True) if p[-5:].lower() == '.flac']
    assert paths
    for path in paths:
        data = open(path, 'rb').read()
        info, index, pcm, status = host_decode(nafp, data)
        assert (status == 0).all(), (path, np.flatnonzero(status))
        x = unjustify(pcm, int(info['bps']), int(info['channels']))
        total = int(info['total_samples'])
        if 0 < total <= len(x):
            x = x[:total]
        if bytes(info['md5']) != bytes(16):
            assert fr.md5_of(x, int(info['bps'])) == bytes(info['md5']), path
