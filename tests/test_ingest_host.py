"""CPU: the host side of the general ingest (include/nafp.h `nafp_ingest_*`, model/utils/ingest.py, riff_scan_ex) against the
numpy restatement tests/_ingest_ref.py -- geometry in both directions, the quantised filter and its response, the decode of
every sample format at its edges, the header scan's accept / refuse rules, and the pieces SegmentSource hands to the device.
No GPU call."""
import ctypes
import struct

import numpy as np
import pytest

import _ingest_ref as ref

RATIOS = [(4000, 8000), (8000, 16000), (11025, 16000), (6000, 8000), (44100, 16000), (44100, 8000), (48000, 8000), (22050, 8000)]


def _geometry(lib, fs_in, fs_out):
    v = [ctypes.c_int() for _ in range(4)]
    st = lib.nafp_ingest_geometry(fs_in, fs_out, *[ctypes.byref(x) for x in v])
    return st, tuple(x.value for x in v)


def _table(lib, fs_in, fs_out):
    st, (L, M, half, T) = _geometry(lib, fs_in, fs_out)
    assert st == 0
    tab = np.zeros((L, T), np.int32)
    assert lib.nafp_ingest_table_host(fs_in, fs_out, tab.ctypes.data_as(ctypes.c_void_p)) == 0
    return tab


def _decode(lib, fmt, data):
    n = len(data) // ref.FORMATS[fmt][1]
    buf = np.frombuffer(b'\0' + bytes(data), np.uint8)[1:]                 # an odd address: the decode takes any alignment
    q = np.full(n, -1, np.int32)
    assert lib.nafp_ingest_decode_host(ref.FORMATS[fmt][0], buf.ctypes.data_as(ctypes.c_void_p), n, q.ctypes.data_as(ctypes.c_void_p)) == 0
    return q.astype(np.int64)


def test_geometry_is_the_issue_table(nafp):
    lib = nafp._lib.load()
    want = {(4000, 8000): (2, 1, 68, 69), (11025, 16000): (640, 441, 21558, 68), (6000, 8000): (4, 3, 135, 68),
            (44100, 8000): (80, 441, 14855, 372)}
    for (a, b), g in want.items():
        assert _geometry(lib, a, b) == (0, g)
        assert ref.geometry(a, b) == g
    assert _geometry(lib, 8000, 8000) == (0, (1, 1, 0, 1)) and _geometry(lib, 16000, 16000) == (0, (1, 1, 0, 1))
    rates = (4000, 6000, 8000, 8001, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 1, 100)
    taken = 0
    for a in rates:
        for b in rates:
            g = ref.geometry(a, b)
            st, got = _geometry(lib, a, b)
            assert (st, got) == ((2, (0, 0, 0, 0)) if g is None else (0, g)), (a, b)
            assert lib.nafp_ingest_n_out(1000, a, b) == (-1 if g is None else ref.n_out(1000, a, b))
            taken += g is not None
    assert taken > 150
    assert ref.geometry(8000, 8001) is None and ref.geometry(8001, 8000) is None            # L = 8001 / 8000 > 640
    assert ref.geometry(11025, 16000) is not None and ref.geometry(11024, 16000) is None    # L = 640 / 1000
    assert _geometry(lib, 200000, 8000)[0] == 2 and _geometry(lib, 8000, 200000)[0] == 2
    assert _geometry(lib, 0, 8000)[0] == 1 and _geometry(lib, 8000, -1)[0] == 1
    assert _geometry(lib, 192000, 1)[0] == 2                                                # the block span beyond 64 KB of LDS
    h = ctypes.c_void_p()
    assert lib.nafp_ingest_create(ctypes.byref(h), 192000, 1) == 2 and not h.value          # at plan creation, before any GPU call
    assert lib.nafp_ingest_create(ctypes.byref(h), 8000, 8001) == 2 and not h.value
    assert lib.nafp_ingest_create(None, 44100, 8000) == 1
    assert lib.nafp_ingest_table_host(44100, 8000, None) == 1
    assert lib.nafp_ingest_i16(None, None, 0, None, 0, None, 0, None) == 1
    assert lib.nafp_ingest_n_out(-1, 4000, 8000) == -1


@pytest.mark.parametrize('fs_in,fs_out', RATIOS)
def test_table_is_the_float64_design(nafp, fs_in, fs_out):
    tab = _table(nafp._lib.load(), fs_in, fs_out).astype(np.int64)
    # the library's I0 / sin and numpy's may differ in the last bit: +-1 unit of 2^-30, not equality (as for the resampler)
    assert np.abs(tab - ref.table(fs_in, fs_out)).max() <= 1
    L, M, half, T = ref.geometry(fs_in, fs_out)
    flat = tab.T.reshape(-1)                                         # index p + t L = v + half
    assert not flat[2 * half + 1:].any() and np.array_equal(flat[:2 * half + 1], flat[:2 * half + 1][::-1])
    # tap sums: |acc| <= 2^26 * 2.5 * 2^30 < 2^58; every phase passes DC unchanged
    assert (np.abs(tab).sum(axis=1) / 2.0 ** 30).max() < 2.5
    assert np.abs(tab.sum(axis=1) / 2.0 ** 30 - 1.0).max() < 1e-4


@pytest.mark.parametrize('fs_in,fs_out', [(44100, 8000), (48000, 8000), (11025, 8000), (44100, 16000), (192000, 8000), (8000, 8000)])
def test_downsampling_table_is_the_resamplers(nafp, fs_in, fs_out):
    lib = nafp._lib.load()
    v = [ctypes.c_int() for _ in range(4)]
    assert lib.nafp_resample_geometry(fs_in, fs_out, *[ctypes.byref(x) for x in v]) == 0
    assert _geometry(lib, fs_in, fs_out) == (0, tuple(x.value for x in v))
    old = np.zeros((v[0].value, v[3].value), np.int32)
    assert lib.nafp_resample_table_host(fs_in, fs_out, old.ctypes.data_as(ctypes.c_void_p)) == 0
    assert _table(lib, fs_in, fs_out).tobytes() == old.tobytes()


@pytest.mark.parametrize('fs_in,fs_out', [(4000, 8000), (11025, 16000), (44100, 16000)])
def test_response_of_the_quantised_table(nafp, fs_in, fs_out):
    """From the library's table by an FFT at the virtual rate, lo = the lower rate: flat to 0.001 dB up to 0.85 lo / 2, at most
    -85 dB from 1.05 lo / 2 (measured on a +-1 perturbed table while the contract was written: 0.00038 dB, -87.5 dB)."""
    tab = _table(nafp._lib.load(), fs_in, fs_out).astype(np.float64)
    L, M, half, T = ref.geometry(fs_in, fs_out)
    h = tab.T.reshape(-1)[:2 * half + 1] / 2.0 ** 30 / L             # unit DC gain
    fv, lo = fs_in * L, min(fs_in, fs_out)
    n_fft = 1 << int(np.ceil(np.log2(len(h) * 16)))
    H = np.abs(np.fft.rfft(h, n_fft))
    f = np.arange(len(H)) * fv / n_fft
    db = 20 * np.log10(np.maximum(H, 1e-30))
    print(f'{fs_in}->{fs_out}: ripple {np.abs(db[f <= 0.85 * lo / 2]).max():.6f} dB, stop band {db[f >= 1.05 * lo / 2].max():.2f} dB')
    assert np.abs(db[f <= 0.85 * lo / 2]).max() <= 0.001
    assert db[f >= 1.05 * lo / 2].max() <= -85.0


def test_restatement_equals_the_definition():
    rng = np.random.default_rng(0)
    for (a, b), n in (((4000, 8000), 200), ((11025, 16000), 150), ((6000, 8000), 300), ((44100, 8000), 1000), ((8000, 8000), 50)):
        m = rng.integers(-2 ** 26, 2 ** 26 + 1, size=n)
        assert np.array_equal(ref.accumulate(m, a, b), ref.accumulate_by_definition(m, a, b))
    # floor division, not truncation, and the 64-bit range: 8 full-scale channels behind the largest tap sum
    assert list(ref.finish(np.array([-1, -(1 << 37) - 1, -(1 << 37), (1 << 37) - 1, 1 << 37, 3 << 37, -(3 << 37) - 1]), 1)) == [0, -1, 0, 0, 1, 2, -2]
    assert list(ref.finish(np.array([(3 << 38) + (3 << 37) - 1, (3 << 38) + (3 << 37), -(3 << 37) - 1]), 3)) == [1, 2, -1]
    assert int(np.abs(ref.accumulate(np.full(600, 2 ** 26), 44100, 8000)).max()) < 2 ** 58


def test_input_range_and_n_out_against_brute_force(nafp):
    from neural_audio_fp_amd.model.utils import ingest as ig
    for a, b in ((4000, 8000), (11025, 16000), (6000, 8000), (44100, 8000), (8000, 8000)):
        L, M, half, T = ref.geometry(a, b)
        for n_in in (0, 1, 2, 5, T * M // L - 1, T * M // L + 1, 441):
            no = ref.n_out(n_in, a, b)
            assert ig.n_out(n_in, a, b) == no
            grid = sorted({g for g in (0, 1, 2, 33, no // 2, no - 1, no) if 0 <= g <= no})
            for n0 in grid:
                for n1 in grid:
                    if n1 < n0:
                        continue
                    got, want = ig.input_range(n0, n1, n_in, a, b), ref.input_range(n0, n1, n_in, a, b)
                    if want is None:
                        assert got[0] == got[1], (a, b, n_in, n0, n1, got)
                    else:
                        assert got == want, (a, b, n_in, n0, n1, got, want)
    lib = nafp._lib.load()
    x, y = ctypes.c_int64(), ctypes.c_int64()
    assert lib.nafp_ingest_input_range(5, 4, 100, 4000, 8000, ctypes.byref(x), ctypes.byref(y)) == 1
    assert lib.nafp_ingest_input_range(0, 4, 100, 4000, 8000, None, None) == 1


def test_decode_every_format_at_its_edges(nafp):
    lib = nafp._lib.load()
    rng = np.random.default_rng(3)
    Q = 2 ** 23
    # 8-bit unsigned
    data = bytes([0, 128, 255, 1, 127, 129]) + rng.integers(0, 256, 500).astype(np.uint8).tobytes()
    got = _decode(lib, 'u8', data)
    assert list(got[:3]) == [-Q, 0, 127 << 16] and np.array_equal(got, ref.decode('u8', data))
    # 16-bit
    data = np.concatenate([[-32768, 32767, 0, -1, 1], rng.integers(-32768, 32768, 500)]).astype('<i2').tobytes()
    got = _decode(lib, 's16', data)
    assert list(got[:4]) == [-Q, 32767 << 8, 0, -256] and np.array_equal(got, ref.decode('s16', data))
    # 24-bit, 3 bytes
    vals = np.concatenate([[-Q, Q - 1, 0, -1, 1, 0x7fff00, -0x800000 + 1], rng.integers(-Q, Q, 500)]).astype('<i4')
    data = vals.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    got = _decode(lib, 's24', data)
    assert np.array_equal(got, vals) and np.array_equal(got, ref.decode('s24', data))
    # 32-bit: rounded to 24 bits, the top clamped
    vals = np.concatenate([[0x7fffffff, 0x7fffff80, 0x7fffff7f, -2 ** 31, 0x0000007f, 0x00000080, -0x80, -0x81, 0x17f, 0x180,
                            -0x17f - 1, -0x181, 0, -1], rng.integers(-2 ** 31, 2 ** 31, 500)]).astype('<i4')
    got = _decode(lib, 's32', vals.tobytes())
    assert list(got[:8]) == [Q - 1, Q - 1, Q - 1, -Q, 0, 1, 0, -1]
    assert np.array_equal(got, ref.decode('s32', vals.tobytes()))
    assert np.array_equal(got, np.minimum(np.floor(vals.astype(np.float64) / 256 + 0.5), Q - 1))
    # floats: zeros, full scale and just below it, beyond, infinities, NaN, denormals, exact ties for even and odd k
    for fmt, ft, eps, tiny in (('f32', np.float32, 2.0 ** -24, 1e-40), ('f64', np.float64, 2.0 ** -53, 1e-310)):
        k = np.array([0, 1, 2, 3, 4, 5, 1000, 1001, Q - 2, Q - 1, 12344, 12345], np.float64)
        ties = (k + 0.5) * 2.0 ** -23
        special = [0.0, -0.0, 1.0, -1.0, 1.0 - eps, -(1.0 - eps), 2.0, -2.0, np.inf, -np.inf, np.nan, tiny, -tiny,
                   np.finfo(ft).tiny, np.finfo(ft).max, -np.finfo(ft).max, 0.25 * 2.0 ** -23, 0.5 * 2.0 ** -23, 0.75 * 2.0 ** -23,
                   1.0 - 2.0 ** -24, -(1.0 - 2.0 ** -24), 1.0 - 2.0 ** -23, 1.0 - 1.5 * 2.0 ** -23]
        with np.errstate(all='ignore'):
            vals = np.concatenate([special, ties, -ties, rng.uniform(-1.2, 1.2, 500), rng.uniform(-1, 1, 200) * 2.0 ** -20,
                                   rng.integers(-Q, Q, 200) * 2.0 ** -23 + rng.choice([0.5, -0.5, 0.25], 200) * 2.0 ** -23]).astype(ft)
        assert np.array_equal(vals[len(special):len(special) + len(k)].astype(np.float64), ties)          # representable: ties stay ties
        data = vals.astype('<f4' if fmt == 'f32' else '<f8').tobytes()
        got = _decode(lib, fmt, data)
        assert list(got[:13]) == [0, 0, Q - 1, -Q, Q - 1, -Q, Q - 1, -Q, Q - 1, -Q, 0, 0, 0], fmt
        assert list(got[13:20]) == [0, Q - 1, -Q, 0, 0, 1, Q - 1], fmt
        assert list(got[len(special):len(special) + len(k)]) == [0, 2, 2, 4, 4, 6, 1000, 1002, Q - 2, Q - 1, 12344, 12346], fmt   # ties to even (Q clamps to Q - 1)
        assert list(got[len(special) + len(k):len(special) + 2 * len(k)]) == [0, -2, -2, -4, -4, -6, -1000, -1002, -(Q - 2), -Q, -12344, -12346], fmt
        assert np.array_equal(got, ref.decode(fmt, data)), fmt
        # a NaN of either sign and with any payload is 0
        nan_bits = (np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff], np.uint32).astype('<u4').tobytes() if fmt == 'f32'
                    else np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xfff0000000000001], np.uint64).astype('<u8').tobytes())
        assert not _decode(lib, fmt, nan_bits).any()
    q = np.zeros(4, np.int32)
    assert lib.nafp_ingest_decode_host(0, q.ctypes.data_as(ctypes.c_void_p), 1, q.ctypes.data_as(ctypes.c_void_p)) == 2
    assert lib.nafp_ingest_decode_host(7, q.ctypes.data_as(ctypes.c_void_p), 1, q.ctypes.data_as(ctypes.c_void_p)) == 2
    assert lib.nafp_ingest_decode_host(2, None, 1, q.ctypes.data_as(ctypes.c_void_p)) == 1
    assert lib.nafp_ingest_decode_host(2, None, 0, None) == 0


def _body(fmt, n, ch, seed=0):
    q = np.random.default_rng(seed).integers(-2 ** 23, 2 ** 23, size=n * ch)
    return ref.encode(fmt, q)


def test_riff_scan_ex_accepts(nafp, tmp_path):
    from neural_audio_fp_amd.model.utils.audio_utils import riff_scan_ex
    for fmt, (code, width) in ref.FORMATS.items():
        for ext in (False, True):
            for ch in (1, 3):
                p = tmp_path / f'{fmt}_{int(ext)}_{ch}.wav'
                p.write_bytes(ref.wav_bytes(fmt, _body(fmt, 100, ch), 44100, ch, extensible=ext))
                info = riff_scan_ex(str(p), 8000)
                assert info == {'rate': 44100, 'channels': ch, 'format': fmt, 'width': width, 'block_align': ch * width,
                                'offset': 12 + 8 + (40 if ext else 16) + 8, 'n_frames': 100}, (fmt, ext, ch)
    # an extensible header's container is block_align / channels whatever wBitsPerSample / wValidBitsPerSample say (20 valid bits in 3 bytes)
    p = tmp_path / 'valid20.wav'
    p.write_bytes(ref.wav_bytes('s24', _body('s24', 10, 2), 48000, 2, extensible=True, bits=20))
    assert riff_scan_ex(str(p), 8000)['format'] == 's24'
    # an odd-sized chunk before `data` (padded to even), and a data size larger than the file (a truncated / streamed file)
    p = tmp_path / 'odd_chunk.wav'
    p.write_bytes(ref.wav_bytes('s24', _body('s24', 77, 2), 48000, 2, extra_chunk=b'x' * 13))
    info = riff_scan_ex(str(p), 8000)
    assert info['n_frames'] == 77 and info['offset'] == 12 + 24 + 8 + 14 + 8
    p = tmp_path / 'big_data.wav'
    p.write_bytes(ref.wav_bytes('f32', _body('f32', 50, 1), 16000, 1, data_size=0xFFFFFFFF))
    assert riff_scan_ex(str(p), 8000)['n_frames'] == 50
    p.write_bytes(ref.wav_bytes('s24', _body('s24', 50, 2) + b'\1\2', 16000, 2, data_size=1 << 20))      # a partial last frame is dropped
    assert riff_scan_ex(str(p), 8000)['n_frames'] == 50
    # upsampling and the model rate itself; without `fs` the rate is not judged
    p.write_bytes(ref.wav_bytes('u8', _body('u8', 50, 1), 4000, 1))
    assert riff_scan_ex(str(p), 8000)['rate'] == 4000
    p.write_bytes(ref.wav_bytes('u8', _body('u8', 50, 1), 8001, 1))
    assert riff_scan_ex(str(p))['rate'] == 8001


def test_riff_scan_ex_refuses_by_name(nafp, tmp_path):
    from neural_audio_fp_amd.model.utils.audio_utils import riff_scan_ex
    p = tmp_path / 'f.wav'

    def refused(match, data, fs=8000):
        p.write_bytes(data)
        with pytest.raises(ValueError, match=match):
            riff_scan_ex(str(p), fs)

    body = _body('s16', 64, 1)
    refused(r'format tag 0x0006 \(A-law\)', ref.wav_bytes('u8', body, 8000, 1, tag=6))
    refused(r'format tag 0x0007 \(mu-law\)', ref.wav_bytes('u8', body, 8000, 1, tag=7))
    refused(r'format tag 0x0002 \(ADPCM\)', ref.wav_bytes('u8', body, 8000, 1, tag=2))
    refused(r'format tag 0x0055 \(MPEG layer 3\)', ref.wav_bytes('u8', body, 8000, 1, tag=0x55))
    refused(r'format tag 0x1234 is not taken', ref.wav_bytes('s16', body, 8000, 1, tag=0x1234))
    refused('0 channels; 1 to 8 are taken', ref.wav_bytes('s16', body, 8000, 0, align=2))
    refused('9 channels; 1 to 8 are taken', ref.wav_bytes('s16', _body('s16', 64, 9), 8000, 9))
    refused('9 channels; 1 to 8 are taken', ref.wav_bytes('s16', _body('s16', 64, 9), 8000, 9, extensible=True))
    refused('12-bit samples', ref.wav_bytes('s16', body, 8000, 1, bits=12))
    refused('block_align 4 != 1 channels \\* 2 bytes', ref.wav_bytes('s16', body, 8000, 1, align=4))
    refused('block_align 5 is not a multiple of 2 channels', ref.wav_bytes('s16', body, 8000, 2, extensible=True, align=5))
    refused('16-bit IEEE float', ref.wav_bytes('s16', body, 8000, 1, tag=3))
    refused('64-bit PCM', ref.wav_bytes('f64', _body('f64', 8, 1), 8000, 1, tag=1))
    refused('40-bit PCM', ref.wav_bytes('s16', _body('s16', 50, 1), 8000, 2, extensible=True, align=10))
    refused('unknown sub-format GUID', ref.wav_bytes('s16', body, 8000, 1, extensible=True, guid=bytes.fromhex('0600000000001000800000aa00389b71')))
    refused('unknown sub-format GUID', ref.wav_bytes('s16', body, 8000, 1, extensible=True, guid=b'\1\0' + b'\0' * 14))
    refused('^Sample rate should be 8000 but got 8001$', ref.wav_bytes('s16', body, 8001, 1))           # L = 8000 > 640
    refused('^Sample rate should be 16000 but got 11024$', ref.wav_bytes('s16', body, 11024, 1), fs=16000)
    refused('^Sample rate should be 8000 but got 200000$', ref.wav_bytes('s16', body, 200000, 1))
    refused('not a RIFF/WAVE file', b'RIFX' + ref.wav_bytes('s16', body, 8000, 1)[4:])
    refused('not a RIFF/WAVE file', b'ID3\x03')
    refused('no data chunk', ref.wav_bytes('s16', body, 8000, 1)[:36])


def _tree(tmp_path):
    """The mixed tree of the issue: 24-bit 48 kHz stereo, float32 44.1 kHz mono, 6 kHz 16-bit, 8-bit 8 kHz, and a native file."""
    spec = [('s24', 48000, 2, int(2.6 * 48000), True), ('f32', 44100, 1, 3 * 44100, False), ('s16', 6000, 1, 9000, False),
            ('u8', 8000, 1, 12345, False), ('s16', 8000, 1, 20000, False)]
    paths, bodies = [], []
    for i, (fmt, fs, ch, n, ext) in enumerate(spec):
        bodies.append(_body(fmt, n, ch, seed=i))
        paths.append(str(tmp_path / f'{i}.wav'))
        with open(paths[-1], 'wb') as f:
            f.write(ref.wav_bytes(fmt, bodies[-1], fs, ch, extensible=ext))
    return spec, paths, bodies


def test_without_the_switch_nothing_changes(nafp, tmp_path, monkeypatch):
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    from neural_audio_fp_amd.model.utils.dataloader_keras import PcmStore
    spec, paths, _ = _tree(tmp_path)
    want = ['^Sample rate should be 8000 but got 48000$', '^Sample rate should be 8000 but got 44100$',
            '^Sample rate should be 8000 but got 6000$', 'expected 16-bit mono PCM$']
    monkeypatch.delenv('NAFP_INGEST_ANY', raising=False)
    monkeypatch.delenv('NAFP_RESAMPLE', raising=False)
    for path, msg in zip(paths, want):
        for cls in (lambda f: SegmentSource([f], bsz=4), lambda f: PcmStore([f], 8000)):
            with pytest.raises(ValueError, match=msg):
                cls(path)
    src = SegmentSource([paths[4]], bsz=4)
    assert not src.ingest and not src.resample and len(next(src.iter_windows(0, src.n_samples, 1000))) == 6
    # NAFP_RESAMPLE=1 alone keeps its own refusals (24-bit; upsampling)
    monkeypatch.setenv('NAFP_RESAMPLE', '1')
    with pytest.raises(ValueError, match='16-bit PCM with 1 or 2 channels'):
        SegmentSource([paths[0]], bsz=4)
    with pytest.raises(ValueError, match='^Sample rate should be 8000 but got 6000$'):
        PcmStore([paths[2]], 8000)
    # the new switch, alone or with the old one: taken; what would materialise samples on the host raises
    for both in (False, True):
        monkeypatch.setenv('NAFP_INGEST_ANY', '1')
        if not both:
            monkeypatch.delenv('NAFP_RESAMPLE')
        src = SegmentSource(paths, bsz=4)
        assert src.ingest and src.resampled == [True, True, True, True, False]
        assert src.n_frames == [ref.n_out(n, fs, 8000) if i < 4 else n for i, (fmt, fs, ch, n, ext) in enumerate(spec)]
        with pytest.raises(NotImplementedError, match='no CPU path'):
            src.read_rows(0, 1)
        assert src.read_rows(src.n_samples - 1, src.n_samples).shape == (1, 1, 8000)       # the native file still reads on the host
        store = PcmStore(paths, 8000)
        assert list(store.n_frames) == src.n_frames
        from neural_audio_fp_amd.model.utils.dataloader_keras import PcmArena
        with pytest.raises(NotImplementedError, match='no CPU path'):
            PcmArena([store]).host()
        monkeypatch.setenv('NAFP_RESAMPLE', '1')
    from neural_audio_fp_amd.model.utils import ingest as ig
    assert ig.rates_summary(src) == {'files': 5, 'resampled': 4, 'rates': {'48000x2xs24': 1, '44100x1xf32': 1, '6000x1xs16': 1,
                                                                          '8000x1xu8': 1, '8000x1xs16': 1}}
    with pytest.raises(ValueError, match='^Sample rate should be 8000 but got 8001$'):
        p = tmp_path / 'odd.wav'
        p.write_bytes(ref.wav_bytes('s16', _body('s16', 100, 1), 8001, 1))
        SegmentSource([str(p)], bsz=4)


def test_pieces_of_iter_windows(nafp, tmp_path, monkeypatch):
    """With the switch on, a launch that holds a file to convert yields the BYTES its rows read -- nafp_ingest_input_range of each
    piece's outputs times block_align -- pieces that pass the kernel's own checks and cover every row's samples once, and windows
    that index the model-rate arena as without the switch."""
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    from neural_audio_fp_amd.model.utils import ingest as ig
    monkeypatch.setenv('NAFP_INGEST_ANY', '1')
    spec, paths, bodies = _tree(tmp_path)
    src = SegmentSource(paths, bsz=5)
    assert src.n_samples == sum(max(1, (n - 8000 + 4000) // 4000) for n in src.n_frames)
    code = {c: name for name, (c, w) in ref.FORMATS.items()}
    rows_seen = 0
    for rows_per_launch in (3, 1000):
        covered = np.zeros(src.n_samples, int)
        for start, n, arena, used, off, valid, work in src.iter_windows(0, src.n_samples, rows_per_launch):
            rows_seen += n
            if work is None:                                  # a launch of native rows only: today's arena
                f = int(np.searchsorted(src.file_first, start, side='right') - 1)
                assert not src.resampled[f]
                covered[start:start + n] += 1
                continue
            raw = arena.view(np.uint8)
            assert work.out_total % 8 == 0 and used % 8 == 0 and 2 * used <= len(raw)
            filled = np.zeros(work.out_total, int)
            for rate, pieces in work.by_rate.items():
                assert pieces.dtype.itemsize == 64
                ig.check_pieces(rate, 8000, pieces, 2 * used, work.out_total)
                for p in pieces:
                    f = [i for i, (fmt, fs, ch, n_in, ext) in enumerate(spec) if fs == rate and n_in == p['n_in']][0]
                    fmt, fs, ch, n_in, ext = spec[f]
                    assert (code[int(p['format'])], int(p['channels'])) == (fmt, ch)
                    assert p['raw_off'] % 16 == 0 and p['out_off'] % 8 == 0                # 16-byte aligned piece starts
                    first, last = ig.input_range(p['out0'], p['out0'] + p['n_out'], p['n_in'], rate, 8000)
                    assert (p['frame0'], p['frame0'] + p['n_frames']) == (first, last)     # (held to brute force in the test above)
                    align = ch * ref.FORMATS[fmt][1]
                    assert raw[p['raw_off']:p['raw_off'] + p['n_frames'] * align].tobytes() == bodies[f][first * align:last * align]
                    assert p['out0'] % src.hop_len == 0
                    filled[p['out_off']:p['out_off'] + p['n_out']] += 1
            assert filled.max() == 1                                                       # no output written twice
            assert np.all(off >= 0) and np.all(off + valid <= work.out_total)
            for o, v in zip(off, valid):
                assert filled[o:o + v].all()                                               # every sample a row reads is produced
            covered[start:start + n] += 1
        assert np.all(covered == 1)                                                        # the pieces cover every row once
    assert rows_seen == 2 * src.n_samples


def test_check_pieces_refuses_each_inconsistency(nafp):
    """Host only: the checks the kernel makes per piece.  (No inconsistent piece is ever launched.)"""
    lib = nafp._lib.load()
    from neural_audio_fp_amd.model.utils import ingest as ig
    fs_in, fs_out, n_in, ch = 48000, 8000, 6000, 3
    first, last = ig.input_range(0, 1000, n_in, fs_in, fs_out)
    assert (first, last) == ref.input_range(0, 1000, n_in, fs_in, fs_out)
    raw_size, out_samples = 17 + (last - first) * 9, 1008
    good = np.array([(17, first, last - first, n_in, 0, 8, 1000, ch, 3, 0)], dtype=ig.PIECE_DTYPE)       # 24-bit: an odd byte offset

    def status(p, raw=raw_size, out=out_samples):
        return lib.nafp_ingest_check_pieces_host(fs_in, fs_out, p.ctypes.data_as(ctypes.c_void_p), len(p), raw, out)

    assert status(good) == 0
    assert status(good, raw=raw_size - 1) == 1                       # the last frame's last byte is outside the raw arena
    assert status(good, out=1007) == 1
    for field, value, want in (('raw_off', -1, 1), ('raw_off', 18, 1), ('raw_off', raw_size + 1, 1), ('frame0', first + 1, 1),
                               ('n_frames', last - first - 1, 1), ('n_frames', n_in + 1, 1), ('n_frames', -1, 1), ('n_in', -1, 1),
                               ('n_in', last - 1, 1), ('out0', -1, 1), ('out0', 1, 1), ('out_off', -1, 1), ('out_off', 9, 1),
                               ('n_out', -1, 1), ('n_out', 1001, 1), ('channels', 0, 2), ('channels', 9, 2), ('channels', 4, 1),
                               ('format', 0, 2), ('format', 7, 2), ('format', 6, 1), ('format', 2, 0)):
        p = good.copy()
        p[field] = value
        assert status(p) == want, (field, value)
    assert status(good, raw=-1) == 1 and lib.nafp_ingest_check_pieces_host(fs_in, fs_out, None, 1, 16, 16) == 1
    assert lib.nafp_ingest_check_pieces_host(8000, 8001, good.ctypes.data_as(ctypes.c_void_p), 1, raw_size, out_samples) == 2
    assert lib.nafp_ingest_check_pieces_host(fs_in, fs_out, None, 0, 0, 0) == 0
    # beyond the file's output count
    n_total = ref.n_out(n_in, fs_in, fs_out)
    a, b = ig.input_range(n_total - 10, n_total, n_in, fs_in, fs_out)
    tail = np.array([(0, a, b - a, n_in, n_total - 10, 0, 10, ch, 3, 0)], dtype=ig.PIECE_DTYPE)
    assert status(tail, raw=(b - a) * 9, out=16) == 0
    tail['n_out'] = 11
    assert status(tail, raw=(b - a) * 9, out=16) == 1
    # struct check: ctypes sees the same 64 bytes
    assert struct.calcsize('<6q4i') == ig.PIECE_DTYPE.itemsize == 64
