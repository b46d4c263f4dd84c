"""CPU: the host side of the resampler (include/nafp.h `nafp_resample_*`, model/utils/resample.py) against the numpy
restatement tests/_resample_ref.py -- geometry, the quantised filter and its response, the input ranges, the refusals, and the
pieces SegmentSource hands to the device.  No GPU call."""
import ctypes
import wave

import numpy as np
import pytest

import _resample_ref as ref


def _geometry(lib, fs_in, fs_out=8000):
    v = [ctypes.c_int() for _ in range(4)]
    st = lib.nafp_resample_geometry(fs_in, fs_out, *[ctypes.byref(x) for x in v])
    return st, tuple(x.value for x in v)


def _table(lib, fs_in, fs_out=8000):
    st, (L, M, half, T) = _geometry(lib, fs_in, fs_out)
    assert st == 0
    tab = np.zeros((L, T), np.int32)
    assert lib.nafp_resample_table_host(fs_in, fs_out, tab.ctypes.data_as(ctypes.c_void_p)) == 0
    return tab


def _write_wav(path, pcm, fs, channels=1, width=2):
    with wave.open(str(path), 'w') as w:
        w.setnchannels(channels); w.setsampwidth(width); w.setframerate(fs)
        w.writeframes(np.asarray(pcm).astype('<i2' if width == 2 else 'u1').tobytes())


def test_geometry_is_the_issue_table(nafp):
    lib = nafp._lib.load()
    want = {44100: (80, 441, 14855, 372), 48000: (1, 6, 203, 407), 11025: (320, 441, 14855, 93)}
    for fs, g in want.items():
        assert _geometry(lib, fs) == (0, g)
        assert ref.geometry(fs) == g
        assert g[0] * g[3] == {44100: 29760, 48000: 407, 11025: 29760}[fs]
    for fs in (12000, 16000, 22050, 24000, 32000, 88200, 96000, 176400, 192000):
        assert _geometry(lib, fs) == (0, ref.geometry(fs))
    assert _geometry(lib, 8000) == (0, (1, 1, 0, 1))                  # the channel average alone


@pytest.mark.parametrize('fs', [44100, 48000, 11025, 16000, 22050, 192000])
def test_table_is_the_float64_design(nafp, fs):
    tab = _table(nafp._lib.load(), fs).astype(np.int64)
    # the library's I0 / sin and numpy's may differ in the last bit: +-1 unit of 2^-30, not equality
    assert np.abs(tab - ref.table(fs)).max() <= 1
    assert np.abs(tab.sum(axis=1) / 2.0 ** 30 - 1.0).max() < 1e-5
    assert (np.abs(tab).sum(axis=1) / 2.0 ** 30).max() < 2.3       # |acc| < 2.3 * 2^30 * 2^16 < 2^47
    L, M, half, T = ref.geometry(fs)
    flat = tab.T.reshape(-1)                                         # index p + t L = v + half
    assert not flat[2 * half + 1:].any() and np.array_equal(flat[:2 * half + 1], flat[:2 * half + 1][::-1])


@pytest.mark.parametrize('fs', [44100, 48000, 11025, 16000])
def test_response_of_the_quantised_table(nafp, fs):
    """From the library's table by an FFT at the virtual rate: flat to 0.001 dB up to 3400 Hz, at most -85 dB from 4200 Hz
    (measured while the contract was written: 0.00038 dB and -87.4 dB; the margins cover a +-1 table)."""
    tab = _table(nafp._lib.load(), fs).astype(np.float64)
    L, M, half, T = ref.geometry(fs)
    h = tab.T.reshape(-1)[:2 * half + 1] / 2.0 ** 30 / L             # unit DC gain
    fv = fs * L
    n_fft = 1 << int(np.ceil(np.log2(len(h) * 16)))
    H = np.abs(np.fft.rfft(h, n_fft))
    f = np.arange(len(H)) * fv / n_fft
    db = 20 * np.log10(np.maximum(H, 1e-30))
    assert np.abs(db[f <= 3400]).max() <= 0.001
    assert db[f >= 4200].max() <= -85.0


def test_restatement_equals_the_definition():
    """The table form (phase p, taps t) the tests compare the GPU with == the definition sum_j hq[n M - j L] m[j]."""
    rng = np.random.default_rng(0)
    for fs, n in ((44100, 1000), (11025, 300), (48000, 1500), (16000, 700), (8000, 50)):
        x = rng.integers(-32768, 32768, size=n).astype(np.int16)
        assert np.array_equal(ref.accumulate(x, fs), ref.accumulate_by_definition(x, fs))
        x2 = rng.integers(-32768, 32768, size=(n, 2)).astype(np.int16)
        assert np.array_equal(ref.accumulate(x2, fs), ref.accumulate_by_definition(x2, fs))
    x2 = rng.integers(-32768, 32768, size=(64, 2)).astype(np.int16)
    assert np.array_equal(ref.resample(x2, 8000), (x2.astype(np.int64).sum(1) + 1) >> 1)
    # 11,025 frames of full-range noise at 44100 Hz: the integer result is the rounding of the float64 convolution
    x = rng.integers(-32768, 32768, size=11025).astype(np.int16)
    acc = ref.accumulate(x, 44100)
    assert np.abs(acc).max() < 2 ** 47
    assert np.array_equal(ref.finish(acc, 1), np.clip(np.floor(acc / 2.0 ** 30 + 0.5), -32768, 32767).astype(np.int16))


def test_input_range_and_n_out_against_brute_force(nafp):
    from neural_audio_fp_amd.model.utils import resample as rs
    for fs in (44100, 48000, 11025):
        for n_in in (0, 1, 5, 185, 186, 441, 4410):
            no = ref.n_out(n_in, fs)
            assert rs.n_out(n_in, fs, 8000) == no
            grid = sorted({g for g in (0, 1, 2, 33, no // 2, no - 1, no) if 0 <= g <= no})
            for n0 in grid:
                for n1 in grid:
                    if n1 < n0:
                        continue
                    got, want = rs.input_range(n0, n1, n_in, fs, 8000), ref.input_range(n0, n1, n_in, fs)
                    if want is None:
                        assert got[0] == got[1], (fs, n_in, n0, n1, got)
                    else:
                        assert got == want, (fs, n_in, n0, n1, got, want)
    lib = nafp._lib.load()
    assert lib.nafp_resample_n_out(-1, 44100, 8000) == -1 and lib.nafp_resample_n_out(10, 4000, 8000) == -1
    a, b = ctypes.c_int64(), ctypes.c_int64()
    assert lib.nafp_resample_input_range(5, 4, 100, 44100, 8000, ctypes.byref(a), ctypes.byref(b)) == 1
    assert lib.nafp_resample_input_range(0, 4, 100, 44100, 8000, None, None) == 1


def test_refusals(nafp, tmp_path, monkeypatch):
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    from neural_audio_fp_amd.model.utils.dataloader_keras import PcmStore, PcmArena
    lib = nafp._lib.load()
    assert _geometry(lib, 8001)[0] == 2 and _geometry(lib, 4000)[0] == 2         # L = 8000; upsampling
    assert _geometry(lib, 200000)[0] == 2 and _geometry(lib, 0)[0] == 1
    h = ctypes.c_void_p()
    assert lib.nafp_resample_create(ctypes.byref(h), 8001, 8000) == 2 and not h.value      # before any GPU call
    assert lib.nafp_resample_create(None, 44100, 8000) == 1
    assert lib.nafp_resample_table_host(44100, 8000, None) == 1
    assert lib.nafp_resample_i16(None, None, 0, None, 0, None, 0, None) == 1
    piece = np.zeros(1, nafp._lib.RESAMPLE_PIECE_DTYPE)
    piece['channels'] = 3
    assert lib.nafp_resample_check_pieces_host(44100, 8000, piece.ctypes.data_as(ctypes.c_void_p), 1, 16, 16) == 2
    rng = np.random.default_rng(1)
    files = {}
    for name, fs, ch, width in (('k16', 16000, 1, 2), ('odd', 8001, 1, 2), ('low', 4000, 1, 2), ('ch3', 44100, 3, 2), ('u8', 44100, 1, 1)):
        files[name] = str(tmp_path / f'{name}.wav')
        _write_wav(files[name], rng.integers(-100, 100, size=3000 * ch), fs, ch, width)
    # without the switch: exactly today's message, from both loaders
    monkeypatch.delenv('NAFP_RESAMPLE', raising=False)
    with pytest.raises(ValueError, match='^Sample rate should be 8000 but got 16000$'):
        SegmentSource([files['k16']], bsz=4)
    with pytest.raises(ValueError, match='^Sample rate should be 8000 but got 16000$'):
        PcmStore([files['k16']], 8000)
    monkeypatch.setenv('NAFP_RESAMPLE', '1')
    for cls in (lambda f: SegmentSource([f], bsz=4), lambda f: PcmStore([f], 8000)):
        with pytest.raises(ValueError, match='Sample rate should be 8000 but got 8001'):
            cls(files['odd'])
        with pytest.raises(ValueError, match='Sample rate should be 8000 but got 4000'):
            cls(files['low'])
        with pytest.raises(ValueError, match='16-bit PCM with 1 or 2 channels'):
            cls(files['ch3'])
        with pytest.raises(ValueError, match='16-bit PCM with 1 or 2 channels'):
            cls(files['u8'])
    # accepted; what would materialise samples on the host raises: there is no CPU resampler
    src = SegmentSource([files['k16']], bsz=4)
    assert src.n_frames == [1500] and src.n_samples == 1
    with pytest.raises(NotImplementedError):
        src.read_rows(0, 1)
    with pytest.raises(NotImplementedError):
        next(src.iter_rows(0, 1, 1))
    store = PcmStore([files['k16']], 8000)
    assert int(store.n_frames[0]) == 1500 and store.end == 1504
    with pytest.raises(NotImplementedError):
        PcmArena([store]).host()


def test_pieces_of_iter_windows(nafp, tmp_path, monkeypatch):
    """With the switch on, a launch that holds a file to resample yields the raw frames its rows read -- exactly
    nafp_resample_input_range of each piece's outputs -- and windows that index the model-rate arena."""
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    from neural_audio_fp_amd.model.utils import resample as rs
    monkeypatch.setenv('NAFP_RESAMPLE', '1')
    rng = np.random.default_rng(2)
    spec = [(44100, 2, 6 * 44100), (8000, 1, 20000), (48000, 1, int(3.2 * 48000)), (11025, 1, 3000), (8000, 2, 9000)]
    paths, pcm = [], []
    for i, (fs, ch, n) in enumerate(spec):
        x = rng.integers(-32768, 32768, size=(n, ch)).astype(np.int16)
        paths.append(str(tmp_path / f'{i}.wav')); pcm.append(x)
        _write_wav(paths[-1], x.reshape(-1), fs, ch)
    src = SegmentSource(paths, bsz=5)
    assert src.n_frames == [ref.n_out(n, fs) if (fs, ch) != (8000, 1) else n for fs, ch, n in spec]
    assert src.resampled == [True, False, True, True, True]
    assert src.n_samples == 11 + 4 + 5 + 1 + 1
    rows_seen = 0
    for rows_per_launch in (7, 1000):
        for start, n, arena, used, off, valid, work in src.iter_windows(0, src.n_samples, rows_per_launch):
            rows_seen += n
            if work is None:                                  # a launch of 8 kHz mono rows only: today's arena
                f = int(np.searchsorted(src.file_first, start, side='right') - 1)
                assert not src.resampled[f]
                continue
            assert work.out_total % 8 == 0 and used % 8 == 0
            ends = []
            for rate, pieces in work.by_rate.items():
                rs.check_pieces(rate, 8000, pieces, used, work.out_total)
                for p in pieces:
                    f = [i for i, (fs, ch, n_in) in enumerate(spec) if fs == rate and n_in == p['n_in'] and ch == p['channels']][0]
                    assert p['raw_off'] % 8 == 0 and p['out_off'] % 8 == 0           # 16-byte aligned piece starts
                    first, last = rs.input_range(p['out0'], p['out0'] + p['n_out'], p['n_in'], rate, 8000)
                    assert (p['frame0'], p['frame0'] + p['n_frames']) == (first, last)
                    want = ref.input_range(int(p['out0']), int(p['out0'] + p['n_out']), int(p['n_in']), rate)
                    assert want == (first, last)
                    ch = int(p['channels'])
                    got = np.asarray(arena[p['raw_off']:p['raw_off'] + p['n_frames'] * ch]).reshape(-1, ch)
                    assert np.array_equal(got, pcm[f][first:last])
                    assert p['out0'] % src.hop_len == 0
                    ends.append((int(p['out_off']), int(p['out_off'] + p['n_out'])))
            ends.sort()
            assert all(a1 <= b0 for (_, a1), (b0, _) in zip(ends, ends[1:])) and ends[-1][1] <= work.out_total
            assert np.all(off >= 0) and np.all(off + valid <= work.out_total)
    assert rows_seen == 2 * src.n_samples
    # rows of one file cut differently read different raw ranges but the same outputs: windows are placed as without resampling
    monkeypatch.delenv('NAFP_RESAMPLE')
    plain = SegmentSource([paths[1]], bsz=5)
    assert len(next(plain.iter_windows(0, plain.n_samples, 1000))) == 6
