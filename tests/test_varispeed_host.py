"""CPU: the varispeed contract (include/nafp.h, tests/_varispeed_ref.py) -- geometry, the host table against the restatement, the
output / input ranges against brute force, the restatement's accuracy against a float64 evaluation of the same filter, the choice
among speed hypotheses, the `--speeds` text, and the plans `SegmentSource(step=...)` makes.  No GPU call anywhere."""
import ctypes
import wave

import numpy as np
import pytest

import _varispeed_ref as ref

ONE = 1 << 24
STEPS = [ref.STEP_MIN, ref.STEP_MAX, ONE, ONE + 1, ref.step_for(1.04), ref.step_for(0.96), ref.step_for(1.0137)]


def _lib_table(lib, step):
    W, T = ref.geometry(step)
    out = np.zeros((ref.PHASES + 1, T), np.int32)
    assert lib.nafp_varispeed_table_host(step, out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out


def test_geometry(nafp):
    from neural_audio_fp_amd.model.utils import varispeed as vs
    assert vs.geometry(ONE) == (34, 68) and vs.geometry(ref.STEP_MIN) == (34, 68) and vs.geometry(ref.STEP_MAX) == (43, 86)
    for step in STEPS:
        assert vs.geometry(step) == ref.geometry(step)
        assert ref.geometry(step)[0] == int(np.ceil(32 / ref.two_fc(step) - 1e-12))
    assert (vs.STEP_MIN, vs.STEP_MAX) == (ref.STEP_MIN, ref.STEP_MAX) == (int(np.ceil(ONE * 0.8)), ONE * 5 // 4)
    lib = nafp._lib.load()
    for bad in (ref.STEP_MIN - 1, ref.STEP_MAX + 1, 0, 2 ** 32 - 1):
        assert lib.nafp_varispeed_geometry(bad, None, None) == 2
        with pytest.raises(ValueError, match='outside'):
            vs.geometry(bad)
    assert vs.step_for(1.04) == round(ONE / 1.04) and vs.step_for(0.8) == ref.STEP_MAX and vs.step_for(1.25) == ref.STEP_MIN
    assert vs.speed_of(vs.step_for(1.04)) == ONE / round(ONE / 1.04)
    for bad in (0.79, 1.26, float('nan')):
        with pytest.raises(ValueError, match='outside'):
            vs.step_for(bad)
    assert vs.PIECE_DTYPE.itemsize == 56


@pytest.mark.parametrize('step', [ref.STEP_MIN, ref.STEP_MAX, ONE, ref.step_for(1.04), ref.step_for(1.0137)])
def test_host_table_equals_the_restatement(nafp, step):
    got, want = _lib_table(nafp._lib.load(), step), ref.table(step)
    assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want)
    # the row p = 512 of tap t is the row p = 0 of tap t - 1: the table is one curve
    assert np.array_equal(want[512, 1:], want[0, :-1])
    gain = np.abs(want).sum(axis=1).max() / 2.0 ** 30
    assert 2.2 < gain < 2.5, gain
    dc = want.sum(axis=1) / 2.0 ** 30
    assert np.all(np.abs(dc - 1.0) < 1e-5), dc


def test_status_codes_without_gpu(nafp):
    lib = nafp._lib.load()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    h = ctypes.c_void_p()
    assert lib.nafp_varispeed_table_host(ONE, None) == 1 and lib.nafp_varispeed_table_host(1, None) == 2
    assert lib.nafp_varispeed_n_out(-1, ONE) == -1 and lib.nafp_varispeed_n_out(1 << 31, ONE) == -1 and lib.nafp_varispeed_n_out(5, 5) == -1
    assert lib.nafp_varispeed_n_out((1 << 31) - 1, ref.STEP_MIN) == ref.n_out((1 << 31) - 1, ref.STEP_MIN)
    assert lib.nafp_varispeed_input_range(0, 1, 10, 5, ctypes.byref(a), ctypes.byref(b)) == 2
    assert lib.nafp_varispeed_input_range(0, 1, 1 << 31, ONE, ctypes.byref(a), ctypes.byref(b)) == 2
    assert lib.nafp_varispeed_input_range(0, 1, 10, ONE, None, ctypes.byref(b)) == 1
    assert lib.nafp_varispeed_input_range(2, 1, 10, ONE, ctypes.byref(a), ctypes.byref(b)) == 1
    assert lib.nafp_varispeed_input_range(0, 1, -1, ONE, ctypes.byref(a), ctypes.byref(b)) == 1
    assert lib.nafp_varispeed_check_pieces_host(5, None, 0, 0, 0) == 2
    assert lib.nafp_varispeed_check_pieces_host(ONE, None, 1, 0, 0) == 1 and lib.nafp_varispeed_check_pieces_host(ONE, None, -1, 0, 0) == 1
    assert lib.nafp_varispeed_check_pieces_host(ONE, None, 0, 0, 0) == 0
    assert lib.nafp_varispeed_create(None, ONE) == 1
    assert lib.nafp_varispeed_create(ctypes.byref(h), ref.STEP_MAX + 1) == 2 and not h.value
    assert lib.nafp_varispeed_destroy(None) == 0
    assert lib.nafp_varispeed_i16(None, None, 0, None, 0, None, 0, None) == 1


@pytest.mark.parametrize('step', [ref.STEP_MIN, ref.STEP_MAX, ONE + 1, ref.step_for(1.04)])
def test_ranges_against_brute_force(nafp, step):
    from neural_audio_fp_amd.model.utils import varispeed as vs
    W, T = ref.geometry(step)
    for n_in in (1, 2, 2 * W - 1, 2 * W, 1000):
        n_total = vs.n_out(n_in, step)
        assert n_total == ref.n_out(n_in, step)
        # every output index below n_out falls inside the file, the next one does not
        assert ((n_total - 1) * step) >> 24 < n_in <= (n_total * step + ONE - 1) >> 24
        # the samples each output reads, by the definition; a range of outputs reads their union
        j = np.arange(n_in)[None, :]
        pos = ((np.arange(n_total, dtype=np.int64) * step) >> 24)[:, None]
        reads = np.concatenate([np.zeros((1, n_in), np.int64), np.cumsum((j >= pos - W + 1) & (j <= pos + W), axis=0)])
        pairs = [(a, b) for a in range(n_total + 1) for b in range(a, n_total + 1)] if n_in < 1000 else \
                [(a, b) for a in range(0, n_total + 1, 97) for b in range(a, n_total + 1, 89)]
        for a, b in pairs:
            got, idx = vs.input_range(a, b, n_in, step), np.flatnonzero(reads[b] - reads[a])
            if len(idx) == 0:
                assert got[0] == got[1] and 0 <= got[0] <= n_in, (a, b, n_in, got)
            else:
                assert got == (idx[0], idx[-1] + 1), (a, b, n_in, got)
        for a, b in pairs[::53]:
            want = ref.input_range(a, b, n_in, step)
            assert want == (None if a == b else vs.input_range(a, b, n_in, step)), (a, b, n_in)


def _interpolation_bound(tab, T):
    """What a straight line between two neighbouring rows can miss of the curve, in units of 2^-30, summed over the taps of ONE
    output: all its T taps share one phase p, so the term is the maximum over p of sum_t e[p][t], where e[p][t] = (the larger
    |second difference| at the two ends of the interval [p, p + 1] of tap t) / 8.  The table is one curve (row 512 of tap t is row 0
    of tap t - 1), along which the second differences are taken; one of rounded entries is off by at most 2."""
    curve = np.concatenate([tab[:512, t] for t in range(T - 1, -1, -1)] + [tab[512:, 0]]).astype(np.float64)
    d2 = np.abs(curve[:-2] - 2 * curve[1:-1] + curve[2:]) + 2.0
    d2 = np.concatenate([[d2[0]], d2, [d2[-1]]])                  # one per curve point k = (T - 1 - t) * 512 + p
    ends = np.maximum(d2[:-1], d2[1:])                            # per interval [k, k + 1]
    return ends.reshape(T, 512).sum(axis=0).max() / 8.0


@pytest.mark.parametrize('speed', [0.8, 0.96, 1.0137, 1.04, 1.25])
def test_restatement_against_float64(speed):
    """|y - float64 evaluation of the same h| on full-scale noise.  The bound, in LSB, from the table itself: 0.5 for the final
    rounding; per tap 2^-30 for the rounding of the table entries (0.5 from the two rows' blend) and of the blended coefficient
    (0.5), times |x| <= 2^15: T * 2^-15; and the interpolation term above, times 2^15 / 2^30.  The whole has to come out near
    0.6 - 0.7 LSB; anything else means the table or this derivation is wrong."""
    step = ref.step_for(speed)
    W, T = ref.geometry(step)
    x = np.random.default_rng(11).integers(-32768, 32768, size=20000).astype(np.int16)
    tab = ref.table(step)
    acc = ref.accumulate(x, step, tab)
    f = ref.evaluate_float(x, step)
    before = np.abs(acc / 2.0 ** 30 - f).max()
    after = np.abs(ref.unclamped(acc) - f).max()
    interp = _interpolation_bound(tab, T) * 2.0 ** -15
    bound = 0.5 + T * 2.0 ** -15 + interp
    print(f'speed {speed}: before rounding {before:.4f} LSB, after {after:.4f}, bound {bound:.4f} (interpolation {interp:.4f})')
    assert 0.6 <= bound <= 0.72, bound
    assert before <= bound - 0.5 and after <= bound


@pytest.mark.parametrize('speed', [0.96, 1.04])
@pytest.mark.parametrize('freq', [1000.0, 3400.0])
def test_sines(speed, freq):
    """A 20000-amplitude sine comes out as the sine at freq * sigma: amplitude within 0.5 %, residual at most 0.5 LSB rms (the
    final rounding alone gives 0.289)."""
    step = ref.step_for(speed)
    W, T = ref.geometry(step)
    n = np.arange(20000)
    x = np.round(20000 * np.sin(2 * np.pi * freq / 8000.0 * n))
    y = ref.varispeed(x.astype(np.int16), step).astype(np.float64)
    m = np.arange(len(y))[2 * W:-2 * W]                               # away from the file's ends
    ph = 2 * np.pi * freq / 8000.0 * (m * step / ONE)
    A = np.stack([np.sin(ph), np.cos(ph)], axis=1)
    coef, *_ = np.linalg.lstsq(A, y[m], rcond=None)
    amp = np.hypot(*coef)
    # the input is itself rounded to integers (0.289 LSB rms of white error, which the filter passes with gain <= 1)
    resid = np.sqrt(np.mean((y[m] - A @ coef) ** 2))
    print(f'speed {speed}, {freq} Hz: amplitude {amp:.2f}, residual {resid:.4f} LSB rms')
    assert abs(amp / 20000 - 1) < 0.005 and resid <= 0.5


def _m(rec, a, b, score, speed, track='t'):
    return {'recording': rec, 'recording_span_s': [a, b], 'score': score, 'speed': speed, 'track': track}


def test_select_across_speeds(nafp):
    from neural_audio_fp_amd.eval.identify import select_across_speeds as sel
    assert sel([]) == []
    # the best score wins a contested span, whatever the order given
    a, b, c = _m('r', 0, 8, 0.85, 1.0), _m('r', 0, 7.7, 0.99, 1.04), _m('r', 0, 8.3, 0.83, 0.96)
    assert sel([a, b, c]) == [b] and sel([c, b, a]) == [b]
    # ties on the score: the speed nearer to 1 in log terms, then the lower speed, then the earlier start
    assert sel([_m('r', 0, 8, 0.9, 1.04), _m('r', 0, 8, 0.9, 1.02)])[0]['speed'] == 1.02
    lo, hi = _m('r', 0, 8, 0.9, 0.5), _m('r', 0, 8, 0.9, 2.0)           # |log| equal exactly: the lower speed
    assert sel([hi, lo]) == [lo]
    e1, e2 = _m('r', 4, 12, 0.9, 1.0, 'x'), _m('r', 0, 8, 0.9, 1.0, 'y')  # all equal but the start; they overlap by exactly half
    assert sel([e1, e2]) == [e2, e1]
    # the half-overlap rule: more than half of the SHORTER span
    long_, short_in, short_edge = _m('r', 0, 20, 0.9, 1.0), _m('r', 2, 6, 0.8, 1.04), _m('r', 18, 22, 0.8, 1.04)
    assert sel([long_, short_in]) == [long_]                           # 4 of 4 s overlap
    assert sel([long_, short_edge]) == [long_, short_edge]             # 2 of 4 s: exactly half is kept
    assert sel([long_, _m('r', 17.9, 21.9, 0.8, 1.04)]) == [long_]
    # two tracks in one recording at different speeds, and another recording untouched by them
    t0 = [_m('r', 0, 6, 0.99, 0.96, 'A'), _m('r', 0, 6.2, 0.84, 1.0, 'A'), _m('r', 0, 6.5, 0.80, 1.04, 'B')]
    t1 = [_m('r', 6, 12, 0.98, 1.04, 'C'), _m('r', 6.2, 12.5, 0.85, 1.0, 'C'), _m('r', 6.4, 13, 0.81, 0.96, 'D')]
    other = [_m('q', 0, 8, 0.5, 1.0, 'E')]
    got = sel(t0[1:] + other + t1[::-1] + t0[:1])
    assert got == [t0[0], t1[0], other[0]]                             # recordings in order of first appearance, then by start
    assert all('speed' in m for m in got)
    # one path given twice: the two recordings are told apart by their place, and do not compete
    twice = [dict(_m('r', 0, 8, 0.9, 1.0), _rec=0), dict(_m('r', 0, 8, 0.8, 1.04), _rec=1)]
    assert sel(twice) == twice and sel([_m('r', 0, 8, 0.9, 1.0), _m('r', 0, 8, 0.8, 1.04)]) == [_m('r', 0, 8, 0.9, 1.0)]


def test_speed_spec(nafp):
    from neural_audio_fp_amd.eval.identify import MAX_SPEEDS, parse_speeds
    got = parse_speeds('0.96,1,1.04')
    assert [s for s, _ in got] == [round(ONE / 0.96), ONE, round(ONE / 1.04)]
    assert [v for _, v in got] == [ONE / round(ONE / 0.96), 1.0, ONE / round(ONE / 1.04)]
    rng = parse_speeds('0.94:1.06:0.01')
    assert len(rng) == 13 and rng[0][0] == round(ONE / 0.94) and rng[6][0] == ONE and rng[-1][0] == round(ONE / 1.06)
    assert [s for s, _ in parse_speeds(' 1 , 0.99:1.01:0.01, 1.0')] == [ONE, round(ONE / 0.99), round(ONE / 1.01)]      # named twice, kept once
    assert len(parse_speeds('0.8:1.25:0.0075')) == 61 and parse_speeds('0.8,1.25') == [(ref.STEP_MAX, 0.8), (ref.STEP_MIN, ONE / ref.STEP_MIN)]
    assert len(parse_speeds(','.join(str(0.9 + 0.001 * k) for k in range(MAX_SPEEDS)))) == MAX_SPEEDS
    for bad, word in (('', 'not a speed'), ('fast', 'not a speed'), ('1,,1.04', 'not a speed'), ('0.9:1.1', 'not a speed'),
                      ('0.9:1.1:0.1:3', 'not a speed'), ('1.1:0.9:0.01', 'lo <= hi'), ('0.9:1.1:0', 'inc > 0'), ('0.9:1.1:-0.1', 'inc > 0'),
                      ('0.79', 'outside'), ('1,1.26', 'outside'), ('0.7:1.0:0.1', 'outside'), ('nan', 'outside'), ('inf', 'outside'),
                      ('0.9:inf:0.1', 'outside'), ('0.9:1.1:nan', 'outside'), ('0.9:1.1:1e-320', 'at most 64'), ('-inf:1:0.1', 'outside'),
                      ('0.9:1.1:0.001', 'at most 64'), (','.join(str(0.9 + 0.001 * k) for k in range(MAX_SPEEDS + 1)), 'at most 64')):
        with pytest.raises(ValueError, match=word):
            parse_speeds(bad)


def test_identify_refuses_a_bad_spec_first(nafp, cfg):
    """Before the library is looked for, let alone a GPU call: the paths below do not exist."""
    from neural_audio_fp_amd.eval.identify import identify
    for bad, word in (('1.3', 'outside'), ('0.9:1.1:0.001', 'at most 64'), ('x', 'not a speed')):
        with pytest.raises(SystemExit, match=word):
            identify(cfg, 'no_such_experiment', '1', ['/nonexistent/recording.wav'], emb_dir='/nonexistent/emb/', speeds=bad)


def _wav(path, pcm, fs=8000, channels=1):
    with wave.open(str(path), 'w') as w:
        w.setnchannels(channels); w.setsampwidth(2); w.setframerate(fs)
        w.writeframes(np.asarray(pcm).astype('<i2').tobytes())


@pytest.mark.parametrize('speed', [1.04, 0.96])
def test_segment_source_under_a_step(nafp, tmp_path, monkeypatch, speed):
    """Geometry and launches of SegmentSource(step=...) on native files: file lengths, segment counts and windows follow the
    stretched lengths; every launch reads exactly the model-rate samples input_range names, its pieces pass the kernel's checks,
    and the restatement run on those pieces alone gives the windows of the whole file's stretched stream."""
    from neural_audio_fp_amd.model.utils import varispeed as vs
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource, n_segments
    for k in ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS', 'NAFP_INGEST_FLAC'):
        monkeypatch.delenv(k, raising=False)
    rng = np.random.default_rng(5)
    pcm = [rng.integers(-32768, 32768, size=n).astype(np.int16) for n in (30011, 7000, 12345, 1)]
    fns = []
    for i, x in enumerate(pcm):
        fns.append(str(tmp_path / f'{i}.wav'))
        _wav(fns[-1], x)
    step = vs.step_for(speed)
    plain = SegmentSource(fns, 4)
    src = SegmentSource(fns, 4, step=step)
    assert plain.step is None and src.step == step
    assert src.n_model == [len(x) for x in pcm] == plain.n_frames
    assert src.n_frames == [ref.n_out(len(x), step) for x in pcm]
    assert list(np.diff(src.file_first)) == [n_segments(n) for n in src.n_frames] and src.n_samples == int(src.file_first[-1])
    assert len(next(plain.iter_windows(0, plain.n_samples, 1000))) == 6         # without a step: nothing new
    for call in (lambda: src.read_rows(0, 2), lambda: src[0], lambda: next(src.iter_rows(0, 2, 2))):
        with pytest.raises(NotImplementedError, match='no CPU path'):
            call()
    with pytest.raises(ValueError, match='outside'):
        SegmentSource(fns, 4, step=ref.STEP_MAX + 1)
    want = [ref.varispeed(x, step) for x in pcm]
    for rows in (3, 7, 1000):
        seen = 0
        for start, n, arena, used, off, valid, work in src.iter_windows(0, src.n_samples, rows):
            assert start == seen and isinstance(work, vs.Stage) and work.inner is None and work.step == step
            pieces = vs.check_pieces(step, work.pieces, used, work.out_total)
            out = np.full(work.out_total, 77, np.int16)
            for pc in pieces:
                first, last = vs.input_range(pc['out0'], pc['out0'] + pc['n_out'], pc['n_in'], step) if pc['n_out'] else (0, 0)
                assert (pc['frame0'], pc['frame0'] + pc['n_frames']) == (first, last) and pc['src_off'] % 8 == 0 and pc['out_off'] % 8 == 0
                f = [len(x) for x in pcm].index(pc['n_in'])
                assert np.array_equal(arena[pc['src_off']:pc['src_off'] + pc['n_frames']], pcm[f][first:last])
                held = np.zeros(pc['n_in'], np.int16)                            # only what the launch read, zeros elsewhere
                held[first:last] = arena[pc['src_off']:pc['src_off'] + pc['n_frames']]
                out[pc['out_off']:pc['out_off'] + pc['n_out']] = ref.finish(ref.accumulate(held, step, n=np.arange(pc['out0'], pc['out0'] + pc['n_out'])))
            for i in range(n):
                f = int(np.searchsorted(src.file_first, start + i, side='right') - 1)
                k = start + i - int(src.file_first[f])
                seg = np.zeros(src.seg_len, np.int16)
                seg[:valid[i]] = out[off[i]:off[i] + valid[i]]
                full = np.zeros(src.seg_len, np.int16)
                part = want[f][k * src.hop_len:k * src.hop_len + src.seg_len]
                full[:len(part)] = part
                assert np.array_equal(seg, full), (rows, start, i)
            seen += n
        assert seen == src.n_samples


def test_segment_source_under_a_step_with_files_to_convert(nafp, tmp_path, monkeypatch):
    """A launch that holds a file the device converts: the model-rate samples of every piece are planned through
    ingest.LaunchPlan.add, as the outputs of a launch without a step are, and the varispeed stage reads the arena they fill."""
    from neural_audio_fp_amd.model.utils import ingest as ig
    from neural_audio_fp_amd.model.utils import varispeed as vs
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    for k in ('NAFP_RESAMPLE', 'NAFP_INGEST_CODECS', 'NAFP_INGEST_FLAC'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('NAFP_INGEST_ANY', '1')
    rng = np.random.default_rng(6)
    _wav(tmp_path / 'a.wav', rng.integers(-32768, 32768, size=2 * 66150), fs=44100, channels=2)
    _wav(tmp_path / 'b.wav', rng.integers(-32768, 32768, size=9000))
    fns = [str(tmp_path / 'a.wav'), str(tmp_path / 'b.wav')]
    step = vs.step_for(1.04)
    src, plain = SegmentSource(fns, 4, step=step), SegmentSource(fns, 4)
    assert src.n_model == plain.n_frames == [12000, 9000] and src.n_frames == [ref.n_out(12000, step), ref.n_out(9000, step)]
    for start, n, arena, used, off, valid, work in src.iter_windows(0, src.n_samples, 5):
        assert isinstance(work, vs.Stage) and isinstance(work.inner, ig.ChunkPieces)
        pieces = vs.check_pieces(step, work.pieces, work.inner.out_total, work.out_total)
        inner = {(int(p['out_off']), int(p['out0']), int(p['n_out'])) for rows in work.inner.by_rate.values() for p in rows}
        assert inner == {(int(p['src_off']), int(p['frame0']), int(p['n_frames'])) for p in pieces}
        for rate, rows in work.inner.by_rate.items():
            ig.check_pieces(rate, 8000, rows, 2 * used, work.inner.out_total)
