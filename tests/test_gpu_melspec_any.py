"""GPU: the general log-mel front end (csrc/melspec_any.hip, nafp_melspec_create_ex) against the float64 oracle at geometries the
tuned kernel refuses, and the contract it shares with the tuned kernel: int16 == float32 input, windows == rows, the deferred
tail, launch independence, a NaN segment, the opt-in, and `generate` on a 16 kHz model.

Bounds: 2e-5 on the log-mel is the project's own bound for this layer (test_melspec_matches_oracle); the oracle's float32
restatement stays within 1.2e-6 of its float64 form at every geometry below, so the margin is the same ~20x.  1e-4 for
melspec_maxnorm, 1e-5 on 1 - cos end to end and 1e-6 next to a NaN segment are the bounds of the tests named next to them."""
import copy
import functools
import json
import wave

import numpy as np
import pytest
import torch

from oracle import melspec as o_mel, nnfp as o_nnfp, segments as o_seg
import _inputs

pytestmark = pytest.mark.gpu

ANY, FORCE = 1, 2
# (fs, seg_len, n_fft, hop, n_mels, f_min, f_max) -> (n_mels, n_frames)
GEOM = {
    'A': ((8000, 8000, 512, 256, 256, 300., 4000.), (256, 32)),        # smaller FFT
    'B': ((16000, 16000, 2048, 512, 256, 300., 8000.), (256, 32)),     # the 16 kHz model, 22-tap filters
    'C': ((8000, 8000, 1024, 256, 100, 300., 4000.), (100, 32)),       # 21-tap filters, n_mels not a multiple of 64
    'D': ((8000, 1001, 256, 100, 40, 0., 4000.), (40, 11)),            # hop no power of two and no divisor of n_fft, odd frames / length
    'E': ((16000, 16000, 4096, 1024, 128, 50., 8000.), (128, 16)),     # largest FFT, 94-tap filters
    'H': ((8000, 2000, 256, 64, 256, 300., 4000.), (256, 32)),         # 63 empty filters
    'L': ((16000, 16000, 256, 64, 64, 300., 8000.), (64, 251)),        # many frame chunks, ragged last one
    'S': ((8000, 300, 512, 128, 64, 300., 4000.), (64, 3)),            # segment shorter than the window
    'F': ((8000, 1000, 128, 50, 21, 0., 4000.), (21, 21)),             # smallest FFT (odd log2, 8 pairs side by side); 441 values per
                                                                       # segment, no multiple of 4: the scalar tail kernel
    'base': ((8000, 8000, 1024, 256, 256, 300., 4000.), (256, 32)),
}


def _audio(B, seed, T, fs):
    """The recipe of test_gpu_parity_forward._audio at any rate: noise plus three sines up to 0.4875 fs."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / float(fs)
    x = 0.1 * rng.normal(size=(B, 1, T))
    for b in range(B):
        f = rng.uniform(300, 0.4875 * fs, size=3)
        x[b, 0] += sum(0.2 * np.sin(2 * np.pi * fi * t + rng.uniform(0, 6.28)) for fi in f)
    return x.astype(np.float32)


def _layer(nafp, tag, flags=ANY, segment_norm=False):
    fs, seg_len, n_fft, hop, n_mels, f_min, f_max = GEOM[tag][0]
    return nafp.Melspec_layer(input_shape=(1, seg_len), segment_norm=segment_norm, n_fft=n_fft, stft_hop=hop, n_mels=n_mels, fs=fs,
                              dur=seg_len / fs, f_min=f_min, f_max=f_max, plan_flags=flags)


@functools.lru_cache(maxsize=None)
def _case(tag, B=5, group=2, segment_norm=False):
    """(input, float64 oracle output): computed once per geometry, shared, never written to."""
    fs, seg_len, n_fft, hop, n_mels, f_min, f_max = GEOM[tag][0]
    x = _audio(B, seed=sum(map(ord, tag)), T=seg_len, fs=fs)
    want = o_mel.melspec_layer(x, fs, n_fft, hop, n_mels, f_min, f_max, segment_norm=segment_norm, group_size=group, dtype=np.float64)
    want.setflags(write=False)
    return _Frozen(x), want


class _Frozen:
    """A shared input nobody can write to: tests take a fresh copy (numpy or device) of it."""

    def __init__(self, x):
        self._x = x

    def numpy(self):
        return self._x.copy()

    def cuda(self):
        return torch.from_numpy(self._x.copy()).cuda()


def _pcm16(x):
    xi = np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)
    return xi, (xi / 2 ** 15).astype(np.float32)          # audio_utils.py:245-246


def _model(nafp, seed=7):
    m = nafp.FingerPrinter(seed=0)
    m.set_weights(_inputs.weight_list(_inputs.weights(seed=seed)))
    return m


@pytest.mark.parametrize('tag', ['A', 'B', 'C', 'D', 'E', 'H', 'L', 'S', 'F'])
def test_general_kernel_matches_oracle(nafp, tag):
    x, want = _case(tag)
    m_pre = _layer(nafp, tag)
    assert m_pre.kernel == 1 and m_pre.front_end['kernel_name'] == 'general'
    got = m_pre(x.cuda(), group_size=2).cpu().numpy()
    assert got.shape == want.shape == (5,) + GEOM[tag][1] + (1,)
    err = np.abs(got - want).max()
    print(f'{tag}: |d log-mel| max = {err:.3e}')
    assert err < 2e-5
    for g0 in (0, 2, 4):                                   # 2, 2, 1 segments: each group has its own zero maximum
        assert got[g0:g0 + 2].max() == 0.0


@pytest.mark.parametrize('tag', ['A', 'F'])
def test_maxnorm(nafp, tag):
    x, want = _case(tag, 5, 2, True)
    got = _layer(nafp, tag, segment_norm=True)(x.cuda(), group_size=2).cpu().numpy()
    err = np.abs(got - want).max()
    print(f'maxnorm {tag}: {err:.3e}')
    assert err < 1e-4


@pytest.mark.parametrize('tag', ['B', 'D'])
def test_int16_and_windows_give_the_same_bytes(nafp, tag):
    seg_len = GEOM[tag][0][1]
    xi, xf = _pcm16(_case(tag)[0].numpy())
    m_pre = _layer(nafp, tag)
    got_f = m_pre(torch.from_numpy(xf).cuda(), group_size=2)
    got_i = m_pre(torch.from_numpy(xi).cuda(), group_size=2)
    assert torch.equal(got_i, got_f)
    # windows: odd offsets into one arena, some segments with a zero tail
    rng = np.random.default_rng(11)
    arena = rng.integers(-9000, 9000, size=4 * seg_len + 64).astype(np.int16)
    off = np.array([1, 7, seg_len // 2 + 3, seg_len + 5, 2 * seg_len + 9, 3 * seg_len + 63], np.int64)
    valid = np.array([seg_len, seg_len - 1, seg_len // 3, seg_len, 1, seg_len - 7], np.int32)
    rows = np.zeros((len(off), 1, seg_len), np.int16)
    for i, (o, v) in enumerate(zip(off, valid)):
        rows[i, 0, :v] = arena[o:o + v]
    for defer in (False, True):
        w = m_pre.forward_windows(torch.from_numpy(arena).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(valid).cuda(),
                                  group_size=4, defer=defer)
        r = m_pre(torch.from_numpy(rows).cuda(), group_size=4, defer=defer)
        if defer:
            assert torch.equal(w.raw, r.raw) and torch.equal(w.gstat, r.gstat)
        else:
            assert torch.equal(w, r)


@pytest.mark.parametrize('tag', ['A', 'C', 'F'])
def test_deferred_then_finish_is_the_direct_call(nafp, tag):
    x = _case(tag)[0].cuda()
    for segment_norm in (False, True):
        m_pre = _layer(nafp, tag, segment_norm=segment_norm)
        for g in (None, 2):
            assert torch.equal(m_pre(x, group_size=g, defer=True).finish(), m_pre(x, group_size=g))


def test_encoder_on_deferred_features_is_bit_identical(nafp):
    x = _case('B')[0].cuda()
    m_pre, m = _layer(nafp, 'B'), _model(nafp)
    for g in (None, 2):
        assert torch.equal(m(m_pre(x, group_size=g, defer=True)), m(m_pre(x, group_size=g)))


def test_forced_general_kernel_at_the_base_geometry(nafp):
    x, want = _case('base')
    xt = x.cuda()
    gen, tuned = _layer(nafp, 'base', FORCE), _layer(nafp, 'base', ANY)
    assert gen.kernel == 1 and tuned.kernel == 0
    got = gen(xt, group_size=2).cpu().numpy()
    ref = tuned(xt, group_size=2).cpu().numpy()
    print(f'base: general vs oracle {np.abs(got - want).max():.3e}, tuned vs oracle {np.abs(ref - want).max():.3e}, '
          f'general vs tuned {np.abs(got - ref).max():.3e}')
    assert np.abs(got - want).max() < 2e-5
    assert np.abs(got - ref).max() < 4e-5                  # both are within 2e-5 of one oracle


@pytest.mark.parametrize('tag', ['B', 'L'])
def test_launch_independence_and_repeatability(nafp, tag):
    fs, seg_len = GEOM[tag][0][:2]
    x = torch.from_numpy(_audio(7, seed=21, T=seg_len, fs=fs)).cuda()
    m_pre = _layer(nafp, tag)
    whole = m_pre(x, group_size=3, defer=True)
    again = m_pre(x, group_size=3, defer=True)
    assert torch.equal(whole.raw, again.raw) and torch.equal(whole.gstat, again.gstat)
    for i in range(7):
        assert torch.equal(m_pre(x[i:i + 1], defer=True).raw[0], whole.raw[i])


def test_more_chunks_than_grid_rows(nafp):
    """hop 1 on a long segment: 65,545 chunks of 16 frames, more than the 65,535 workgroups a segment gets, so the first ten
    workgroups take a second chunk.  The raw rows against the float64 oracle on three stretches -- the head, the frames around
    chunk 65,535 and the tail: frame t of the segment is frame t - a of x[a : a + n] wherever the window (128) lies inside."""
    fs, n_fft, hop, n_mels, f_min, f_max = 8000, 128, 1, 3, 0., 4000.
    T, n = 65545 * 16 - 8, 4096
    x = _audio(1, seed=3, T=T, fs=fs)
    m_pre = nafp.Melspec_layer(input_shape=(1, T), n_fft=n_fft, stft_hop=hop, n_mels=n_mels, fs=fs, dur=T / fs, f_min=f_min,
                               f_max=f_max, plan_flags=ANY)
    assert m_pre.n_frames == T + 1 and m_pre.front_end['workgroups_per_segment'] == 65545
    d = m_pre(torch.from_numpy(x).cuda(), defer=True)
    raw, gstat = d.raw.cpu().numpy().reshape(n_mels, T + 1), d.gstat.cpu().numpy()
    assert gstat[0] == raw.max() and gstat[1] == raw.min()
    for a, lo, hi in ((0, 0, n - 64), (65535 * 16 - n // 2, 64, n - 64), (T - n, 64, n + 1)):
        want = o_mel.melspec_layer(x[:, :, a:a + n], fs, n_fft, hop, n_mels, f_min, f_max, return_raw=True)[1][0]
        err = np.abs(raw[:, a + lo:a + hi] - want[:, lo:hi]).max()
        print(f'frames {a + lo} ... {a + hi - 1}: |d log-mel| max = {err:.3e}')
        assert err < 2e-5
    out = d.finish().cpu().numpy()
    assert out.max() == 0.0 and np.array_equal(out.reshape(n_mels, T + 1), np.maximum(raw - raw.max(), np.float32(-80)))


def test_nan_sample_poisons_its_own_segment_only(nafp):
    """The contract of test_nan_segment_through_the_front_end_and_the_deferred_path, on the general kernel."""
    fs, seg_len = GEOM['B'][0][:2]
    m_pre, m = _layer(nafp, 'B'), _model(nafp)
    x = torch.from_numpy(_audio(6, seed=5, T=seg_len, fs=fs)).cuda()
    clean = m(m_pre(x, defer=True)).clone()
    x2 = x.clone()
    x2[4, 0, 1234] = float('nan')
    keep = [b for b in range(6) if b != 4]
    for defer in (True, False):
        emb = m(m_pre(x2, defer=defer))
        assert bool(torch.isnan(emb[4]).all())
        assert bool(torch.isfinite(emb[keep]).all())
        assert float((emb[keep] - clean[keep]).abs().max()) < 1e-6


@functools.lru_cache(maxsize=None)
def _end_to_end_case():
    fs, seg_len, n_fft, hop, n_mels, f_min, f_max = GEOM['B'][0]
    x = _audio(6, seed=5, T=seg_len, fs=fs)
    w = o_nnfp.init_weights(seed=4, randomize_affine=True)
    want = o_nnfp.fingerprinter(o_mel.melspec_layer(x, fs, n_fft, hop, n_mels, f_min, f_max), w)
    return x, w, want


def test_end_to_end_audio_to_fingerprint_16k(nafp, cfg, arith):
    x, w, want = _end_to_end_case()
    m_pre, m_fp = _layer(nafp, 'B'), nafp.get_fingerprinter(cfg)
    m_fp.set_weights(_inputs.weight_list(w))
    emb = m_fp(m_pre(torch.from_numpy(x).cuda())).cpu().numpy()
    cos = (emb * want).sum(1)
    print(f'end to end B ({arith}): 1 - cos max = {(1 - cos).max():.3e}')
    assert (1 - cos).max() < 1e-5
    assert np.abs(np.linalg.norm(emb, axis=1) - 1).max() < 1e-5


def test_opt_in(nafp, cfg, monkeypatch, capfd):
    c = copy.deepcopy(cfg)
    c['MODEL']['STFT_WIN'] = 512
    c['MODEL']['F_MIN'] = 310.                    # a geometry no other test builds: the layer announces a geometry once per process
    monkeypatch.delenv('NAFP_MELSPEC_ANY', raising=False)
    with pytest.raises(nafp._lib.NafpError, match='NAFP_MELSPEC_ANY'):
        nafp.get_melspec_layer(c)
    assert nafp.get_melspec_layer(cfg).kernel == 0
    monkeypatch.setenv('NAFP_MELSPEC_ANY', '1')
    capfd.readouterr()
    m_pre = nafp.get_melspec_layer(c)
    again = nafp.get_melspec_layer(c)
    err = capfd.readouterr().err
    assert m_pre.kernel == 1 and again.kernel == 1 and (m_pre.n_mels, m_pre.n_frames) == (256, 32)
    assert err.count('general kernel') == 1 and 'n_fft 512' in err and 'f_min 310' in err
    assert m_pre.front_end['n_fft'] == 512 and m_pre.front_end['kernel'] == 1
    assert nafp.get_melspec_layer(cfg).kernel == 0          # the shipped geometry stays on the tuned kernel


def test_generate_with_a_16k_model(nafp, cfg, tmp_path, monkeypatch):
    from neural_audio_fp_amd.model import generate as g
    monkeypatch.setenv('NAFP_MELSPEC_ANY', '1')
    fs, seg_len, n_fft, hop, n_mels, f_min, f_max = GEOM['B'][0]
    c = copy.deepcopy(cfg)
    c['MODEL'].update({'FS': fs, 'STFT_WIN': n_fft, 'STFT_HOP': hop, 'N_MELS': n_mels, 'F_MIN': f_min, 'F_MAX': f_max})
    c['BSZ']['TS_BATCH_SZ'] = 1                   # every segment is its own max-normalisation group
    c['DIR']['LOG_ROOT_DIR'] = str(tmp_path) + '/logs/'
    c['DIR']['OUTPUT_ROOT_DIR'] = str(tmp_path) + '/logs/emb/'
    src = tmp_path / 'src'; src.mkdir()
    rng = np.random.default_rng(16)
    t = np.arange(5 * fs) / float(fs)
    for i, n in enumerate([3 * fs, 4 * fs + 123, 5 * fs]):
        pcm = rng.integers(-3000, 3000, size=n) + (6000 * np.sin(2 * np.pi * (700 + 1900 * i) * t[:n])).astype(int)
        with wave.open(str(src / f'{i}.wav'), 'w') as wv:
            wv.setnchannels(1); wv.setsampwidth(2); wv.setframerate(fs)
            wv.writeframes(pcm.astype('<i2').tobytes())
    m_fp = nafp.get_fingerprinter(c)
    m_fp.set_weights(_inputs.weight_list(_inputs.weights(seed=8)))
    g.save_checkpoint(c['DIR']['LOG_ROOT_DIR'] + 'checkpoint/', 'exp16', 3, m_fp)
    g.generate_fingerprint(c, 'exp16', None, str(src), None, True)
    out_dir = c['DIR']['OUTPUT_ROOT_DIR'] + '/exp16/3/'
    shape = tuple(np.load(out_dir + 'custom_source_shape.npy'))
    assert shape == (5 + 7 + 9, 128)
    got = np.asarray(np.memmap(out_dir + 'custom_source.mm', dtype='float32', mode='r', shape=shape))
    paths = sorted(str(p) for p in src.glob('*.wav'))
    segs = np.concatenate(list(o_seg.load_batches(paths, 1, fs=fs))).astype(np.float32)          # int16 / 2^15: exact in float32
    assert segs.shape == (shape[0], 1, seg_len)
    m_pre = nafp.get_melspec_layer(c)
    assert m_pre.kernel == 1
    want = torch.cat([m_fp(m_pre(torch.from_numpy(s[None]).cuda())) for s in segs]).cpu().numpy()
    assert np.array_equal(got, want)
    fe = json.load(open(out_dir + 'front_end.json'))
    assert (fe['fs'], fe['seg_len'], fe['n_fft'], fe['hop'], fe['n_mels'], fe['f_min'], fe['f_max']) == GEOM['B'][0]
    assert fe['kernel'] == 1 and fe['kernel_name'] == 'general' and fe['n_frames'] == 32 and fe['widest_filter'] == 22
