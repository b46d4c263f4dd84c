"""GPU: nafp_augment_rows (window -> bg mix -> IR -> normalise, one launch) vs the oracle's restatement
of load_audio / bg_mix_batch / ir_aug_batch (oracle/augment.py) on the same windows and the same draws."""
import wave

import numpy as np
import pytest
import torch

from oracle import augment as A

pytestmark = pytest.mark.gpu


def _write_wav(path, pcm, fs=8000):
    with wave.open(path, 'w') as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(fs)
        w.writeframes(np.asarray(pcm).astype('<i2').tobytes())


def _oracle_rows(arena, rows, T):
    out = np.zeros((len(rows), T))
    for i, r in enumerate(rows):
        x = A.window(arena[r['ev_off']:r['ev_off'] + r['ev_valid']], 0, T)
        if r['mix']:
            nz = np.zeros(T)
            for key in ('nz', 'nz2'):
                if r[key + '_off'] >= 0:
                    nz += A.window(arena[r[key + '_off']:r[key + '_off'] + r[key + '_valid']], 0, T)
            x = A.bg_mix_rows(x[None], nz[None], [float(r['snr_db'])], [float(r['amp'])])[0]
        if r['ir_off'] >= 0:
            ir = arena[r['ir_off']:r['ir_off'] + r['ir_len']].astype(np.float64) / 2 ** 15
            x = A.ir_aug_rows(x[None], [ir])[0]
        out[i] = x
    return out


@pytest.fixture()
def corpus(tmp_path):
    rng = np.random.default_rng(7)
    t = np.arange(120000) / 8000.0

    def music(n):
        return (rng.integers(-2000, 2000, size=n) + 9000 * np.sin(2 * np.pi * rng.uniform(200, 3000) * t[:n])).astype(int)
    mk = lambda sub, arrs: [(_write_wav(str(tmp_path / f'{sub}{i}.wav'), a), str(tmp_path / f'{sub}{i}.wav'))[1] for i, a in enumerate(arrs)]
    ir = lambda n: (12000 * rng.normal(size=n) * np.exp(-np.arange(n) / 80.0)).astype(int)
    return {'ev': mk('ev', [music(120000), music(50000), np.zeros(30000, int), music(8000)]),
            'bg': mk('bg', [rng.integers(-6000, 6000, size=40000), np.zeros(9000, int)]),
            'ir': mk('ir', [ir(300), ir(2000), ir(601), np.zeros(50, int)]), 'sp': mk('sp', [rng.integers(-3000, 3000, size=20000)])}


@pytest.mark.parametrize('speech', [False, True])
def test_augmented_batch_matches_oracle(nafp, corpus, speech):
    from neural_audio_fp_amd.model.utils.dataloader_keras import genUnbalSequence
    ds = genUnbalSequence(corpus['ev'], bsz=48, n_anchor=8, shuffle=True, random_offset_anchor=True,
                          bg_mix_parameter=[True, corpus['bg'], (0, 10)], ir_mix_parameter=[True, corpus['ir']],
                          speech_mix_parameter=[speech, corpus['sp'], (3, 7)], seed=11)
    arena = ds.arena.host()
    worst = 0.0
    for idx in range(min(len(ds), 6)):
        rows = ds.plan(idx)
        Xa, Xp = ds[idx]                                          # same draws: plan() is a pure function of (seed, epoch, idx)
        assert Xa.shape == (8, 1, 8000) and Xp.shape == (40, 1, 8000) and Xa.dtype == torch.float32
        got = torch.cat([Xa, Xp])[:, 0].cpu().numpy()
        want = _oracle_rows(arena, rows, 8000)
        assert np.array_equal(got[:8], want[:8].astype(np.float32))          # anchors: exact int16 / 2^15
        worst = max(worst, np.abs(got - want).max())
        assert np.abs(got - want).max() < 2e-5
        # silent event / silent background / silent IR rows took the reference's special branches
    print('worst |augment - oracle|', worst)
    assert np.isfinite(got).all()


def test_special_rows(nafp, corpus):
    """silent event, silent background, silent impulse response, window past the end of a file."""
    from neural_audio_fp_amd import _lib
    from neural_audio_fp_amd.model.utils.dataloader_keras import genUnbalSequence
    ds = genUnbalSequence(corpus['ev'], bsz=4, n_anchor=2, bg_mix_parameter=[True, corpus['bg'], (0, 10)],
                          ir_mix_parameter=[True, corpus['ir']])
    arena = ds.arena.host()
    rows = np.zeros(5, dtype=_lib.AUG_ROW_DTYPE)
    rows['nz2_off'] = -1; rows['amp'] = [0.5, 0.25, 1.0, 0.7, 1.0]; rows['snr_db'] = 4.0; rows['mix'] = 1
    ev, bg, ir = ds.ev.start, ds.bg.start, ds.ir.start
    rows['ev_off'] = [ev[2], ev[0] + 123, ev[0] + 77, ev[1] + 46001, ev[3]]      # silent event | ... | 3999 valid samples | whole 1-s file
    rows['ev_valid'] = [8000, 8000, 8000, 3999, 8000]
    rows['nz_off'] = [bg[0], bg[1], bg[0] + 16000, bg[0] + 5, bg[1]]              # | silent bg | ...
    rows['nz_valid'] = [8000, 8000, 8000, 8000, 1000]
    rows['ir_off'] = [ir[0], ir[1], ir[3], ir[2], -1]                              # | | silent IR | 600 of 601 taps | none
    rows['ir_len'] = [300, 600, 50, 600, 0]
    got = ds.run(rows)[:, 0].cpu().numpy()
    want = _oracle_rows(arena, rows, 8000)
    assert np.abs(got - want).max() < 2e-5
    assert np.abs(got[2]).max() == 0.0                        # circular convolution with a silent IR is silence
    assert abs(np.abs(got[0]).max() - 1.0) < 1e-6 and abs(np.abs(got[4]).max() - 1.0) < 1e-6


def _edge_arena():
    """one int16 arena for every seg_len up to 19000: an event that is non-zero at both ends of every window, two noises and three
    impulse responses (640 decaying taps; 600 taps whose energy sits in the last five; the places where each starts)."""
    rng = np.random.default_rng(19000)
    n = 19000
    t = np.arange(n + 32) / 8000.0                            # every row takes its own window of the event
    ev = (rng.integers(-2000, 2000, size=n + 32) + 9000 * np.sin(2 * np.pi * 440.0 * t)).astype(np.int16)
    ev[ev == 0] = 1
    bg = rng.integers(-6000, 6000, size=n).astype(np.int16)
    sp = rng.integers(-3000, 3000, size=n).astype(np.int16)
    ir = (12000 * rng.normal(size=640) * np.exp(-np.arange(640) / 80.0)).astype(np.int16)
    ir[:4] = [9000, -5000, 3000, -2000]                       # the 1-, 2- and 3-tap responses are not silent
    ir[596:640] = rng.integers(200, 400, size=44)             # taps 596 (beyond a 597-tap response's last) .. 639 (beyond the 600 kept) matter
    tail = np.zeros(600, np.int16)
    tail[595:] = [3000, -7000, 12000, -9000, 5000]
    parts, at, pos = {}, [], 3                                # odd starts: nothing here needs an aligned window
    for name, a in (('ev', ev), ('bg', bg), ('sp', sp), ('ir', ir), ('tail', tail)):
        parts[name] = pos
        at.append((pos, a))
        pos += len(a) + 5
    arena = np.zeros(pos + 8, np.int16)
    for o, a in at:
        arena[o:o + len(a)] = a
    return arena, parts


_EDGE_CASES = [  # name, ev_valid (None = seg_len), mix, (nz, nz2) present, snr_db, amp, (ir, ir_len)
    ('anchor', None, 0, (0, 0), 0.0, 1.0, None),
    ('anchor with a zero tail', -37, 0, (0, 0), 0.0, 1.0, None),
    ('anchor without a sample', 0, 0, (0, 0), 0.0, 1.0, None),
    ('1 tap', None, 0, (0, 0), 0.0, 1.0, ('ir', 1)),
    ('2 taps', None, 0, (0, 0), 0.0, 1.0, ('ir', 2)),
    ('3 taps', None, 0, (0, 0), 0.0, 1.0, ('ir', 3)),
    ('597 taps', None, 0, (0, 0), 0.0, 1.0, ('ir', 597)),
    ('600 taps after a mix', None, 1, (1, 0), 4.0, 0.5, ('ir', 600)),
    ('640 taps given, 600 used', None, 0, (0, 0), 0.0, 1.0, ('ir', 640)),
    ('energy in the last taps: the circular wrap', None, 0, (0, 0), 0.0, 1.0, ('tail', 600)),
    ('speech without background', None, 1, (0, 1), 6.0, 0.7, None),
    ('speech without background, then 3 taps', -101, 1, (0, 1), 6.0, 0.7, ('ir', 3)),
    ('mix without any noise', None, 1, (0, 0), 3.0, 0.3, None),
    ('mix without any noise, then 597 taps', None, 1, (0, 0), 3.0, 0.3, ('ir', 597)),
    ('no valid sample, mixed', 0, 1, (1, 1), 5.0, 0.9, None),
    ('no valid sample, mixed, 600 taps', 0, 1, (1, 0), 5.0, 0.9, ('ir', 600)),
    ('no valid sample, 600 taps', 0, 0, (0, 0), 0.0, 1.0, ('ir', 600)),
    ('snr -20 dB', None, 1, (1, 1), -20.0, 0.6, None),
    ('snr +40 dB, 600 taps', None, 1, (1, 0), 40.0, 0.2, ('tail', 600)),
]


@pytest.mark.parametrize('T', [608, 8000, 16000, 19000])
def test_rows_at_the_edges_through_the_abi(nafp, T):
    """nafp_augment_rows on its own arena and row table: the shortest seg_len that holds the 600 taps and their padding, 1 s, 2 s
    (130 KB of dynamic LDS) and the 19000 limit; 1 / 2 / 3 / 597 / 600 taps, 640 given (the kernel keeps MAX_IR_LENGTH = 600, as the
    loader does: the oracle gets those 600), a response with its energy in the last taps over an event that is non-zero at both ends
    of the window (the circular wrap); a speech window without a background window, a mix without any noise, no valid sample with
    and without a mix, SNR -20 and +40 dB; anchors bit for bit; and an empty table."""
    import ctypes
    from neural_audio_fp_amd import _lib
    lib = _lib.load()
    arena, at = _edge_arena()
    rows = np.zeros(len(_EDGE_CASES), dtype=_lib.AUG_ROW_DTYPE)
    for i, (name, valid, mix, (nz, nz2), snr, amp, ir) in enumerate(_EDGE_CASES):
        r = rows[i]
        r['ev_off'] = at['ev'] + i                             # a different window per row
        r['ev_valid'] = T if valid is None else (T + valid if valid < 0 else valid)
        r['mix'], r['snr_db'], r['amp'] = mix, snr, amp
        r['nz_off'], r['nz_valid'] = (at['bg'] + 2 * i, T - 3 * i) if nz else (-1, 0)
        r['nz2_off'], r['nz2_valid'] = (at['sp'] + i, T - 100) if nz2 else (-1, 0)
        r['ir_off'], r['ir_len'] = (at[ir[0]], ir[1]) if ir else (-1, 0)
    assert int((rows['ev_off'] + rows['ev_valid']).max()) <= at['ev'] + 19000 + 32
    for_oracle = rows.copy()
    for_oracle['ir_len'] = np.minimum(rows['ir_len'], 600)
    want = _oracle_rows(arena, for_oracle, T)

    pcm = torch.from_numpy(arena).cuda()
    d_rows = torch.from_numpy(rows.view(np.uint8).reshape(-1)).cuda()
    out = torch.full((len(rows), T), float('nan'), device='cuda')
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.nafp_augment_rows(ptr(pcm), ptr(d_rows), len(rows), T, ptr(out), stream) == 0
    got = out.cpu().numpy()
    err = np.abs(got - want).max(axis=1)
    for (name, *_), e in zip(_EDGE_CASES, err):
        print(f'T {T} {name}: {e:.3e}')
    assert np.isfinite(got).all() and err.max() < 2e-5
    for i, (name, valid, mix, _, _, _, ir) in enumerate(_EDGE_CASES):
        if not mix and ir is None:                             # anchors: exact int16 / 2^15, zero tail
            assert np.array_equal(got[i], want[i].astype(np.float32)), name
        if valid == 0 and not mix:
            assert not got[i].any(), name                      # silence stays silence, also through an impulse response
    peak = np.abs(got).max(axis=1)
    by_name = {c[0]: i for i, c in enumerate(_EDGE_CASES)}
    assert abs(peak[by_name['640 taps given, 600 used']] - 1.0) < 1e-6 and abs(peak[by_name['snr +40 dB, 600 taps']] - 1.0) < 1e-6
    assert abs(peak[by_name['speech without background']] - 0.7) < 1e-6 and abs(peak[by_name['mix without any noise']] - 0.3) < 1e-6
    # the 640-tap row differs from what all 640 taps would give by far more than the tolerance: the clamp is seen
    all_taps = _oracle_rows(arena, rows[by_name['640 taps given, 600 used']:][:1], T)[0]
    assert np.abs(all_taps - want[by_name['640 taps given, 600 used']]).max() > 1e-3

    # an empty table: NAFP_OK, nothing written
    out.fill_(-3.0)
    assert lib.nafp_augment_rows(ptr(pcm), ptr(d_rows), 0, T, ptr(out), stream) == 0
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())


def test_dataset2wav_writes_one_augmented_clip_per_source(nafp, cfg, tmp_path):
    import copy, importlib.util, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('dataset2wav', os.path.join(root, 'tools', 'dataset2wav.py'))
    d2w = importlib.util.module_from_spec(spec); spec.loader.exec_module(d2w)
    rng = np.random.default_rng(5)
    base = str(tmp_path) + '/'
    t = np.arange(48000) / 8000.0
    for i in range(2):
        os.makedirs(base + 'music/q/db/x', exist_ok=True)
        _write_wav(base + f'music/q/db/x/{i}.wav', (rng.integers(-500, 500, size=48000) + 8000 * np.sin(2 * np.pi * (400 + 300 * i) * t)).astype(int))
    os.makedirs(base + 'bg/ts'); os.makedirs(base + 'ir/ts')
    _write_wav(base + 'bg/ts/0.wav', rng.integers(-3000, 3000, size=30000))
    _write_wav(base + 'ir/ts/0.wav', (15000 * np.exp(-np.arange(300) / 25.0) * rng.normal(size=300)).astype(int))
    c = copy.deepcopy(cfg)
    c['DIR'].update({'SOURCE_ROOT_DIR': base + 'music/', 'BG_ROOT_DIR': base + 'bg/', 'IR_ROOT_DIR': base + 'ir/'})
    files = d2w.synthesize(c, 'q/db', base + 'out', snr=(10, 10), interval=1, clip_sec=6)
    assert [f.split('/')[-2:] for f in files] == [['x', '0.wav'], ['x', '1.wav']]
    for f in files:
        with wave.open(f) as w:
            assert (w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()) == (8000, 1, 2, 48000)
            x = np.frombuffer(w.readframes(48000), dtype='<i2').astype(np.float64) / 32767
        pieces = np.abs(x.reshape(6, 8000)).max(1)
        assert np.all(pieces > 0.99) and np.all(pieces <= 1.0)     # every 1-s piece was max-normalised after the IR
