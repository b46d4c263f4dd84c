"""GPU: nafp_augment_rows_speed (csrc/augment.hip: replicas played at another speed inside the batch kernel).

BYTE EQUALITY with the composition of the two existing kernels -- nafp_varispeed_i16 renders the row's outputs into a scratch window,
nafp_augment_rows runs the chain on it -- and, independently of both, the events rendered by the numpy restatement of the varispeed
contract (tests/_varispeed_ref.py) through the float64 oracle chain (oracle/augment.py) within the 2e-5 that tests/test_gpu_augment.py
uses for this kernel's chain."""
import ctypes
import wave

import numpy as np
import pytest
import torch

import _varispeed_ref as ref
from oracle import augment as A

pytestmark = pytest.mark.gpu

ONE = 1 << 24
# both ends of the range, unity through a slot (a 0.95-Nyquist low-pass, not the identity), one step with W = 34 and one with W = 37
STEPS = [ref.STEP_MIN, ref.STEP_MAX, ONE, int(round(ONE * 0.93)), int(round(ONE * 1.07))]


def _write_wav(path, pcm, fs=8000):
    with wave.open(path, 'w') as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(fs)
        w.writeframes(np.asarray(pcm).astype('<i2').tobytes())


class World:
    """The corpus in one arena (through the loader's stores), on the host and on the device, and a step set."""


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    import neural_audio_fp_amd as nafp
    from neural_audio_fp_amd.model.utils.dataloader_keras import genUnbalSequence
    tmp = tmp_path_factory.mktemp('speed_aug')
    rng = np.random.default_rng(7)
    t = np.arange(120000) / 8000.0

    def music(n):
        return (rng.integers(-2000, 2000, size=n) + 9000 * np.sin(2 * np.pi * rng.uniform(200, 3000) * t[:n])).astype(int)
    mk = lambda sub, arrs: [(_write_wav(str(tmp / f'{sub}{i}.wav'), a), str(tmp / f'{sub}{i}.wav'))[1] for i, a in enumerate(arrs)]
    ir = lambda n: (12000 * rng.normal(size=n) * np.exp(-np.arange(n) / 80.0)).astype(int)
    loud = lambda n: np.where(rng.integers(0, 2, size=n) > 0, 32767, -32768)
    # events: 0 long | 1 medium | 2 silent | 3 one segment | 4 shorter than a segment | 5 full scale | 6 the target, a multiple of 8
    # samples so that nothing lies between it and its neighbours | 7 full scale
    w = World()
    w.files = {'ev': mk('ev', [music(120000), music(50000), np.zeros(30000, int), music(8000), music(5000), loud(12000), music(20000), loud(12000)]),
               'bg': mk('bg', [rng.integers(-6000, 6000, size=40000), np.zeros(9000, int)]),
               'ir': mk('ir', [ir(300), ir(2000), ir(601), np.zeros(50, int)]), 'sp': mk('sp', [rng.integers(-3000, 3000, size=20000)])}
    w.ds = genUnbalSequence(w.files['ev'], bsz=4, n_anchor=2, bg_mix_parameter=[True, w.files['bg'], (0, 10)],
                            ir_mix_parameter=[True, w.files['ir']], speech_mix_parameter=[True, w.files['sp'], (3, 7)])
    w.arena = w.ds.arena.host()
    assert int(w.ds.ev.start[6]) == int(w.ds.ev.start[5]) + 12000 and int(w.ds.ev.start[7]) == int(w.ds.ev.start[6]) + 20000
    assert abs(int(w.arena[w.ds.ev.start[6] - 1])) >= 32767 and abs(int(w.arena[w.ds.ev.start[7]])) >= 32767
    w.pcm = torch.from_numpy(w.arena).cuda()
    w.lib = nafp._lib.load()
    w._lib = nafp._lib
    h = ctypes.c_void_p()
    steps = np.asarray(STEPS, np.uint32)
    assert w.lib.nafp_aug_speedset_create(ctypes.byref(h), steps.ctypes.data_as(ctypes.c_void_p), len(steps)) == 0
    w.set = h
    w.tables = {s: ref.table(s) for s in STEPS}
    w.cache = {}
    yield w
    w.lib.nafp_aug_speedset_destroy(h)


_ptr = lambda t: ctypes.c_void_p(t.data_ptr())
_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
_stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _plain(w, rows, T, pcm=None):
    pcm = w.pcm if pcm is None else pcm
    out = torch.full((len(rows), T), float('nan'), device='cuda')
    d_rows = _dev(rows)
    assert w.lib.nafp_augment_rows(_ptr(pcm), _ptr(d_rows), len(rows), T, _ptr(out), _stream()) == 0
    return out.cpu().numpy()


def _speed(w, rows, speeds, T, set_=None):
    out = torch.full((len(rows), T), float('nan'), device='cuda')
    d_rows, d_sp = _dev(rows), (_dev(speeds) if speeds is not None else None)
    st = w.lib.nafp_augment_rows_speed(set_ or w.set, _ptr(w.pcm), w.pcm.numel(), _ptr(d_rows), _ptr(d_sp) if d_sp is not None else None,
                                       len(rows), T, _ptr(out), _stream())
    assert st == 0, st
    return out.cpu().numpy()


def _existing(sp, T, steps):
    """outputs of the row's window that exist: [out0, out0 + T) n [0, n_out)"""
    return int(np.clip(ref.n_out(int(sp['n_in']), steps[sp['slot']]) - int(sp['out0']), 0, T))


def _composition(w, rows, speeds, T, steps=STEPS):
    """The same rows through the two existing kernels: every speed row's outputs rendered by nafp_varispeed_i16 (varispeed.Plan.run)
    into a scratch window appended to a copy of the arena, a plain nafp_aug_row pointed at it, nafp_augment_rows."""
    from neural_audio_fp_amd.model.utils import varispeed as vs
    n_arena = len(w.arena)
    scratch = torch.zeros((max(len(rows), 1) * T,), dtype=torch.int16, device='cuda')
    rows2 = rows.copy()
    by_step = {}
    for i, sp in enumerate(speeds):
        if sp['slot'] < 0:
            continue
        cnt = _existing(sp, T, steps)
        rows2['ev_off'][i], rows2['ev_valid'][i] = n_arena + i * T, cnt
        if cnt:
            by_step.setdefault(steps[sp['slot']], []).append((int(sp['file_off']), 0, int(sp['n_in']), int(sp['n_in']), int(sp['out0']), i * T, cnt, 0))
    for step, pieces in by_step.items():
        vs.plan_for(step).run(w.pcm, np.asarray(pieces, dtype=vs.PIECE_DTYPE), scratch)
    return _plain(w, rows2, T, pcm=torch.cat([w.pcm, scratch]))


def _ref_events(w, rows, speeds, T, steps=STEPS):
    """(arena with the events of the speed rows appended, plain rows over it): the events by tests/_varispeed_ref.py alone."""
    ext = np.zeros(len(rows) * T, np.int16)
    rows2 = rows.copy()
    for i, sp in enumerate(speeds):
        if sp['slot'] < 0:
            continue
        step = steps[sp['slot']]
        cnt = _existing(sp, T, steps)
        rows2['ev_off'][i], rows2['ev_valid'][i] = len(w.arena) + i * T, cnt
        if cnt:
            x = w.arena[int(sp['file_off']):int(sp['file_off']) + int(sp['n_in'])]
            n = np.arange(int(sp['out0']), int(sp['out0']) + cnt, dtype=np.int64)
            ext[i * T:i * T + cnt] = ref.finish(ref.accumulate(x, step, w.tables[step], n=n))
    return np.concatenate([w.arena, ext]), rows2


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


# what follows the event: (mix, speech, impulse response)
_CHAINS = [(1, 0, 1), (1, 1, 1), (0, 0, 0), (0, 0, 1), (1, 1, 0)]


def _cases(w, T):
    """(names, rows, speeds): per step, on the long file out0 = 0, a window that ends past n_out, a window wholly past n_out; the file
    shorter than a segment; the file between full-scale neighbours at its first and at its last outputs; then the silent file, two
    plain rows (slot -1) and an anchor.  Every chain occurs with every kind of row."""
    ev, bg, sp_, ir = w.ds.ev, w.ds.bg, w.ds.sp, w.ds.ir
    names, rows, speeds = [], [], []

    def add(name, slot, f, out0, chain, k):
        mix, speech, use_ir = chain
        R, S = np.zeros(1, dtype=w._lib.AUG_ROW_DTYPE), np.zeros(1, dtype=w._lib.AUG_SPEED_DTYPE)
        r, s = R[0], S[0]                                       # views: the fields are written through them
        r['ev_off'], r['ev_valid'] = int(ev.start[f]) + 16 * k, int(min(T, max(0, ev.n_frames[f] - 16 * k)))      # used by plain rows only
        r['nz_off'] = r['nz2_off'] = r['ir_off'] = -1
        r['amp'], r['snr_db'], r['mix'] = (0.3 + 0.05 * (k % 9), float(k % 11), 1) if mix else (1.0, 0.0, 0)
        if mix:
            r['nz_off'], r['nz_valid'] = int(bg.start[0]) + 37 * k, T
        if mix and speech:
            r['nz2_off'], r['nz2_valid'] = int(sp_.start[0]) + 11 * k, T - 7
        if use_ir:
            j = k % 3
            r['ir_off'], r['ir_len'] = int(ir.start[j]), min([300, 600, 600][j], T // 2)
        s['slot'] = slot
        if slot >= 0:
            s['file_off'], s['n_in'], s['out0'] = int(ev.start[f]), int(ev.n_frames[f]), out0
        names.append(name); rows.append(R); speeds.append(S)

    k = 0
    for slot, step in enumerate(STEPS):
        n_long, n_short, n_tgt = (ref.n_out(int(ev.n_frames[f]), step) for f in (0, 4, 6))
        for name, f, out0 in [('out0 = 0', 0, 0), ('ends past n_out', 0, n_long - T // 2 - 3), ('wholly past n_out', 0, n_long + 5),
                              ('short file', 4, max(0, n_short - 3 * T // 4)), ('between loud neighbours, first outputs', 6, 0),
                              ('between loud neighbours, last outputs', 6, n_tgt - T)]:
            add(f'step {step} {name}', slot, f, out0, _CHAINS[k % len(_CHAINS)], k)
            k += 1
    add('silent file', 1, 2, 100, (1, 0, 1), k); k += 1
    add('plain row, mixed', -1, 1, 0, (1, 1, 1), k); k += 1
    add('plain row, bare', -1, 3, 0, (0, 0, 0), k); k += 1
    add('anchor', -1, 0, 0, (0, 0, 0), k)
    return names, np.concatenate(rows), np.concatenate(speeds)


def _got(w, T):
    """The new entry's output for the case table of T, computed once per T and shared (read only)."""
    if T not in w.cache:
        names, rows, speeds = _cases(w, T)
        rows_h, sp_h = np.ascontiguousarray(rows), np.ascontiguousarray(speeds)
        assert w.lib.nafp_augment_speed_check_host(w.set, rows_h.ctypes.data_as(ctypes.c_void_p), sp_h.ctypes.data_as(ctypes.c_void_p),
                                                   len(rows), len(w.arena), T) == 0
        got = _speed(w, rows, speeds, T)
        got.setflags(write=False)
        w.cache[T] = (names, rows, speeds, got)
    return w.cache[T]


@pytest.mark.parametrize('T', [8000, 512])
def test_byte_equal_to_varispeed_then_augment_rows(world, T):
    names, rows, speeds, got = _got(world, T)
    want = _composition(world, rows, speeds, T)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    for i, name in enumerate(names):
        assert got[i].tobytes() == want[i].tobytes(), (T, name, float(np.abs(got[i] - want[i]).max()))
    # the cases are what they say: both tap counts, windows cut by n_out, zero events, the clamp of int16 next to full scale untouched
    assert {ref.geometry(s)[0] for s in STEPS} >= {34, 37, 43}
    cnt = np.asarray([_existing(s, T, STEPS) if s['slot'] >= 0 else T for s in speeds])
    assert (cnt == 0).sum() >= len(STEPS) and ((cnt > 0) & (cnt < T)).sum() >= len(STEPS)
    past = [i for i, n in enumerate(names) if 'wholly past' in n]
    assert any(rows['mix'][i] for i in past) and any(not rows['mix'][i] for i in past)
    for i in past:
        if not rows['mix'][i]:
            assert not got[i].any(), names[i]                   # silence stays silence, also through an impulse response


@pytest.mark.parametrize('T', [8000, 512])
def test_events_of_the_numpy_restatement_through_the_float64_oracle(world, T):
    names, rows, speeds, got = _got(world, T)
    arena2, rows2 = _ref_events(world, rows, speeds, T)
    want = _oracle_rows(arena2, rows2, T)
    err = np.abs(got - want).max(axis=1)
    for name, e in zip(names, err):
        print(f'T {T} {name}: {e:.3e}')
    assert err.max() < 2e-5
    bare = [i for i in range(len(rows)) if not rows['mix'][i] and rows['ir_off'][i] < 0]
    assert sum(speeds['slot'][i] >= 0 for i in bare) >= len(STEPS)
    for i in bare:                                              # no mix, no impulse response: the contract's int16 / 2^15, bit for bit
        x = arena2[rows2['ev_off'][i]:rows2['ev_off'][i] + rows2['ev_valid'][i]].astype(np.float32) / np.float32(32768.0)
        assert np.array_equal(got[i, :len(x)], x) and not got[i, len(x):].any(), names[i]
    # a neighbour's sample never enters: among the rows held bit for bit are the target's first and last outputs, whose taps reach
    # past both ends of the file, and the restatement saw the file alone
    tgt = [names[i] for i in bare if 'loud neighbours' in names[i]]
    assert any('first outputs' in n for n in tgt) and any('last outputs' in n for n in tgt)


def test_plain_entry_is_unchanged(world):
    T = 8000
    names, rows, speeds, got = _got(world, T)
    plain = _plain(world, rows, T)
    assert _speed(world, rows, None, T).tobytes() == plain.tobytes()                 # speeds == NULL
    out = torch.empty((len(rows), T), device='cuda')
    d_rows = _dev(rows)
    assert world.lib.nafp_augment_rows_speed(None, _ptr(world.pcm), world.pcm.numel(), _ptr(d_rows), None, len(rows), T, _ptr(out),
                                             _stream()) == 0                           # ... needs no set either
    assert out.cpu().numpy().tobytes() == plain.tobytes()
    off = speeds.copy()
    off['slot'] = -1                                                                   # every slot -1; the other fields are not looked at
    assert _speed(world, rows, off, T).tobytes() == plain.tobytes()
    minus = np.flatnonzero(speeds['slot'] == -1)
    assert len(minus) >= 3
    assert got[minus].tobytes() == plain[minus].tobytes()                             # slot -1 rows inside the mixed launch
    # a seg_len the speed path cannot hold is refused before any launch, with speeds only
    small = rows[:2].copy(); small['ev_valid'] = 64; small['mix'] = 0; small['ir_off'] = -1
    o = torch.empty((2, 64), device='cuda')
    d_small, d_sp = _dev(small), _dev(off[:2])
    assert world.lib.nafp_augment_rows_speed(world.set, _ptr(world.pcm), world.pcm.numel(), _ptr(d_small), _ptr(d_sp), 2, 64, _ptr(o), _stream()) == 2
    assert world.lib.nafp_augment_rows_speed(world.set, _ptr(world.pcm), world.pcm.numel(), _ptr(d_small), None, 2, 64, _ptr(o), _stream()) == 0
    assert o.cpu().numpy().tobytes() == _plain(world, small, 64).tobytes()


def test_rows_do_not_depend_on_their_launch(world):
    T = 8000
    names, rows, speeds, got = _got(world, T)
    again = _speed(world, rows, speeds, T)
    assert again.tobytes() == got.tobytes()                                           # the launch repeated
    for i in (0, 1, 7, 11, 16, 29, 30, len(rows) - 3):
        alone = _speed(world, rows[i:i + 1], speeds[i:i + 1], T)
        assert alone[0].tobytes() == got[i].tobytes(), names[i]
    order = np.random.default_rng(3).permutation(len(rows))
    assert _speed(world, rows[order], speeds[order], T).tobytes() == got[order].tobytes()
    # a set that holds the same step at another slot gives the same bytes
    h = ctypes.c_void_p()
    steps = np.asarray(STEPS[::-1], np.uint32)
    assert world.lib.nafp_aug_speedset_create(ctypes.byref(h), steps.ctypes.data_as(ctypes.c_void_p), len(steps)) == 0
    sp2 = speeds.copy()
    sp2['slot'] = np.where(speeds['slot'] >= 0, len(STEPS) - 1 - speeds['slot'], -1)
    try:
        assert _speed(world, rows, sp2, T, set_=h).tobytes() == got.tobytes()
    finally:
        torch.cuda.synchronize()
        world.lib.nafp_aug_speedset_destroy(h)


def test_inconsistent_entries_give_a_zero_event(world):
    """Entries with in-range pointers that are merely inconsistent -- no out-of-range address can arise from them: a slot equal to
    the number of steps, a negative slot other than -1, an out0 far beyond n_out (inside and outside what the host check accepts)."""
    T = 8000
    names, rows, speeds, got = _got(world, T)
    pick = [0, 1, 3, 6, 9, 12]                                   # speed rows with windows that exist: chains 0, 1, 3, 1, 4, 2
    assert all(speeds['slot'][i] >= 0 and _existing(speeds[i], T, STEPS) > 0 for i in pick)
    r, s = rows[pick].copy(), speeds[pick].copy()
    s['slot'][1] = len(STEPS)
    s['out0'][2] = 1 << 40
    s['out0'][3] = ref.n_out(int(s['n_in'][3]), STEPS[s['slot'][3]]) + 10 ** 6
    s['slot'][5] = -2
    out = _speed(world, r, s, T)
    zero = s.copy()                                              # the same rows with an event that does not exist: the composition's zero event
    zero['slot'] = np.where(np.isin(np.arange(6), [1, 2, 3, 5]), 0, s['slot'])
    zero['out0'] = np.where(np.isin(np.arange(6), [1, 2, 3, 5]), 1 << 31, s['out0'])
    want = _composition(world, r, zero, T)
    assert np.isfinite(out).all()
    assert out.tobytes() == want.tobytes()
    assert out[0].tobytes() == got[0].tobytes() and out[4].tobytes() == got[9].tobytes()      # the neighbours in the launch are untouched
    assert not out[5].any() and not out[2].any()                 # no mix: the zero event itself, also through an impulse response
    assert out[1].any() and out[3].any()                         # mixed: the noise alone, normalised (the reference's silent-event branch)


def test_through_the_loader(world):
    from neural_audio_fp_amd.model.utils.dataloader_keras import genUnbalSequence
    f = world.files
    args = dict(bsz=48, n_anchor=8, shuffle=True, random_offset_anchor=True, bg_mix_parameter=[True, f['bg'], (0, 10)],
                ir_mix_parameter=[True, f['ir']], speech_mix_parameter=[True, f['sp'], (3, 7)], seed=11)
    on = genUnbalSequence(f['ev'], speed_mix_parameter=[True, (0.8, 1.25), 7], **args)
    off = genUnbalSequence(f['ev'], **args)
    assert len(on.arena.host()) == len(world.arena) and on.arena.total == len(world.arena)      # the same arena as the fixture's
    n_speed = 0
    for idx in (0, 1, len(on) - 1):
        rows, speeds = on.plan(idx), on.plan_speed(idx)
        Xa, Xp = on[idx]
        assert Xa.shape == (8, 1, 8000) and Xp.shape == (40, 1, 8000) and Xa.dtype == torch.float32
        got = torch.cat([Xa, Xp])[:, 0].cpu().numpy()
        want = _composition(world, rows, speeds, 8000, steps=on.speed_steps)
        assert got.tobytes() == want.tobytes(), idx
        n_speed += int((speeds['slot'] >= 0).sum())
        # off: today's batch, from the same seed -- the plain entry on the same table; the anchors are the same in both
        Ya, Yp = off[idx]
        assert off.plan(idx).tobytes() == rows.tobytes()
        today = _plain(world, rows, 8000)
        assert torch.cat([Ya, Yp])[:, 0].cpu().numpy().tobytes() == today.tobytes()
        assert Ya.cpu().numpy().tobytes() == Xa.cpu().numpy().tobytes()
        unity = np.flatnonzero(speeds['slot'] == -1)
        assert got[unity].tobytes() == today[unity].tobytes()
    assert n_speed > 60
    # the synthesised queries (replicas only) take the same path
    q = genUnbalSequence(f['ev'], 16, 8, shuffle=False, bg_mix_parameter=[True, f['bg'], (0, 10)], ir_mix_parameter=[True, f['ir']],
                         speech_mix_parameter=[True, f['sp'], (3, 7)], reduce_batch_first_half=True, drop_the_last_non_full_batch=False,
                         speed_mix_parameter=[True, (0.9, 1.1), 3])
    assert q.arena.total == len(world.arena)                     # the same stores in the same places
    X, none = q[1]
    rows, speeds = q.plan(1), q.plan_speed(1)
    assert none == [] and X.shape == (8, 1, 8000) and (speeds['slot'][8:] >= 0).any()
    assert X[:, 0].cpu().numpy().tobytes() == _composition(world, rows[8:], speeds[8:], 8000, steps=q.speed_steps).tobytes()
