"""GPU: nafp_varispeed_i16 (csrc/varispeed.hip) against the numpy restatement tests/_varispeed_ref.py -- BIT EQUALITY everywhere:
the arithmetic is exact integer arithmetic, so there is no tolerance to set.

Every launch here goes through one helper: each piece's source samples are only what nafp_varispeed_input_range names, uploaded
between runs of garbage; the output arena is full of a sentinel, with gaps between the pieces' output ranges; the pieces are
shuffled.  The helper checks the outputs against the restatement and that every int16 outside the output ranges kept the sentinel."""
import ctypes

import numpy as np
import pytest

import _varispeed_ref as ref

pytestmark = pytest.mark.gpu
ONE = 1 << 24
SENTINEL, GARBAGE = 12345, -23131
STEPS = [ref.STEP_MIN, ref.STEP_MAX, ONE, ONE + 1, ref.step_for(1.04), ref.step_for(0.96), ref.step_for(1.0137)]
_TABLES, _WANT = {}, {}


def _table(step):
    if step not in _TABLES:
        _TABLES[step] = ref.table(step)
    return _TABLES[step]


def _inputs(n_in):
    """name -> int16 file of n_in samples."""
    rng = np.random.default_rng(1000 + n_in)
    return {'noise': rng.integers(-32768, 32768, size=n_in).astype(np.int16),
            'square': np.where((np.arange(n_in) // 32) % 2 == 0, 32767, -32767).astype(np.int16),
            'floor': np.full(n_in, -32768, np.int16)}


def _launch(vs, torch, step, files, cuts, seed=0, shuffle=True, out=None, return_arenas=False):
    """files: list of int16 arrays; cuts[i]: outputs per piece of file i (None: one piece).  Returns the outputs per file."""
    rng = np.random.default_rng(seed)
    rows, src_parts, src_at, out_at, where = [], [], 0, 3, []
    for i, x in enumerate(files):
        n_total = ref.n_out(len(x), step)
        cut = n_total if not cuts[i] else cuts[i]
        for o0 in range(0, max(n_total, 1), max(cut, 1)):
            o1 = min(n_total, o0 + cut)
            first, last = vs.input_range(o0, o1, len(x), step)
            pad = int(rng.integers(1, 9))
            src_parts += [np.full(pad, GARBAGE, np.int16), x[first:last], np.full(3, GARBAGE, np.int16)]
            rows.append((src_at + pad, first, last - first, len(x), o0, out_at, o1 - o0, 0))
            where.append((i, o0, o1, out_at))
            src_at += pad + (last - first) + 3
            out_at += (o1 - o0) + int(rng.integers(1, 7))
    order = rng.permutation(len(rows)) if shuffle else np.arange(len(rows))
    pieces = np.array([rows[k] for k in order], dtype=vs.PIECE_DTYPE)
    src = torch.from_numpy(np.concatenate(src_parts)).cuda()
    host_out = np.full(out_at + 5, SENTINEL, np.int16)
    d_out = torch.from_numpy(host_out.copy()).cuda()
    vs.plan_for(step).run(src, pieces, d_out)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    outs = [np.zeros(ref.n_out(len(x), step), np.int16) for x in files]
    untouched = np.ones(len(got), bool)
    for i, o0, o1, at in where:
        outs[i][o0:o1] = got[at:at + o1 - o0]
        untouched[at:at + o1 - o0] = False
    assert np.all(got[untouched] == SENTINEL), 'an int16 outside the pieces\' output ranges was written'
    return (outs, got) if return_arenas else outs


@pytest.mark.parametrize('step', STEPS)
def test_every_input_and_length(nafp, step):
    import torch
    from neural_audio_fp_amd.model.utils import varispeed as vs
    W, T = ref.geometry(step)
    tab = _table(step)
    assert vs.geometry(step) == (W, T)
    files, names = [], []
    for n_in in (1, 2 * W - 1, 255, 256, 257, 3000):
        for name, x in _inputs(n_in).items():
            files.append(x); names.append((n_in, name))
    outs = _launch(vs, torch, step, files, [None] * len(files), seed=step % 1000)
    fracs = set()
    for (n_in, name), x, y in zip(names, files, outs):
        acc = ref.accumulate(x, step, tab)
        assert np.array_equal(y, ref.finish(acc)), (step, n_in, name, int(np.flatnonzero(y != ref.finish(acc))[0]))
        if name == 'square' and n_in == 3000:                  # the Gibbs overshoot leaves the int16 range on both sides: the clamp is used
            assert ref.unclamped(acc).max() > 32767 and ref.unclamped(acc).min() < -32768
            assert y.max() == 32767 and y.min() == -32768
        if name == 'floor' and n_in == 3000:
            assert np.all(y[2 * W:-2 * W] == -32768)
        fracs.update(int(v) for v in (np.arange(len(y), dtype=np.int64) * step) & (ONE - 1))
    assert 0 in fracs                                          # frac == 0: output 0 of every file
    assert any(s % 2 for s in STEPS)                           # the case below is among the cases
    if step % 2:
        # an odd step reaches every fraction; the last one, p == 511 with w == 32767, at n * step = -1 mod 2^24: a piece around
        # that output of a long file, of which only the samples it reads exist here
        n_star = (-pow(step, -1, ONE)) % ONE
        pos, p, w = ref.phases(np.array([n_star]), step)
        assert (int(p[0]), int(w[0])) == (511, 32767)
        n_in = int(pos[0]) + 2000
        o0, o1 = n_star - 300, n_star + 300
        first, last = vs.input_range(o0, o1, n_in, step)
        held = np.random.default_rng(3).integers(-32768, 32768, size=last - first).astype(np.int16)
        pieces = np.array([(2, first, last - first, n_in, o0, 1, o1 - o0, 0)], dtype=vs.PIECE_DTYPE)
        src = torch.from_numpy(np.concatenate([[GARBAGE] * 2, held, [GARBAGE] * 2]).astype(np.int16)).cuda()
        d_out = torch.full((o1 - o0 + 2,), SENTINEL, dtype=torch.int16, device='cuda')
        vs.plan_for(step).run(src, pieces, d_out)
        got = d_out.cpu().numpy()
        want = ref.finish(ref.accumulate(held, step, tab, n=np.arange(o0, o1), frame0=first))
        assert np.array_equal(got[1:-1], want) and got[0] == SENTINEL and got[-1] == SENTINEL


@pytest.mark.parametrize('step', [ref.step_for(1.04), ref.STEP_MAX, ref.STEP_MIN])
def test_pieces(nafp, step):
    """However a file's outputs are cut into pieces, and whatever shares the launch, the bytes are those of its one-piece output."""
    import torch
    from neural_audio_fp_amd.model.utils import varispeed as vs
    tab = _table(step)
    rng = np.random.default_rng(8)
    a, b = rng.integers(-32768, 32768, size=3000).astype(np.int16), rng.integers(-32768, 32768, size=1777).astype(np.int16)
    want_a, want_b = ref.varispeed(a, step, tab), ref.varispeed(b, step, tab)
    (one,) = _launch(vs, torch, step, [a], [None])
    assert np.array_equal(one, want_a)
    for cut in (1, 255, 256, 257, 997):
        (got,) = _launch(vs, torch, step, [a], [cut], seed=cut)
        assert np.array_equal(got, one), cut
    # two files in one launch, their pieces shuffled together
    ga, gb = _launch(vs, torch, step, [a, b], [257, 255], seed=99)
    assert np.array_equal(ga, want_a) and np.array_equal(gb, want_b)
    # two runs: identical bytes
    first = _launch(vs, torch, step, [a, b], [997, 256], seed=5, return_arenas=True)[1]
    again = _launch(vs, torch, step, [a, b], [997, 256], seed=5, return_arenas=True)[1]
    assert first.tobytes() == again.tobytes()


def test_inconsistent_piece_is_zeroed(nafp):
    """A piece whose samples are not all present is skipped with its outputs zeroed, its neighbours are intact, nothing is written
    for a piece whose output range leaves the arena, and the host check reports both."""
    import torch
    from neural_audio_fp_amd.model.utils import varispeed as vs
    lib = nafp._lib.load()
    step = ref.step_for(0.96)
    tab = _table(step)
    x = np.random.default_rng(9).integers(-32768, 32768, size=3000).astype(np.int16)
    want = ref.varispeed(x, step, tab)
    cuts = [(0, 600), (600, 1300), (1300, 2000)]
    rows, at = [], 0
    for o0, o1 in cuts:
        first, last = vs.input_range(o0, o1, len(x), step)
        rows.append([first, first, last - first, len(x), o0, at, o1 - o0, 0])        # the whole file is uploaded: src_off = frame0
        at += o1 - o0 + 4
    good = np.array([tuple(r) for r in rows], dtype=vs.PIECE_DTYPE)
    out_n = at + 10
    call = lambda pcs: lib.nafp_varispeed_check_pieces_host(step, pcs.ctypes.data_as(ctypes.c_void_p), len(pcs), len(x), out_n)
    assert call(good) == 0
    bad = good.copy()
    bad[1]['frame0'] += 1; bad[1]['src_off'] += 1                                   # its first sample is "not present"
    assert call(bad) == 1
    with pytest.raises(nafp._lib.NafpError):
        vs.check_pieces(step, bad, len(x), out_n)
    gone = bad.copy()
    gone[2]['out_off'] = out_n - 5                                                  # its outputs would leave the arena
    assert call(gone) == 1
    unsupported = good.copy()
    unsupported[0]['n_in'] = 1 << 31
    assert call(unsupported) == 2
    src = torch.from_numpy(x).cuda()
    for pcs in (bad, gone):
        d_out = torch.full((out_n,), SENTINEL, dtype=torch.int16, device='cuda')
        d_p = torch.from_numpy(pcs.view(np.uint8).reshape(-1).copy()).cuda()
        plan = vs.plan_for(step)
        assert lib.nafp_varispeed_i16(plan.handle, nafp._lib.ptr(src), src.numel(), nafp._lib.ptr(d_p), len(pcs), nafp._lib.ptr(d_out),
                                      out_n, nafp._lib.current_stream()) == 0
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        expect = np.full(out_n, SENTINEL, np.int16)
        expect[rows[0][5]:rows[0][5] + 600] = want[0:600]
        expect[rows[1][5]:rows[1][5] + 700] = 0
        if pcs is bad:
            expect[rows[2][5]:rows[2][5] + 700] = want[1300:2000]
        assert np.array_equal(got, expect)


def test_status_codes_before_any_gpu_call(nafp):
    import torch
    from neural_audio_fp_amd.model.utils import varispeed as vs
    lib, L = nafp._lib.load(), nafp._lib
    h = ctypes.c_void_p()
    assert lib.nafp_varispeed_create(ctypes.byref(h), ref.STEP_MIN - 1) == 2 and lib.nafp_varispeed_create(ctypes.byref(h), ref.STEP_MAX + 1) == 2
    assert lib.nafp_varispeed_create(None, ONE) == 1
    plan = vs.plan_for(ONE)
    buf = torch.zeros(64, dtype=torch.int16, device='cuda')
    pcs = torch.zeros(56, dtype=torch.uint8, device='cuda')
    args = lambda **kw: [kw.get('plan', plan.handle), kw.get('src', L.ptr(buf)), kw.get('n_src', 64), kw.get('pieces', L.ptr(pcs)), kw.get('n', 1),
                         kw.get('out', L.ptr(buf)), kw.get('n_out', 64), None]
    for kw in (dict(plan=None), dict(src=None), dict(out=None), dict(pieces=None), dict(n=-1), dict(n_src=-1), dict(n_out=-1)):
        assert lib.nafp_varispeed_i16(*args(**kw)) == 1, kw
    assert lib.nafp_varispeed_i16(*args(n=0)) == 0
    with pytest.raises(TypeError):
        plan.run(buf.to(torch.int32), np.zeros(0, vs.PIECE_DTYPE), buf)
    with pytest.raises(ValueError, match='outside'):
        vs.plan_for(ref.STEP_MAX + 1)
