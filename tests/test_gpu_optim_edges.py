"""GPU: the Adam / LAMB kernels (csrc/optim.hip) term by term at their edges, against the float64 oracle through the two-stage
comparison of tests/_optim_ref.py (its docstring derives the bounds by counting roundings): m and v to 4U of their absolute terms,
the weights to 2U |w| + K U |step| (K = 16 Adam, 32 LAMB) from the kernel's own float32 m, v, one step at a time.  The cases
(tests/_optim_ref.py: cases()) hold ragged last blocks of multi-block tensors, stackings on every path of the per-variable norm sum,
both launches of a table of more than 48 tensors, tables of exactly 48 and 49, each of p / g / m / v on its own 4 bytes off the 16-byte
grid, epsilon- and decay-dominated steps, zero gradients, weights and variables, and steps 1 to 10^6; each runs through the C entry
points and, where the wrapper can express it, through Adam / LAMB.apply_gradients.  tests/test_optim_ref_host.py shows that these cases
catch every listed mutation at these bounds.

A refused step changes nothing: a table of 50 real tensors whose 50th alone is invalid returns the error code and leaves p, m, v of
all 50 bit-identical (before the whole-table check in front of the first launch, tensors 0..47 had been updated by then).

OBSERVED ON THE MI355X (maxima over all cases, in the units of the bounds; the `observe` fixture records each case next to its bound):
                                   m [U]         v [U]         w, excess over 2U |w| [U of the step]
  Adam, C entry points / wrapper   1.84 of 4     1.95 of 4      1.99 of 16   (step_1, wd_0p1_eps_1e-3, step_2)
  LAMB, C entry points / wrapper   1.84 of 4     1.95 of 4      4.50 of 32   (step_1, wd_0p1_eps_1e-3, step_1)
  three steps on the GPU           1.79 of 4     1.93 of 4      1.39 of 16 (Adam), 3.53 of 32 (LAMB)
  No kernel misses a bound.  The float32 emulation reaches 1.89 / 2.76 / 1.89 (Adam) and 5.47 (LAMB) on the same cases: the kernels fuse
  a product into the sums of m and v, the emulation rounds it.  The zero cases are exact (0 of every bound).
"""
import numpy as np
import pytest
import torch

import _optim_ref as R

pytestmark = pytest.mark.gpu
INV = 1                                       # NAFP_ERR_INVALID_ARG
SENTINEL = 12345.5


class Dev:
    """A float32 array on the GPU inside an allocation of n + 2 floats whose spare elements hold a sentinel; `misaligned` starts it
    4 bytes into the allocation (x[1:] is contiguous: the wrapper takes it too)."""

    def __init__(self, a, misaligned=False):
        self.buf = torch.full((a.size + 2,), SENTINEL, dtype=torch.float32, device='cuda')
        self.t = self.buf[1:1 + a.size] if misaligned else self.buf[:a.size]
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == (4 if misaligned else 0)
        self.spare = [0, a.size + 1] if misaligned else [a.size, a.size + 1]

    def get(self):
        buf = self.buf.cpu().numpy()
        assert all(buf[i] == SENTINEL for i in self.spare), 'the kernel wrote outside its tensor'
        return self.t.cpu().numpy().copy()


def _upload(tensors):
    return [{k: Dev(getattr(t, a), t.misalign == k) for k, a in (('p', 'w'), ('g', 'g'), ('m', 'm'), ('v', 'v'))} for t in tensors]


def _opt_table(nafp, dev, tensors):
    arr = (nafp._lib.OptTensor * len(dev))()
    for i, (d, t) in enumerate(zip(dev, tensors)):
        arr[i] = nafp._lib.OptTensor(d['p'].t.data_ptr(), d['g'].t.data_ptr(), d['m'].t.data_ptr(), d['v'].t.data_ptr(), t.w.size, t.var_len)
    return arr


def _c_step(nafp, kind, arr, hp, step, ws=None):
    """One step through the C entry points; returns the status."""
    lib, raw = nafp._lib.load(), hp.raw
    stream = nafp._lib.current_stream()
    if kind == 'adam':
        rc = lib.nafp_adam_step(arr, len(arr), raw['lr'], raw['b1'], raw['b2'], raw['eps'], step, stream)
    else:
        need = int(lib.nafp_lamb_workspace_bytes(arr, len(arr)))
        if ws is None:
            assert need > 0
            ws = torch.empty((need,), dtype=torch.uint8, device='cuda')
        rc = lib.nafp_lamb_step(arr, len(arr), raw['lr'], raw['b1'], raw['b2'], raw['eps'], raw['wd'], step, nafp._lib.ptr(ws), ws.numel(), stream)
    torch.cuda.synchronize()
    return rc


def _make_optimizer(kind, hp):
    from neural_audio_fp_amd.model.fp import lamb_optimizer as m
    raw = hp.raw
    if kind == 'adam':
        return m.Adam(learning_rate=raw['lr'], beta_1=raw['b1'], beta_2=raw['b2'], epsilon=raw['eps'])
    return m.LAMB(learning_rate=raw['lr'], beta_1=raw['b1'], beta_2=raw['b2'], epsilon=raw['eps'], weight_decay_rate=raw['wd'])


def _check(kind, tensors, new, hp, step, observe, tag):
    worst = {'m': 0.0, 'v': 0.0, 'w': 0.0}
    for t, (wn, mn, vn) in zip(tensors, new):
        obs = R.compare(kind, (t.w, t.g, t.m, t.v), (wn, mn, vn), t.var_len, hp, step)
        worst = {k: max(worst[k], obs[k]) for k in worst}
    print(f'{tag} {kind}: ' + ', '.join(f'{k} {worst[k]:.3f} / {b:g}' for k, b in R.bounds(kind).items()))
    for k, b in R.bounds(kind).items():
        observe(f'{tag} {k} [U]', worst[k], b * (1 + 1e-12))
    return worst


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('case', R.cases(), ids=R.case_ids())
def test_c_entry_points(nafp, observe, kind, case):
    hp = case.hp(kind)
    dev = _upload(case.tensors)
    assert _c_step(nafp, kind, _opt_table(nafp, dev, case.tensors), hp, case.step) == 0
    new = [(d['p'].get(), d['m'].get(), d['v'].get()) for d in dev]
    for t, d in zip(case.tensors, dev):
        assert np.array_equal(d['g'].get(), t.g)                                    # the gradient is read only
    _check(kind, case.tensors, new, hp, case.step, observe, 'C')
    if case.name == 'zero_weights_and_gradient':
        assert all((w == 0).all() and (m == 0).all() and (v == 0).all() for w, m, v in new)      # exactly 0
    if case.name == 'zero_gradient' and kind == 'lamb':                                 # update = wd w, ratio = 1 / wd: w_new = w (1 - lr)
        for t, (w, _, _) in zip(case.tensors, new):
            w64 = t.w.astype(np.float64)                                               # 2U |w (1 - lr)| + 32U |lr w| <= 10U |w| at lr = 1/4
            assert (np.abs(w - w64 * (1 - hp.lr)) <= 10 * R.U * np.abs(w64)).all()


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('case', [c for c in R.cases() if not any(t.misalign in ('m', 'v') for t in c.tensors)],
                         ids=lambda c: c.name)       # the wrapper owns m and v: it cannot misalign them
def test_apply_gradients(nafp, observe, kind, case):
    hp = case.hp(kind)
    dev = _upload(case.tensors)
    ws, gs = [d['p'].t for d in dev], [d['g'].t for d in dev]
    opt = _make_optimizer(kind, hp)
    opt.load_state_dict({'iterations': case.step - 1, 'm': [torch.from_numpy(t.m) for t in case.tensors],
                         'v': [torch.from_numpy(t.v) for t in case.tensors]}, ws)
    opt.apply_gradients(zip(gs, ws), var_lens=[t.var_len for t in case.tensors])
    torch.cuda.synchronize()
    assert opt.iterations == case.step
    sd = opt.state_dict(ws)
    new = [(d['p'].get(), m.numpy(), v.numpy()) for d, m, v in zip(dev, sd['m'], sd['v'])]
    _check(kind, case.tensors, new, hp, case.step, observe, 'wrapper')               # fails if the loaded m, v were not the ones used


def _small_table(name, n=6):
    return R.make_table(name, [(1, 4097), (6, 96), (3, 96), (1, 5), (130, 33), (1, 8193)][:n], 'normal')


@pytest.mark.parametrize('kind', R.KINDS)
def test_three_steps_with_the_state_on_the_gpu(nafp, observe, kind):
    """m and v persist in the optimizer's slots; the reference is re-seeded from the GPU's float32 state at every step.  The second
    and third apply_gradients see the same buffers and take the cached table."""
    tensors = _small_table('three_steps')
    for t in tensors:
        t.m[:], t.v[:] = 0, 0
    hp = R.HP(kind)
    dev = _upload(tensors)
    ws, gs = [d['p'].t for d in dev], [d['g'].t for d in dev]
    opt = _make_optimizer(kind, hp)
    rng = np.random.default_rng(11)
    table = None
    for step in (1, 2, 3):
        for t, d in zip(tensors, dev):
            t.g = rng.normal(size=t.g.size).astype(np.float32)
            d['g'].t.copy_(torch.from_numpy(t.g))                  # same buffer, new values
        opt.apply_gradients(zip(gs, ws), var_lens=[t.var_len for t in tensors])
        torch.cuda.synchronize()
        if table is None:
            table = opt._cache[1]
        assert opt._cache[1] is table                              # built once
        sd = opt.state_dict(ws)
        new = [(d['p'].get(), m.numpy().copy(), v.numpy().copy()) for d, m, v in zip(dev, sd['m'], sd['v'])]
        _check(kind, tensors, new, hp, step, observe, f'step {step}')
        for t, (w, m, v) in zip(tensors, new):
            t.w, t.m, t.v = w, m, v
    assert opt.iterations == 3 and all(np.abs(t.m).max() > 0 for t in tensors)


def test_load_state_dict_then_step_uses_the_loaded_moments(nafp):
    tensors = _small_table('loaded', 3)
    out = []
    for loaded in (True, False):
        dev = _upload(tensors)
        ws = [d['p'].t for d in dev]
        opt = _make_optimizer('adam', R.HP('adam'))
        if loaded:
            opt.load_state_dict({'iterations': 4, 'm': [torch.from_numpy(t.m) for t in tensors], 'v': [torch.from_numpy(t.v) for t in tensors]}, ws)
        else:
            opt.iterations = 4
        opt.apply_gradients(zip([d['g'].t for d in dev], ws))
        torch.cuda.synchronize()
        out.append(([d['p'].get() for d in dev], opt.state_dict(ws)))
    hp = R.HP('adam')
    for i, t in enumerate(tensors):
        obs = R.compare('adam', (t.w, t.g, t.m, t.v), (out[0][0][i], out[0][1]['m'][i].numpy(), out[0][1]['v'][i].numpy()), t.var_len, hp, 5)
        assert not R.misses('adam', obs), obs
        assert not np.array_equal(out[0][0][i], out[1][0][i])      # ... and zero slots give other weights


def test_adam_is_repeatable_bit_for_bit(nafp):
    """Adam has no atomics: the same state gives the same bits.  (No such claim for LAMB: its norms are summed with double atomics.)"""
    case = R.cases()[0]
    hp = case.hp('adam')
    runs = []
    for _ in range(2):
        dev = _upload(case.tensors)
        assert _c_step(nafp, 'adam', _opt_table(nafp, dev, case.tensors), hp, case.step) == 0
        runs.append([(d['p'].get(), d['m'].get(), d['v'].get()) for d in dev])
    for a, b in zip(*runs):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('defect', ['numel_not_a_multiple_of_var_len', 'null_grad'])
def test_refused_step_changes_nothing(nafp, kind, defect):
    """50 real tensors, only the 50th invalid -- it sits in the SECOND launch.  The error code comes back and p, m, v of all 50 are
    bit-identical to before.  Every pointer is a real allocation of the right size."""
    tensors = R.make_table('refused', [(1, 60 + i) for i in range(49)] + [(3, 96)], 'normal')
    dev = _upload(tensors)
    arr = _opt_table(nafp, dev, tensors)
    ws = torch.empty((int(nafp._lib.load().nafp_lamb_workspace_bytes(arr, 50)),), dtype=torch.uint8, device='cuda')
    if defect == 'null_grad':
        arr[49].grad = None
    else:
        arr[49].var_len = 7                                        # 288 % 7 == 1
    assert _c_step(nafp, kind, arr, R.HP(kind), 2, ws=ws) == INV
    for i, (t, d) in enumerate(zip(tensors, dev)):
        assert np.array_equal(d['p'].get(), t.w) and np.array_equal(d['m'].get(), t.m) and np.array_equal(d['v'].get(), t.v), i
    # the same table, mended, steps
    arr = _opt_table(nafp, dev, tensors)
    assert _c_step(nafp, kind, arr, R.HP(kind), 2, ws=ws) == 0
    assert not np.array_equal(dev[0]['p'].get(), tensors[0].w) and not np.array_equal(dev[49]['m'].get(), tensors[49].m)
