"""GPU: the NT-Xent kernels (csrc/ntxent.hip: first generation, second generation, the symmetric and the fused ROW + COL backward)
at their edges, element by element against the float64 reference and the a-priori bounds of tests/_ntxent_ref.py.

Every call goes through the harness of tests/_ntxent_worker.py: NaN-filled workspace and outputs, 4096 guard bytes behind the
stated workspace size.  Every observed error / bound is recorded through `observe(..., 1.0)`.  That the bounds are tight enough
to see one wrong row is the business of tests/test_ntxent_ref_host.py (no GPU needed)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _ntxent_ref as nr
import _ntxent_worker as W

pytestmark = pytest.mark.gpu


def _check(case, observe):
    out, ratios = W.run_case(case)
    assert out['guard'], 'write beyond nafp_ntxent_workspace_bytes'
    assert W.all_finite(out), 'an output element was never written, or a partial was read before it was written'
    for kind in nr.KINDS:
        observe(f'{kind} error / bound', ratios[kind], 1.0)
    return out


@pytest.mark.parametrize('case', nr.GEOMETRY, ids=repr)
def test_tile_and_owner_geometry(nafp, observe, case):
    """n = 16, 17, 32, 33: self and positive column in one tile, in two, on a tile boundary; 64 / 65: a second 128-owner block with 2
    valid owners; 521: 33 tiles, 2 per split, the ragged one alone in the last split; 530: 34 tiles, the ragged one (4 valid columns)
    second in its split.  d = 64: the NB = 2 store path; d = 256: the first-generation kernels."""
    out = _check(case, observe)
    if case.n == 1:                       # one admissible column per row: the reference's loss and gradient are exactly 0
        want = case.ref()
        assert want.loss_sum == 0.0 and not want.d_org.any() and not want.d_rep.any()
        assert abs(out['loss']) <= want.b_loss_sum


@pytest.mark.parametrize('case', nr.PER_ROW, ids=repr)
def test_per_row_losses(nafp, observe, case):
    """n_local = 1: loss_sum is CE_a(i) + CE_b(i) of ONE anchor -- a single row's log-sum-exp seen from outside (and owner blocks with
    2 valid owners of 128)."""
    _check(case, observe)


@pytest.mark.parametrize('case', nr.SHARDS, ids=repr)
def test_ragged_shards(nafp, observe, case):
    """Unequal, unaligned shards of 530: loss_sum, the sharded sim_mtx (n_local x 1059) and both gradient contributions."""
    out = _check(case, observe)
    assert out['sim'].shape == (case.n_local, 1059)


def test_unequal_shards_cover_sums_to_single_device_gradient(nafp, observe):
    full_case = nr.Case('geometry', 530)
    full, want = W.run_case(full_case)[0], full_case.ref()
    tot = {k: np.zeros((530, 128)) for k in ('d_org', 'd_rep')}
    bound = {k: np.zeros((530, 128)) for k in ('d_org', 'd_rep')}
    loss, b_loss = 0.0, 0.0
    for case in nr.COVER:
        out, r = _check(case, observe), case.ref()
        for k in tot:
            tot[k] += out[k].astype(np.float64)
            bound[k] += getattr(r, 'b_' + k)
        loss += out['loss']; b_loss += r.b_loss_sum
    for k in tot:
        observe(f'{k}: cover vs reference', nr.ratio(np.abs(tot[k] - getattr(want, k)), bound[k]), 1.0)
        observe(f'{k}: cover vs single-device call',
                nr.ratio(np.abs(tot[k] - full[k].astype(np.float64)), bound[k] + getattr(want, 'b_' + k)), 1.0)
    observe('loss: cover vs reference', abs(loss - want.loss_sum) / b_loss, 1.0)


def test_fused_row_col_launch_agrees_with_symmetric_pass(nafp, observe):
    """n_local = n_global = 530 with cloned local buffers takes the fused ROW + COL launch; the pointer-identical call the symmetric
    single pass.  Same reference, so they agree to the sum of their bounds."""
    cloned_case = [c for c in nr.SHARDS if c.clone][0]
    cloned, sym, want = W.run_case(cloned_case)[0], W.run_case(nr.Case('geometry', 530))[0], cloned_case.ref()
    assert cloned['guard'] and sym['guard'] and W.all_finite(cloned) and W.all_finite(sym)
    for k in ('d_org', 'd_rep'):
        observe(f'{k} difference / bound', nr.ratio(np.abs(cloned[k].astype(np.float64) - sym[k]), 2 * getattr(want, 'b_' + k)), 1.0)
    observe('sim difference / bound', nr.ratio(np.abs(cloned['sim'].astype(np.float64) - sym['sim']), 2 * want.b_sim), 1.0)
    observe('loss difference / bound', abs(cloned['loss'] - sym['loss']) / (2 * want.b_loss_sum), 1.0)


@pytest.mark.parametrize('case', nr.TEMPERATURE + nr.MAGNITUDE, ids=repr)
def test_temperature_and_magnitude(nafp, observe, case):
    """tau from 0.01 to 1 (the 1 / tau float pair, the folded log2 scale, the online log-sum-exp far from [-20, 20]); embeddings scaled
    by 3 (logits up to 180); exact duplicates (ties at the row maximum, a positive equal to its anchor)."""
    _check(case, observe)


def test_nan_input_gives_nan_loss(nafp):
    a, b = nr.NAN_CASE.inputs()
    out = W.call(a, b, 33, 0, 0.05)
    assert out['guard']
    assert np.isnan(nr.NAN_CASE.ref().loss_sum) and np.isnan(out['loss'])


def test_two_calls_are_bit_identical(nafp):
    """The kernels promise a fixed summation order."""
    case = nr.DETERMINISM
    a, b = case.inputs()
    for n_local, off in ((case.n_local, case.off), (case.n, 0)):
        x, y = W.call(a, b, n_local, off, case.tau), W.call(a, b, n_local, off, case.tau)
        assert x['guard'] and y['guard']
        assert np.float32(x['loss']).tobytes() == np.float32(y['loss']).tobytes()
        for k in ('sim', 'd_org', 'd_rep'):
            assert x[k].tobytes() == y[k].tobytes(), k


ENV_PATHS = (('NAFP_NTXENT_V2', '0'),             # the first-generation kernels at d = 64 / 128
             ('NAFP_NTXENT_SYM', '0'),            # single device through the fused ROW + COL launch
             ('NAFP_NTXENT2_MAXSPLIT', '1'),      # one split walks all 34 tiles: the deepest double-buffered loop
             ('NAFP_NTXENT2_MAXSPLIT', '3'))


def test_environment_selected_paths(nafp, observe):
    """The library reads these variables once per process: each setting runs tests/_ntxent_worker.py in a fresh child, one at a time."""
    import json
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_ntxent_worker.py')
    base = {k: v for k, v in os.environ.items() if not k.startswith('NAFP_NTXENT')}
    for var, val in ENV_PATHS:
        res = subprocess.run([sys.executable, worker], env=dict(base, **{var: val}), capture_output=True, text=True, timeout=180)
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith('{')]
        assert lines, (var, val, res.returncode, res.stdout[-2000:], res.stderr[-2000:])
        rep = json.loads(lines[-1])
        bad = {n: c for n, c in rep['cases'].items() if not (c['guard'] and c['finite'])}
        assert not bad, (var, val, bad)
        for kind in nr.KINDS:
            observe(f'{var}={val} {kind} error / bound', rep['worst'][kind], 1.0)
        assert res.returncode == 0 and rep['ok'], (var, val, res.returncode, res.stderr[-2000:])
