"""CPU: the float64 NT-Xent reference of tests/_ntxent_ref.py against oracle/ntxent.py, and the condition that keeps its bounds
honest: every mutant (one wrong row) leaves the bounds of the unmutated reference, for every input set the GPU tests compare."""
import numpy as np
import pytest

import _ntxent_ref as nr
from oracle import ntxent as o_nt


def _t32(tau):
    return float(np.float32(tau))


@pytest.mark.parametrize('n,d,tau', [(1, 128, 0.05), (2, 128, 0.05), (5, 64, 0.5), (33, 128, 0.05), (65, 256, 0.05), (97, 128, 0.01)])
def test_reference_equals_oracle_single_device(n, d, tau):
    a, b = nr.pairs(n, d, tau)
    r = nr.ref(a, b, n, 0, tau)
    loss, sim, _ = o_nt.compute_loss(a, b, tau=_t32(tau))
    ga, gb = o_nt.grad_embeddings(a, b, tau=_t32(tau))
    assert abs(r.loss_sum / n - loss) < 1e-12 * max(1.0, abs(loss))
    assert r.loss_rows.shape == (2 * n,) and abs(r.loss_rows.sum() - r.loss_sum) < 1e-12 * max(1.0, abs(r.loss_sum))
    assert r.sim.shape == (n, 2 * n - 1) and np.abs(r.sim - sim).max() < 1e-12 * max(1.0, np.abs(sim).max())
    assert np.abs(r.d_org - ga).max() < 1e-12 and np.abs(r.d_rep - gb).max() < 1e-12
    if n == 1:
        assert r.loss_sum == 0.0 and not r.d_org.any() and not r.d_rep.any()


@pytest.mark.parametrize('ranks,n_a,d', [(4, 10, 128), (3, 11, 64), (2, 33, 128)])
def test_reference_equals_replica_loss_and_shards_sum_to_full_gradient(ranks, n_a, d):
    n = ranks * n_a
    a, b = nr.pairs(n, d, 0.05)
    tot_a, tot_b, total = np.zeros((n, d)), np.zeros((n, d)), 0.0
    full = nr.ref(a, b, n, 0, 0.05)
    for k in range(ranks):
        sl = slice(k * n_a, (k + 1) * n_a)
        r = nr.ref(a, b, n_a, k * n_a, 0.05)
        want = o_nt.replica_loss_fn(np.concatenate([a[sl], b[sl]]), a, b, k, _t32(0.05))
        assert np.abs(r.loss_rows[:n_a] + r.loss_rows[n_a:] - want).max() < 1e-12 * max(1.0, np.abs(want).max())
        assert np.abs(r.sim - full.sim[sl]).max() < 1e-12           # a shard's sim_mtx is its rows of the single-device one
        assert np.allclose(r.b_sim, full.b_sim[sl], rtol=1e-12, atol=0)
        tot_a += r.d_org; tot_b += r.d_rep; total += r.loss_sum
    ga, gb = o_nt.grad_embeddings(a, b, tau=_t32(0.05))
    assert np.abs(tot_a - ga).max() < 1e-12 and np.abs(tot_b - gb).max() < 1e-12
    assert abs(total - full.loss_sum) < 1e-12 * abs(full.loss_sum)


def test_unequal_shards_sum_to_full_gradient():
    a, b = nr.pairs(65, 128, 0.05)
    full = nr.ref(a, b, 65, 0, 0.05)
    parts = [nr.ref(a, b, nl, off, 0.05) for nl, off in ((7, 0), (20, 7), (1, 27), (37, 28))]
    assert np.abs(sum(p.d_org for p in parts) - full.d_org).max() < 1e-12
    assert np.abs(sum(p.d_rep for p in parts) - full.d_rep).max() < 1e-12


def test_reference_is_inside_its_own_bounds_and_nan_propagates():
    c = nr.Case('x', 33)
    assert nr.compare(nr.as_outputs(c.ref()), c.ref()) == {'loss': 0.0, 'sim': 0.0, 'grad': 0.0}
    a, b = nr.NAN_CASE.inputs()
    r = nr.ref(a, b, 33, 0, 0.05)
    assert np.isnan(r.loss_sum)
    assert not (nr.ratio(np.array([np.nan, 0.0]), np.ones(2)) < 1.0)


def test_cover_is_a_partition():
    assert sorted((c.off, c.off + c.n_local) for c in nr.COVER) == [(0, 77), (77, 277), (277, 278), (278, 530)]


@pytest.mark.parametrize('case', nr.all_compared_cases(), ids=repr)
def test_every_mutant_leaves_the_bounds(case):
    """One wrong row must show: the mutated reference, compared like a kernel's output, exceeds the bound of the unmutated
    reference in every output kind the mutant changes."""
    want = case.ref()
    for mutant in nr.MUTANTS:
        if not nr.mutant_applies(case, mutant):
            continue
        got = nr.compare(nr.as_outputs(case.ref(mutate=mutant)), want)
        for kind in nr.mutant_kinds(case, mutant):
            assert got[kind] > 1.0, (case, mutant, kind, got[kind])
