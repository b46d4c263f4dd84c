"""CPU: the references, input sets and mutants of the exact-search edge tests (tests/_search_ref.py) hold what the GPU tests
(tests/test_gpu_search_edges.py) rely on: the references agree with oracle/search.py, the exactness premise holds, the exact
sets are rich in ties at the k-th place, and every mutant fails the GPU tests' own comparison on every set it applies to."""
import numpy as np
import pytest

import _search_ref as sr
from oracle import search as S

EXACT_MUTANTS = tuple(m for m in sr.MUTANTS if m != 'clamp_missing')


def _same_bytes(got, want):
    """The comparison of the exact GPU cases: ids equal, distance bytes equal."""
    return np.array_equal(got[1], want[1]) and got[0].tobytes() == want[0].tobytes()


def _exact_sets():
    """(name, q, x, k, nq_launch) of every exact set the GPU tests use."""
    for c in sr.GEOMETRY + list(sr.BEHIND + sr.SHORT + sr.IVF + sr.LARGE) + [sr.PREFIX]:
        q, x = sr.case_inputs(c)
        yield c.name, q, x, c.k, c.nq
    q, sample = sr.large_many_queries()
    yield 'large-many', q[sample], sr.case_inputs(sr.LARGE[0])[1], 20, sr.LARGE_NQ_MANY
    for d in sr.DIMS:
        for k in (20, 32):
            for sc in sr.PLACED_SCENARIOS:
                q, x, _ = sr.placed_set(d, k, sc)
                yield f'placed-{sc}-d{d}-k{k}', q, x, k, len(q)


def test_references_agree_with_the_oracle():
    rng = np.random.default_rng(0)
    for n, nq, d, k in ((50, 7, 64, 20), (300, 9, 128, 32), (5, 3, 64, 20)):
        x, q = rng.normal(size=(n, d)).astype(np.float32), rng.normal(size=(nq, d)).astype(np.float32)
        Dw, Iw = S.flat_l2_search(q, x, k)
        D, I, B = sr.topk_f64(q, x, k)
        kk = min(k, n)
        assert np.array_equal(I[:, :kk], Iw) and np.abs(D[:, :kk] - Dw).max() < 1e-12
        assert (I[:, kk:] == -1).all() and np.isposinf(D[:, kk:]).all() and (B[:, :kk] > 0).all()
        xi, qi = rng.integers(-2, 3, size=(n, d)).astype(np.float32), rng.integers(-2, 3, size=(nq, d)).astype(np.float32)
        Dw, Iw = S.flat_l2_search(qi, xi, k)                      # integers: float64 is exact too, and ties are frequent
        De, Ie = sr.topk_exact(qi, xi, k)
        assert np.array_equal(Ie[:, :kk], Iw) and np.array_equal(De[:, :kk], Dw.astype(np.float32))
        assert (Ie[:, kk:] == -1).all() and np.isposinf(De[:, kk:]).all()
        sr.check(De, Ie, qi, xi, k)                                # the float comparison accepts the exact result
        sr.check(D.astype(np.float32), I, q, x, k)                 # and the float64 result rounded once


def test_plan_restatement_covers_one_two_ragged_and_capped_splits():
    assert sr.plan_splits(129, 960, 20) == (1, 15) and sr.plan_splits(129, 961, 20) == (2, 8)
    assert sr.plan_splits(129, 1025, 20) == (2, 9)                # 9 + 8 tiles, the last of one row
    assert sr.plan_splits(40, sr.LARGE[0].n, 20) == (sr.split_cap(20), 8) == (102, 8)
    assert sr.plan_splits(40, sr.LARGE[1].n, 32) == (sr.split_cap(32), 8) == (64, 8)
    assert sr.plan_splits(sr.LARGE_NQ_MANY, sr.LARGE[0].n, 20)[0] < 102
    assert sr.plan_splits(5, sr.PLACED_N, 20) == (3, 9)           # the split boundary placed_positions assumes: row 576


def test_geometry_lists_every_value_at_every_dimension():
    for d in sr.DIMS:
        cs = [c for c in sr.GEOMETRY if c.d == d]
        assert {c.n for c in cs} == set(sr.N_INDEX) and {c.nq for c in cs} == set(sr.N_QUERY)
        assert {c.k for c in cs} == set(sr.KS) and {c.amax for c in cs} == {1, 2}


def test_exactness_premise_and_tie_shares():
    """Every magnitude of every exact set is below 2^24 (float32 holds it without rounding), and where a share means something
    (at least 127 queries, more than 2 k index rows) at least a quarter of the queries have a tie straddling the k-th place."""
    n_rich = 0
    for name, q, x, k, _ in _exact_sets():
        m = sr.exactness_margin(q, x)
        assert max(m.values()) < 2 ** 24 // 1024, (name, m)        # in fact below 2^14
        assert np.abs(x).max() <= 2 and np.abs(q).max() <= 3
        if len(q) >= 127 and len(x) > 2 * k:
            straddle, inside = sr.tie_shares(q, x, k)
            assert straddle >= 0.25, (name, straddle)
            assert k == 1 or inside >= 0.9, (name, inside)
            n_rich += 1
    assert n_rich >= 30


def test_every_mutant_fails_the_exact_comparison_where_it_applies():
    killed = {m: 0 for m in EXACT_MUTANTS}
    all_apply = set()
    for name, q, x, k, nq_launch in _exact_sets():
        want = sr.topk_exact(q, x, k, nq_launch=nq_launch)
        assert _same_bytes(want, sr.topk_exact(q, x, k)), name
        straddle, inside = (s > 0 for s in sr.tie_shares(q, x, k))
        n_app = 0
        for m in EXACT_MUTANTS:
            if not sr.applies(m, len(x), nq_launch, k, want[1], straddle, inside):
                continue
            assert not _same_bytes(sr.topk_exact(q, x, k, mutate=m, nq_launch=nq_launch), want), (name, m)
            killed[m] += 1
            n_app += 1
        if n_app == len(EXACT_MUTANTS):
            all_apply.add(name)
    assert min(killed.values()) >= 12, killed
    # every mutant at once: on geometry cases of every dimension, both large indexes and the IVF sets with k > 20
    assert {d for c in sr.GEOMETRY if c.name in all_apply for d in [c.d]} == set(sr.DIMS), all_apply
    assert 'large-k32' in all_apply and 'ivf-d128-k21' in all_apply and 'prefix' in all_apply, all_apply


def test_placed_duplicates_expect_the_smallest_positions_at_distance_zero():
    for d in sr.DIMS:
        for k in (20, 32):
            for sc in sr.PLACED_SCENARIOS:
                q, x, pos = sr.placed_set(d, k, sc)
                assert len(pos) > k and np.array_equal(pos, np.sort(pos))
                D, I = sr.topk_exact(q, x, k)
                for r in (0, 4):
                    assert np.array_equal(I[r], pos[:k]) and (D[r] == 0).all()
                for m in ('tie_larger_id', 'kth_keeps_later', 'halves_swapped'):
                    assert not np.array_equal(sr.topk_exact(q, x, k, mutate=m)[1][0], pos[:k]), (d, k, sc, m)
    pos = sr.placed_positions(20)
    assert all(p % 8 < 4 and p < 64 for p in pos['same_lane'])                        # one lane half, one tile
    assert {p // 32 for p in pos['blocks']} == {0, 1} and {p // 64 for p in pos['tiles']} == {0, 1}
    assert {p // 64 for p in pos['splits']} == {8, 9} and {p // 64 for p in pos['ragged_tile']} == {24}
    assert len({p // 64 for p in pos['scattered']}) >= 12


def test_every_mutant_fails_the_float_comparison_where_it_applies():
    killed = {m: 0 for m in sr.MUTANTS}
    for c in sr.FLOAT_CASES:
        q, x = sr.float_inputs(c)
        D, I, _ = sr.topk_f64(q, x, c.k)
        worst = sr.check(D.astype(np.float32), I, q, x, c.k)
        assert worst['dist'] < 0.05                                # one rounding against a bound of hundreds of u
        if c.kind == 'self':
            hit = (I == np.asarray([np.nonzero((x == q[r]).all(1))[0][0] for r in range(len(q))])[:, None]).any(1)
            assert hit.all() and (D[:, 0] == 0).all()
        for m in sr.MUTANTS:
            if m in ('tie_larger_id', 'kth_keeps_later'):
                continue                                           # float sets have no exact ties
            if not sr.applies(m, c.n, c.nq, c.k, I, False, False, self_queries=c.kind == 'self'):
                continue
            Dm, Im, _ = sr.topk_f64(q, x, c.k, mutate=m)
            with pytest.raises(AssertionError):
                sr.check(Dm.astype(np.float32), Im, q, x, c.k)
            killed[m] += 1
    for m in ('halves_swapped', 'split_last_tile_dropped', 'ragged_last_row_dropped', 'clamp_missing', 'k20_truncated'):
        assert killed[m] >= 2, killed


def test_norms_set_orders_by_distance_not_inner_product():
    for c in sr.FLOAT_CASES:
        if c.kind == 'norms':
            q, x = sr.float_inputs(c)
            n = np.linalg.norm(x.astype(np.float64), axis=1)
            assert n.min() < 0.3 and n.max() > 3.5
            _, I, _ = sr.topk_f64(q, x, c.k)
            ip = np.argmax(q.astype(np.float64) @ x.astype(np.float64).T, axis=1)
            assert (ip != I[:, 0]).mean() > 0.5


def test_bound_is_a_few_hundred_units_for_unit_vectors():
    q, x = sr.unit_rows(4, 128, 2), sr.unit_rows(9, 128, 1)
    b = sr.dist_bound(q, x)
    assert 300 * sr.U < b.min() and b.max() < 700 * sr.U
