"""CPU: the integer references, input sets, restated plan and mutants of the IVF edge tests (tests/_ivf_exact_ref.py) hold what
the GPU tests (tests/test_gpu_ivf_edges.py) rely on: the exactness premise, the plan restatement against the library's own
workspace queries, each case in the regime its name claims (from the reference and the restated plan, never from GPU output),
agreement with the float64 restatements, and every mutant failing the GPU tests' own comparison wherever it applies.
Run with -s for the case table."""
import numpy as np
import pytest

import _ivf_exact_ref as X
import _ivf_ref as R
import _ivf_rr_ref as RR


def _sample(nq):
    """The query rows a mutant is evaluated on (the partial lists are simulated per query in Python)."""
    return np.arange(nq) if nq <= 9 else np.unique([0, 1, 2, nq // 2, nq - 1])


def _runs(case):
    return [(nq, npb, k, False) for nq, npb, k in case.narrow] + [(nq, npb, k, True) for nq, npb, k in case.wide]


def _mutant(case, run, m, sample):
    nq, npb, k, wide = run
    return X.adc_topk_exact(case.f('q')[:nq][sample], case.f('cent'), case.f('pq'), case.codes, case.lists, case.probes(nq, npb)[sample],
                            k, case.s, mutate=None if m == 'simulate' else m, nq_launch=nq, wide=wide, labels=case.labels if wide else None, simulate=m == 'simulate')


def test_exactness_margin_holds_for_every_case():
    for case in X.search_cases() + [X.rerank(d) for d in X.DIMS]:
        m = X.exactness_margin(case)
        print(f'{case.name}: scale 2^{case.s}, d {case.d}, margins {m}')
        assert m['entry'] <= X.ENTRY_MAX and m['row'] < 2 ** 24 and m['rerank'] < 2 ** 24 and m['f16_exact'], (case.name, m)
        assert case.s in (0, -3, -10) and np.abs(case.f('q')).max() * 2.0 ** -case.s <= 16
    assert {c.d for c in X.search_cases()} == set(X.DIMS)
    assert {(c.name.split('-')[0], c.s) for c in X.search_cases() if c.s} == {('few_values', -3), ('few_values', -10), ('spread', -3),
                                                                             ('spread', -10)}
    # the scaled entries really reach the binary16 subnormals (below 2^-14) and stay multiples of 2^-24
    T, _ = X.adc_tables_exact(X.few_values(128, -10).f('q')[:4], X.few_values(128, -10).f('cent'), X.few_values(128, -10).f('pq'),
                              np.arange(4), np.arange(4), -10)
    assert ((T > 0) & (T < 2.0 ** -14)).mean() > 0.5 and np.array_equal(T.astype(np.float16).astype(np.float32), T)
    for d in X.DIMS:                                              # the encoders: integer residuals, sums far below 2^24
        c = X.encode_ties(d)
        assert np.abs(c.x - c.cent[c.lists]).max() <= 3 and np.abs(c.pq).max() == 2 and np.abs(c.refine).max() == 2


def test_plan_restatement_equals_the_librarys_workspace_queries(nafp):
    lib = nafp._lib.load()
    seen = set()
    for case in X.search_cases():
        for nq, npb, k, wide in _runs(case):
            total, parts = X.workspace_total(nq, case.nlist, npb, k, wide=wide)
            got = lib.nafp_ivf_pq_wide_workspace_bytes(nq, case.nlist, npb, k) if wide else lib.nafp_ivf_search_workspace_bytes(nq, case.nlist, npb, k, 1)
            assert got == total, (case.name, nq, npb, k, wide, got, total)
            seen.add(parts)
    for case, npb, k in X.flat_cases():
        assert lib.nafp_ivf_search_workspace_bytes(len(case.q), case.nlist, npb, k, 0) == X.workspace_total(len(case.q), case.nlist, npb, k, kind=0)[0]
    for nq in X.BATCH_NQ:
        for k, wide in ((20, False), (32, False), (100, True)):
            fn = lib.nafp_ivf_pq_wide_workspace_bytes if wide else (lambda a, b, c, d: lib.nafp_ivf_search_workspace_bytes(a, b, c, d, 1))
            assert fn(nq, 8, 3, k) == X.workspace_total(nq, 8, 3, k, wide=wide)[0]
    assert {1, 128, 819} <= seen and len(seen) >= 8, seen
    assert lib.nafp_last_hip_error() == 0                         # host-only computations
    # the formulas the issue states
    assert X.ivf_parts(1, 1, 20) == 819 and X.ivf_parts(1, 1, 128) == 128 and X.ivf_parts(2048, 1, 20) == 1
    assert X.part_rows(785, 128, 0) == (0, 7) and X.part_rows(785, 128, 112) == (784, 785) and X.part_rows(785, 128, 113) == (785, 785)
    assert len({X.ivf_parts(nq * 3, 3, 20) for nq in X.BATCH_NQ}) == 3


def test_each_case_is_in_the_regime_its_name_claims():
    c = X.all_tied()
    parts = X.ivf_parts(1, 1, 20)
    empty = [p for p in range(parts) if X.part_rows(c.n, parts, p)[0] == X.part_rows(c.n, parts, p)[1]]
    assert parts == 819 > c.n == 785 and len(empty) == 34 and c.n == 3 * 256 + 17
    for nq, npb, k, wide in _runs(c):
        D, I = c.ref(nq, npb, k, wide)
        assert (I == np.arange(k)).all() and (D == D[:, :1]).all()
    # few_values: a handful of distinct distances among 1 003 rows, ids interleaved across the lists
    for d in X.DIMS:
        c = X.few_values(d)
        dist = X.sq_distances(c.q, c.recon())
        n_val = max(len(np.unique(r)) for r in dist[0::2])
        print(f'{c.name}: at most {n_val} distinct distances per even query, {max(len(np.unique(r)) for r in dist)} per odd one, over {c.n} rows')
        assert n_val <= 8 and (c.lists[:16] == np.arange(16) % 8).all()
        for nq, npb, k, wide in _runs(c):
            assert X.applies('tie_larger_id', c, nq, npb, k, wide) and X.applies('kth_keeps_later', c, nq, npb, k, wide)
    # kth_tie: the k-th place inside a level of 12 that straddles a part boundary and both lists
    c = X.kth_tie()
    dist = X.sq_distances(c.q[:1], c.recon())[0]
    for nq, npb, k, wide in _runs(c):
        D, I = c.ref(nq, npb, k, wide)
        parts = X.ivf_parts(nq * 2, 2, X.template_k(k, wide))
        block = np.nonzero(dist == int(D[0, -1]))[0]
        per = -(-np.bincount(c.lists)[c.lists[block]] // parts)
        part = (block // 2) // per                                # lists are i % 2: a row's position in its list is i // 2
        assert len(block) == X.KTH_T and k % X.KTH_T and set(c.lists[block]) == {0, 1}
        assert parts == 1 or len(set(zip(c.lists[block], part))) >= 3, (nq, k, parts)
        assert np.array_equal(np.sort(I[0][D[0] == D[0, -1]]), block[:(D[0] == D[0, -1]).sum()])
        assert X.applies('kth_keeps_later', c, nq, npb, k, wide)
    assert {X.ivf_parts(nq * 2, 2, 20) for nq in (5, 131)} == {205, 8}
    # wide_prune: one part, every wave prunes, rows in and out of the result tie the k1-th distance
    for order in ('late', 'shuffled', 'relabelled'):
        c = X.wide_prune(order)
        for k1 in X.WIDE_PRUNE_K1:
            assert X.workspace_total(2048, 1, 1, k1, wide=True)[1] == 1
            prunes = X.simulated_prunes(c, k1)
            print(f'{c.name} k1 {k1}: simulated prunes per wave {prunes}')
            assert min(prunes) >= 2, (order, k1, prunes)
            D, I = c.ref(2048, 1, k1, True)
            d0 = X.sq_distances(c.q[:1], c.recon())[0]
            assert 0 < (D[0] == D[0, -1]).sum() < (d0 == int(D[0, -1])).sum()      # kept and rejected rows at the k1-th distance
    c = X.wide_prune('relabelled')
    assert all(X.applies('wide_threshold_tie_rejected', c, 2048, 1, k1, True, sample=[0]) for k1 in (80, 128))
    assert not any(X.applies('wide_threshold_tie_rejected', X.wide_prune(o), 2048, 1, 128, True, sample=[0]) for o in ('late', 'shuffled'))
    # short_lists: padding in every run, a row of nothing but padding, the clamp
    c = X.short_lists(6)
    for nq, npb, k, wide in _runs(c):
        D, I = c.ref(nq, npb, k, wide)
        assert (I[:, -1] == -1).all() and np.isposinf(D[:, -1]).all()
        if npb <= 2:
            assert (I[1] == -1).all() and (I[3] == -1).all()
    assert np.bincount(c.lists, minlength=6).tolist() == [7, 0, 5, 0, 11, 0]
    c = X.short_lists(1)
    assert c.probes(4, 5).shape == (4, 1) and (np.sort(c.ref(4, 5, 20)[1][:, :9], axis=1) == np.arange(9)).all() and (c.ref(4, 5, 20)[1][:, 9:] == -1).all()
    # zero_distance: +0.0 at the first places, a row and its copy
    c = X.zero_distance()
    D, I = c.ref(20, 4, 20)
    assert (D[:, :2].view(np.uint32) == 0).all() and (I[:, 0] == np.arange(20)).all() and (I[:, 1] == 300 + np.arange(20)).all()
    # spread: few ties
    for c in (X.spread(128), X.spread(256)):
        D, _ = c.ref(131, 8, 32)
        assert (np.diff(D, axis=1) == 0).mean() < 0.2
    # probe_ties: the cut inside a tie group, duplicated centroids
    c = X.probe_ties()
    assert (X.sq_distances(c.q[:1], c.cent)[0][:8] == 1).all() and (c.cent[8:] == c.cent[8]).all()
    assert c.probes(21, 5)[0].tolist() == [0, 1, 2, 3, 4] and c.probes(21, 5)[1, :4].tolist() == [8, 9, 10, 11]
    assert all(X.probe_applies(c, 21, npb) for npb in X.PROBE_TIES_NPROBE)


def test_references_agree_with_the_float64_restatements():
    """Integers times a power of two are exact in float64 too, so the restatements must give the same distances, and the same
    ids up to ties (checked through the integer distances).  Every run of every case; all query rows of a run of up to 131
    queries, five sampled rows of the 2 048-query runs (the restatement loops over queries in Python)."""
    for case in X.search_cases():
        q, cent, pq = case.f('q'), case.f('cent'), case.f('pq')
        dist = X.sq_distances(case.q, case.recon())
        for nq, npb, k, wide in _runs(case):
            rows = np.arange(nq) if nq <= 131 else _sample(nq)
            P = case.probes(nq, npb)
            Pw, _ = R.probe(q[:nq][rows], cent, npb)
            assert np.array_equal(Pw, P[rows]), case.name
            if wide and case.labels is not None:
                continue                                          # the restatement knows rows by index only
            D, I = (a[rows] for a in case.ref(nq, npb, k, wide))
            Dw, Iw = R.adc_search(q[:nq][rows], cent, pq, case.codes, case.lists, P[rows], k)
            assert np.array_equal(Dw.astype(np.float32), D), (case.name, nq, npb, k)
            differ = np.argwhere(I != Iw)
            assert all(dist[rows[r], I[r, c]] == dist[rows[r], Iw[r, c]] for r, c in differ), case.name
            assert np.array_equal(I, Iw)                          # in fact the very ids: both order by (distance, id)
    for d in X.DIMS:
        c = X.rerank(d)
        for k1, k in X.RERANK_RUNS:
            cand = np.where(c.cand[:, :k1] < c.n, c.cand[:, :k1], -1)
            D, I = X.rerank_exact(c.f('q'), c.cand[:, :k1], c.f('cent'), c.f('pq'), c.f('refine'), c.codes, c.rcodes, c.lists, c.n, k)
            Dw, Iw = RR.rerank(c.f('q'), cand, c.f('cent'), c.f('pq'), c.f('refine'), c.codes, c.rcodes, c.lists, k)
            assert np.array_equal(Dw.astype(np.float32), D) and np.array_equal(I, Iw), (d, k1, k)
        e = X.encode_ties(d)
        res = e.x - e.cent[e.lists]
        assert np.array_equal(X.encode_exact(e.f('x'), e.f('pq'), e.lists, e.f('cent')), R.pq_encode(res, e.pq))
        assert np.array_equal(X.encode_exact(res.astype(np.float32), e.f('pq')), R.pq_encode(res, e.pq))
        assert np.array_equal(X.refine_encode_exact(e.f('x'), e.f('refine'), False), RR.refine_encode(e.x, e.refine))
        assert np.array_equal(X.refine_encode_exact(e.f('x'), e.f('refine'), True), RR.pack_codes(RR.refine_encode(e.x, e.refine)))
    for case, npb, k in X.flat_cases():
        P = case.probes(len(case.q), npb)
        x = case.recon().astype(np.float32)
        D, I = X.flat_topk_exact(case.f('q'), x, case.lists, P, k)
        Dw, Iw = R.ivf_flat_search(case.f('q'), x, case.lists, P, k)
        assert np.array_equal(Dw.astype(np.float32), D) and np.array_equal(I, Iw), case.name


def test_the_partial_list_simulation_is_the_plain_reference():
    """Going through parts, K-entry partial lists, the wave filter and the merge without a mutant gives the reference's bytes: the
    simulation the part, merge and threshold mutants live in is itself right."""
    for case in (X.all_tied(), X.few_values(64), X.kth_tie(), X.wide_prune('relabelled'), X.wide_prune('late'), X.short_lists(6)):
        for run in _runs(case):
            rows = _sample(run[0])[:3]
            want = tuple(a[rows] for a in case.ref(*run))
            assert X.same(_mutant(case, run, 'simulate', rows), want), (case.name, run)


def test_every_mutant_fails_the_comparison_where_it_applies():
    killed = {m: set() for m in X.MUTANTS}
    for case in X.search_cases():
        for run in _runs(case):
            nq, npb, k, wide = run
            rows = _sample(nq)
            want = tuple(a[rows] for a in case.ref(*run))
            applying = []
            for m in X.SEARCH_MUTANTS:
                if X.applies(m, case, nq, npb, k, wide, sample=rows):
                    assert not X.same(_mutant(case, run, m, rows), want), (case.name, run, m)
                    killed[m].add(case.name)
                    applying.append(m)
                elif m in ('tie_larger_id', 'kth_keeps_later', 'padding_unwritten', 'zero_distance_negative', 'partial_padding_stale'):
                    assert X.same(_mutant(case, run, m, rows), want), (case.name, run, m)      # the predicate is sharp
            parts = X.workspace_total(nq, case.nlist, npb, k, wide=wide)[1]
            print(f'{case.name}: scale 2^{case.s} d {case.d} {"wide" if wide else "narrow"} nq {nq} nprobe {npb} k {k}: parts {parts}, '
                  f'K {X.template_k(k, wide)}; applies: {applying}')
        for nq, npb in sorted({(r[0], r[1]) for r in _runs(case)}):
            if X.probe_applies(case, nq, npb):
                assert not X.same(X.probe_exact(case.f('q')[:nq], case.f('cent'), npb, case.s, mutate='probe_tie_larger_list'), case.probes(nq, npb))
                killed['probe_tie_larger_list'].add(case.name)
    for d in X.DIMS:
        c = X.rerank(d)
        args = (c.f('cent'), c.f('pq'), c.f('refine'), c.codes, c.rcodes, c.lists, c.n)
        for k1, k in X.RERANK_RUNS:
            want = X.rerank_exact(c.f('q'), c.cand[:, :k1], *args, k)
            for m in X.RERANK_MUTANTS:
                differs = not X.same(X.rerank_exact(c.f('q'), c.cand[:, :k1], *args, k, mutate=m), want)
                assert differs == X.rerank_applies(m, c, k1, k), (c.name, k1, k, m)
                if differs:
                    killed[m].add(c.name)
        e = X.encode_ties(d)
        res = e.x - e.cent[e.lists]
        assert X.encode_applies(res, e.pq) and X.encode_applies(e.x, e.refine)
        assert not X.same(X.encode_exact(e.f('x'), e.f('pq'), e.lists, e.f('cent'), mutate='encode_tie_larger_code'),
                          X.encode_exact(e.f('x'), e.f('pq'), e.lists, e.f('cent')))
        for packed in (False, True):
            assert not X.same(X.refine_encode_exact(e.f('x'), e.f('refine'), packed, mutate='encode_tie_larger_code'),
                              X.refine_encode_exact(e.f('x'), e.f('refine'), packed))
        killed['encode_tie_larger_code'].add(e.name)
    print({m: sorted(v) for m, v in killed.items()})
    assert all(killed[m] for m in X.MUTANTS), {m: len(v) for m, v in killed.items()}
    # where each mutant must show: the cases built for it
    assert {'all_tied', 'kth_tie', 'few_values-d64', 'few_values-d128-s-10', 'wide_prune-late'} <= killed['kth_keeps_later']
    assert {'few_values-d64', 'few_values-d256', 'kth_tie'} <= killed['merge_ties_by_probe_order']
    assert {'all_tied', 'kth_tie', 'few_values-d128'} <= killed['part_last_row_dropped']
    assert killed['wide_threshold_tie_rejected'] == {'wide_prune-relabelled'}
    assert {'short_lists-nlist6', 'short_lists-nlist1', 'rerank-d256'} <= killed['padding_unwritten']
    assert {'zero_distance', 'rerank-d64'} <= killed['zero_distance_negative']
    assert {'all_tied', 'wide_prune-late', 'wide_prune-shuffled'} <= killed['k20_truncated']
    assert {'probe_ties', 'few_values-d64', 'kth_tie'} <= killed['probe_tie_larger_list']
    assert {'all_tied', 'short_lists-nlist6', 'short_lists-nlist1', 'kth_tie'} <= killed['partial_padding_stale']
