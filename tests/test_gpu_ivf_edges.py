"""GPU: the selection code of the approximate indexes (csrc/ivf.hip: the three IVF-PQ scans, ivf_merge_kernel,
ivf_pqr_rerank_kernel, ivf_probe_kernel, the arg-mins of the two encoders; nafp_ivf_flat_search with nprobe < nlist) at its
ties, padding and part splits.

Every input is integers times a power of two (tests/_ivf_exact_ref.py): float32 -- and binary16 for the table entries --
computes every quantity without rounding, so each result is determined bit for bit and is compared with the int64 reference
ordered by (distance, id) through `X.same`: equal shapes, types and BYTES, +0.0 for a zero distance included.  Nothing is
excused.  tests/test_ivf_exact_ref_host.py shows on the CPU that each case is in the regime its name claims and that a flipped
tie-break, a `>=` at the k-th place, a part one row short, a merge by probe order, a threshold tie on the wrong side,
unwritten padding (in the output or in a part's K partial slots), -0.0 and k > 20 from 20-entry lists each fail this comparison.

The C entry points are called directly.  The lists are built with nafp_ivf_bucket and nafp_ivf_pq_lists (nafp_ivf_flat_lists);
outputs sit between guard bytes and are pre-filled with a sentinel.  Every search runs twice: with the workspace full of 0xFF
bytes (partial ids -1, keys NaN), and with ATTRACTIVE stale partial lists where the call lays its own out -- keys of +1e30 with
the valid id 0, which would win every merge -- so a part that leaves some of its K padding slots unwritten (an empty part, a
short list) shows; both runs must give the reference's bytes.  One exception to "as the
building blocks leave them": the `relabelled` order of wide_prune hands the wide search an ids array whose labels do not ascend
along the list -- the wide scan and the merge select by the packed (key, id) alone, and only so can a row tie the prune threshold
with the SMALLER id."""
import numpy as np
import pytest
import torch

import _ivf_exact_ref as X
from test_gpu_search_edges import Guarded, _dev, _lib

pytestmark = pytest.mark.gpu

F32, F16 = 0, 1
_LISTS = {}


def _out(nq, k):
    """Guarded, sentinel-filled (distances, ids) of a search."""
    D, I = Guarded(nq * k * 4), Guarded(nq * k * 4)
    D.t.view(torch.int32).fill_(int(X.SENT_D.view(np.int32)))
    I.t.view(torch.int32).fill_(int(X.SENT_I))
    return D, I


def _read(G, nq, k, dtype=torch.float32):
    assert G.intact(), 'a guard was written'
    return G.t.view(dtype).reshape(nq, k).cpu().numpy()


def _workspace(need, stale=None):
    """`need` guarded bytes of 0xFF; stale = X.partial_lists_at(..): attractive partial lists (+1e30, id 0) on top."""
    assert need > 0
    ws = Guarded(need, fill=0xFF)
    if stale is not None:
        o_pk, o_pi, m = stale
        assert o_pk + 4 * m <= o_pi and o_pi + 4 * m <= need
        ws.t[o_pk:o_pk + 4 * m].view(torch.float32).fill_(X.STALE_KEY)
        ws.t[o_pi:o_pi + 4 * m].view(torch.int32).fill_(0)
    return ws


def _both(what, run):
    """run(stale) for the two workspace fills; the results must be the same bytes."""
    a, b = run(False), run(True)
    assert X.same(a, b), f'{what}: the result depends on what the workspace held'
    return a


def _bucket(keys_t, n, nb):
    L, lib = _lib()
    offsets = torch.empty(nb + 1, dtype=torch.int32, device='cuda')
    ids = torch.full((max(n, 1),), -1, dtype=torch.int32, device='cuda')
    need = int(lib.nafp_ivf_bucket_workspace_bytes(n, nb, 1))
    ws = _workspace(need)
    L.check(lib.nafp_ivf_bucket(L.ptr(keys_t), 4, n, nb, 1, L.ptr(offsets), L.ptr(ids), L.ptr(ws.t), need, L.current_stream()), 'ivf_bucket')
    torch.cuda.synchronize()
    assert ws.intact()
    return offsets, ids


class Lists:
    """The device side of a case: parameters, codes in insertion order, and the inverted lists from the building blocks."""

    def __init__(self, case):
        L, lib = _lib()
        self.case = case
        self.cent, self.pq, self.refine = _dev(case.f('cent')), _dev(case.f('pq')), _dev(case.f('refine'))
        self.codes, self.rcodes, self.assign = _dev(case.codes), _dev(case.rcodes), _dev(case.lists)
        self.offsets, self.ids = _bucket(self.assign, case.n, case.nlist)
        self.sorted = torch.empty((case.n, X.M), dtype=torch.uint8, device='cuda')
        L.check(lib.nafp_ivf_pq_lists(L.ptr(self.codes), case.n, X.M, L.ptr(self.ids), L.ptr(self.sorted), L.current_stream()), 'ivf_pq_lists')
        torch.cuda.synchronize()
        order = np.lexsort((np.arange(case.n), case.lists))       # ascending ids inside each list
        assert np.array_equal(self.ids.cpu().numpy(), order) and np.array_equal(self.sorted.cpu().numpy(), case.codes[order])
        assert np.array_equal(self.offsets.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(case.lists, minlength=case.nlist))]))
        self.labels = None if case.labels is None else _dev(case.labels[order].astype(np.int32))


def _lists(case):
    if case.name not in _LISTS:
        _LISTS.clear()                                            # one at a time
        _LISTS[case.name] = Lists(case)
    return _LISTS[case.name]


def _search(S, q_t, nprobe, k, entry, lut=F32):
    """One call of nafp_ivf_pq_search ('plain'), _ex ('ex') or _wide ('wide') -> (D float32, I int32) numpy."""
    L, lib = _lib()
    c = S.case
    nq = int(q_t.shape[0])
    wide = entry == 'wide'
    ids = S.labels if wide and S.labels is not None else S.ids
    need = int(lib.nafp_ivf_pq_wide_workspace_bytes(nq, c.nlist, nprobe, k) if wide else lib.nafp_ivf_search_workspace_bytes(nq, c.nlist, nprobe, k, 1))
    return _both(f'{c.name} {entry}', lambda stale: _search_once(S, q_t, nprobe, k, entry, lut, ids, need, stale))


def _search_once(S, q_t, nprobe, k, entry, lut, ids, need, stale):
    L, lib = _lib()
    c = S.case
    nq = int(q_t.shape[0])
    ws = _workspace(need, X.partial_lists_at(nq, c.nlist, nprobe, k, wide=entry == 'wide') if stale else None)
    D, I = _out(nq, k)
    head = (L.ptr(q_t), nq, L.ptr(S.cent), c.nlist, c.d, nprobe, L.ptr(S.pq), X.M, L.ptr(S.sorted), L.ptr(S.offsets), L.ptr(ids), k,
            L.ptr(D.t), L.ptr(I.t))
    tail = (L.ptr(ws.t), need, L.current_stream())
    if entry == 'plain':
        L.check(lib.nafp_ivf_pq_search(*head, *tail), 'ivf_pq_search')
    elif entry == 'ex':
        L.check(lib.nafp_ivf_pq_search_ex(*head, lut, *tail), 'ivf_pq_search_ex')
    else:
        L.check(lib.nafp_ivf_pq_search_wide(*head, lut, *tail), 'ivf_pq_search_wide')
    torch.cuda.synchronize()
    assert ws.intact(), 'a workspace guard was written'
    return _read(D, nq, k), _read(I, nq, k, torch.int32)


def _assert_same(got, want, what):
    if not X.same(got, want):
        bad = np.nonzero((got[1] != want[1]).any(1) | (got[0].view(np.uint32) != want[0].view(np.uint32)).any(1))[0]
        r = bad[0]
        raise AssertionError(f'{what}: {len(bad)} query rows differ; row {r}: ids {got[1][r].tolist()} / want {want[1][r].tolist()}, '
                             f'dist {got[0][r].tolist()} / want {want[0][r].tolist()}')


CASES = X.search_cases()


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_pq_searches_give_the_reference_bytes(nafp, case):
    """nafp_ivf_pq_search, nafp_ivf_pq_search_ex and nafp_ivf_pq_search_wide, both table precisions: f16 = f32 = the reference,
    and the wide search at k1 <= 32 = the narrow one."""
    S = _lists(case)
    q = _dev(case.f('q'))
    for nq, nprobe, k in case.narrow:
        want = case.ref(nq, nprobe, k)
        what = f'{case.name} nq {nq} nprobe {nprobe} k {k}'
        _assert_same(_search(S, q[:nq], nprobe, k, 'plain'), want, what + ' pq_search')
        _assert_same(_search(S, q[:nq], nprobe, k, 'ex', F32), want, what + ' ex f32')
        _assert_same(_search(S, q[:nq], nprobe, k, 'ex', F16), want, what + ' ex f16')
        _assert_same(_search(S, q[:nq], nprobe, k, 'wide', F32), want, what + ' wide f32 at a narrow k')
        _assert_same(_search(S, q[:nq], nprobe, k, 'wide', F16), want, what + ' wide f16 at a narrow k')
    for nq, nprobe, k1 in case.wide:
        want = case.ref(nq, nprobe, k1, True)
        for lut in (F32, F16):
            _assert_same(_search(S, q[:nq], nprobe, k1, 'wide', lut), want, f'{case.name} nq {nq} nprobe {nprobe} k1 {k1} wide lut {lut}')


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_adc_tables_export_exactly_the_references_entries(nafp, case):
    L, lib = _lib()
    S = _lists(case)
    nq = min(len(case.q), 16)
    pair_q = np.repeat(np.arange(nq), case.nlist).astype(np.int32)
    pair_l = np.tile(np.arange(case.nlist), nq).astype(np.int32)
    want, _ = X.adc_tables_exact(case.f('q'), case.f('cent'), case.f('pq'), pair_q, pair_l, case.s)
    q, pq_t, pl_t = _dev(case.f('q')[:nq]), _dev(pair_q), _dev(pair_l)
    for lut, dtype, np_t in ((F32, torch.float32, np.float32), (F16, torch.float16, np.float16)):
        out = Guarded(len(pair_q) * X.M * X.KS * (4 if lut == F32 else 2), fill=0xFF)
        L.check(lib.nafp_ivf_pq_adc_tables(L.ptr(q), nq, L.ptr(pq_t), L.ptr(pl_t), len(pair_q), L.ptr(S.cent), case.nlist, case.d, L.ptr(S.pq),
                                           X.M, lut, L.ptr(out.t), L.current_stream()), 'ivf_pq_adc_tables')
        torch.cuda.synchronize()
        got = _read(out, len(pair_q), X.M * X.KS, dtype).reshape(want.shape)
        assert got.astype(np.float32).tobytes() == want.tobytes() and got.tobytes() == want.astype(np_t).tobytes(), (case.name, lut)


PQR = [c for c in CASES if c.labels is None]


@pytest.mark.parametrize('case', PQR, ids=lambda c: c.name)
def test_pqr_search_stages(nafp, case):
    """nafp_ivf_pqr_search: stage 1 is the wide search's reference, the final output rerank_exact of the REFERENCE's stage-1 ids."""
    L, lib = _lib()
    S = _lists(case)
    nq, nprobe = min(len(case.q), 131), case.wide[0][1]
    q = _dev(case.f('q')[:nq])
    for k, kf in ((20, 4), (32, 4), (5, 1), (21, 3)):
        k1 = k * kf
        want1 = case.ref(nq, nprobe, k1, True)
        want = X.rerank_exact(case.f('q')[:nq], want1[1], case.f('cent'), case.f('pq'), case.f('refine'), case.codes, case.rcodes, case.lists,
                              case.n, k, case.s)
        for lut, stale in ((F32, False), (F32, True), (F16, False), (F16, True)):
            need = int(lib.nafp_ivf_pq_wide_workspace_bytes(nq, case.nlist, nprobe, k1))
            ws = _workspace(need, X.partial_lists_at(nq, case.nlist, nprobe, k1, wide=True) if stale else None)
            D, I = _out(nq, k)
            D1, I1 = _out(nq, k1)
            L.check(lib.nafp_ivf_pqr_search(L.ptr(q), nq, L.ptr(S.cent), case.nlist, case.d, nprobe, L.ptr(S.pq), X.M, L.ptr(S.sorted),
                                            L.ptr(S.offsets), L.ptr(S.ids), L.ptr(S.assign), L.ptr(S.codes), L.ptr(S.refine), X.RF_M, 4,
                                            L.ptr(S.rcodes), case.n, k, kf, L.ptr(D.t), L.ptr(I.t), L.ptr(D1.t), L.ptr(I1.t), lut, L.ptr(ws.t), need,
                                            L.current_stream()), 'ivf_pqr_search')
            torch.cuda.synchronize()
            assert ws.intact()
            what = f'{case.name} nq {nq} nprobe {nprobe} k {k} x {kf} lut {lut} stale {stale}'
            _assert_same((_read(D1, nq, k1), _read(I1, nq, k1, torch.int32)), want1, what + ' stage 1')
            _assert_same((_read(D, nq, k), _read(I, nq, k, torch.int32)), want, what + ' re-ranked')


@pytest.mark.parametrize('d', X.DIMS)
def test_rerank_entry_point(nafp, d):
    """nafp_ivf_pqr_rerank on tied reconstructions, -1 holes, an all -1 row, ids >= n_rows, a candidate named twice, fewer valid
    candidates than k; k1 = 1, 100, 128, k = k1 and k < k1."""
    L, lib = _lib()
    c = X.rerank(d)
    S = _lists(c)
    q = _dev(c.f('q'))
    for k1, k in X.RERANK_RUNS:
        cand = np.ascontiguousarray(c.cand[:, :k1])
        want = X.rerank_exact(c.f('q'), cand, c.f('cent'), c.f('pq'), c.f('refine'), c.codes, c.rcodes, c.lists, c.n, k)
        D, I = _out(len(c.q), k)
        cd = _dev(cand)
        L.check(lib.nafp_ivf_pqr_rerank(L.ptr(q), len(c.q), d, L.ptr(cd), k1, L.ptr(S.cent), L.ptr(S.assign), L.ptr(S.pq), X.M, L.ptr(S.codes),
                                        L.ptr(S.refine), X.RF_M, 4, L.ptr(S.rcodes), c.n, k, L.ptr(D.t), L.ptr(I.t), L.current_stream()),
                'ivf_pqr_rerank')
        torch.cuda.synchronize()
        _assert_same((_read(D, len(c.q), k), _read(I, len(c.q), k, torch.int32)), want, f'{c.name} k1 {k1} k {k}')


def _probe(S, q_t, nprobe):
    L, lib = _lib()
    nq = int(q_t.shape[0])
    P = Guarded(nq * nprobe * 4)
    P.t.view(torch.int32).fill_(int(X.SENT_I))
    L.check(lib.nafp_ivf_probe(L.ptr(q_t), nq, L.ptr(S.cent), S.case.nlist, S.case.d, nprobe, L.ptr(P.t), L.current_stream()), 'ivf_probe')
    torch.cuda.synchronize()
    return _read(P, nq, nprobe, torch.int32)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_probe_orders_by_distance_then_list_id(nafp, case):
    S = _lists(case)
    q = _dev(case.f('q'))
    runs = {(nq, min(npb, case.nlist)) for nq, npb, _ in case.narrow + case.wide}
    if case.name == 'probe_ties':
        runs |= {(21, npb) for npb in X.PROBE_TIES_NPROBE}
    for nq, npb in sorted(runs):
        assert X.same(_probe(S, q[:nq], npb), case.probes(nq, npb)), (case.name, nq, npb)


@pytest.mark.parametrize('d', X.DIMS)
def test_encoders_take_the_smaller_code_on_equal_distance(nafp, d):
    """nafp_ivf_pq_encode with assign / coarse and on given residuals, nafp_ivf_refine_encode packed and unpacked; 257 rows."""
    L, lib = _lib()
    c = X.encode_ties(d)
    x, res = _dev(c.f('x')), _dev((c.x - c.cent[c.lists]).astype(np.float32))
    cent, pq, refine, assign = _dev(c.f('cent')), _dev(c.f('pq')), _dev(c.f('refine')), _dev(c.lists)
    want = X.encode_exact(c.f('x'), c.f('pq'), c.lists, c.f('cent'))
    for rows, a, co in ((x, assign, cent), (res, None, None)):
        out = Guarded(c.n * X.M)
        L.check(lib.nafp_ivf_pq_encode(L.ptr(rows), c.n, d, L.ptr(a), L.ptr(co), L.ptr(pq), X.M, L.ptr(out.t), L.current_stream()), 'ivf_pq_encode')
        torch.cuda.synchronize()
        assert X.same(_read(out, c.n, X.M, torch.uint8), want), (d, a is None)
    for packed in (0, 1):
        width = 2 if packed else 4
        out = Guarded(c.n * width)
        L.check(lib.nafp_ivf_refine_encode(L.ptr(x), c.n, d, L.ptr(refine), X.RF_M, 4, packed, L.ptr(out.t), L.current_stream()), 'ivf_refine_encode')
        torch.cuda.synchronize()
        assert X.same(_read(out, c.n, width, torch.uint8), X.refine_encode_exact(c.f('x'), c.f('refine'), bool(packed))), (d, packed)


@pytest.mark.parametrize('case,nprobe,k', X.flat_cases(), ids=lambda v: str(v))
def test_ivf_flat_with_fewer_probes_than_lists(nafp, case, nprobe, k):
    """nafp_ivf_flat_search with nprobe < nlist over the cases' reconstructed rows (integers)."""
    L, lib = _lib()
    x = case.recon().astype(np.float32)
    nq = len(case.q)
    want = X.flat_topk_exact(case.f('q'), x, case.lists, case.probes(nq, nprobe), k)
    xd, q, cent, assign = _dev(x), _dev(case.f('q')), _dev(case.f('cent')), _dev(case.lists)
    offsets, ids = _bucket(assign, case.n, case.nlist)
    bound = int(lib.nafp_ivf_flat_rows_bound(case.n, case.nlist))
    rows, hn, rid = Guarded(bound * case.d * 4, fill=0xFF), Guarded(bound * 4, fill=0xFF), Guarded(bound * 4, fill=0xFF)
    row_off = torch.empty(case.nlist + 1, dtype=torch.int32, device='cuda')
    L.check(lib.nafp_ivf_flat_lists(L.ptr(xd), case.n, case.d, L.ptr(offsets), L.ptr(ids), case.nlist, L.ptr(row_off), L.ptr(rows.t), L.ptr(hn.t),
                                    L.ptr(rid.t), L.current_stream()), 'ivf_flat_lists')
    need = int(lib.nafp_ivf_search_workspace_bytes(nq, case.nlist, nprobe, k, 0))
    for stale in (False, True):
        _flat_once(case, nprobe, k, q, cent, rows, hn, row_off, rid, need, stale, want)


def _flat_once(case, nprobe, k, q, cent, rows, hn, row_off, rid, need, stale, want):
    L, lib = _lib()
    nq = len(case.q)
    ws = _workspace(need, X.partial_lists_at(nq, case.nlist, nprobe, k, kind=0) if stale else None)
    D, I = _out(nq, k)
    L.check(lib.nafp_ivf_flat_search(L.ptr(q), nq, L.ptr(cent), case.nlist, case.d, nprobe, L.ptr(rows.t), L.ptr(hn.t), L.ptr(row_off), L.ptr(rid.t), k,
                                     L.ptr(D.t), L.ptr(I.t), L.ptr(ws.t), need, L.current_stream()), 'ivf_flat_search')
    torch.cuda.synchronize()
    assert rows.intact() and hn.intact() and rid.intact() and ws.intact()
    _assert_same((_read(D, nq, k), _read(I, nq, k, torch.int32)), want, f'{case.name} nprobe {nprobe} k {k} stale {stale}')


@pytest.mark.parametrize('case', [X.few_values(64), X.few_values(128, -10), X.kth_tie(), X.spread(256)], ids=lambda c: c.name)
def test_batching_independence_under_ties(nafp, case):
    """The same query rows searched alone (nq = 1), as 131 and inside 2 048: three different `parts`, identical bytes."""
    S = _lists(case)
    nprobe = min(3, case.nlist)
    q131 = case.f('q')[:131]
    big = _dev(q131[np.arange(2048) % 131])
    for k, entry, luts in ((20, 'ex', (F32, F16)), (21, 'ex', (F32, F16)), (100, 'wide', (F32, F16))):
        want = case.ref(131, nprobe, k, entry == 'wide')
        assert len({X.workspace_total(nq, case.nlist, nprobe, k, wide=entry == 'wide')[1] for nq in X.BATCH_NQ}) == 3
        for lut in luts:
            what = f'{case.name} nprobe {nprobe} k {k} {entry} lut {lut}'
            got = _search(S, big, nprobe, k, entry, lut)
            _assert_same(tuple(a[:131] for a in got), want, what + ' inside 2048')
            _assert_same(tuple(a[1965:2048] for a in got), tuple(a[:83] for a in want), what + ' inside 2048, the last rows')
            _assert_same(_search(S, big[:131], nprobe, k, entry, lut), want, what + ' as 131')
            for r in (0, 1, 130):
                _assert_same(_search(S, big[r:r + 1], nprobe, k, entry, lut), tuple(a[r:r + 1] for a in want), what + f' row {r} alone')
