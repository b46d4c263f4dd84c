"""GPU: nafp_search_topk_l2 (csrc/search.hip: search_topk_body + search_merge_kernel) and the same scan body under
nafp_ivf_flat_search, at their ties, boundaries and splits.

EXACT CASES.  Inputs with small integer entries (tests/_search_ref.py): float32 computes every key and distance without
rounding, so the result is determined bit for bit and is compared with np.array_equal on the ids and on the bytes of the
distances against the int64 (distance, id) order.  Nothing is excused.  tests/test_search_ref_host.py shows on the CPU that the
sets are rich in ties at the k-th place and that a flipped tie-break, a `>=` insertion, a wrong row mapping, a skipped tile or
row, or k > 20 served by the 20-entry lists each fail this comparison.

FLOAT CASES.  `_search_ref.check` with the a-priori bound derived there; the worst observed / bound ratio of every case is
recorded through `observe` with tolerance 1.

HARNESS (`Call`).  The C ABI directly; outputs and workspace sit between 4096 guard bytes.  Every search runs twice: with the
workspace full of NaN bytes and handed over 256-byte aligned, and with an attractive stale pattern (keys of +1e30 with the valid
id 0) handed over 8 bytes past a 256-byte boundary.  Both runs must give the same bytes and leave every guard intact.
"""
import numpy as np
import pytest
import torch

import _search_ref as sr

pytestmark = pytest.mark.gpu

GUARD = 4096
GUARD_BYTE = 0xA5
OK, UNSUPPORTED, WORKSPACE = 0, 2, 4


def _lib():
    from neural_audio_fp_amd import _lib as L
    return L, L.load()


class Guarded:
    """`nbytes` of device memory between two guards; `t` is the uint8 view of the payload, which starts `shift` bytes past a
    256-byte boundary."""

    def __init__(self, nbytes, shift=0, fill=GUARD_BYTE):
        self.raw = torch.full((GUARD + 256 + shift + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device='cuda')
        self.off = GUARD + (-(self.raw.data_ptr() + GUARD)) % 256 + shift
        self.n = nbytes
        self.t = self.raw[self.off:self.off + nbytes]
        assert (self.t.data_ptr() - shift) % 256 == 0
        self.t.fill_(fill)

    def intact(self):
        return bool((self.raw[:self.off] == GUARD_BYTE).all()) and bool((self.raw[self.off + self.n:] == GUARD_BYTE).all())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Index:
    """Device rows and their prepared aux array (guarded) for the first n_index rows of `x_all`."""

    def __init__(self, x_all, n_index=None):
        L, lib = _lib()
        self.x = x_all if torch.is_tensor(x_all) else _dev(x_all)
        self.n = int(self.x.shape[0] if n_index is None else n_index)
        self.d = int(self.x.shape[1])
        self.aux = Guarded(int(lib.nafp_search_index_aux_floats(self.n)) * 4, fill=0xFF)
        L.check(lib.nafp_search_index_prepare(L.ptr(self.x), self.n, self.d, L.ptr(self.aux.t), L.current_stream()), 'prepare')
        torch.cuda.synchronize()
        assert self.aux.intact()


def n_splits(nq, n, k):
    """The split count of a launch, from the public workspace query."""
    _, lib = _lib()
    K = sr.template_k(k)
    need = int(lib.nafp_search_workspace_bytes(nq, n, k))
    splits, rem = divmod(need - 256, nq * 2 * K * 8)
    assert need > 0 and rem == 0
    return splits


def _fill_attractive(ws, nq, splits, K):
    """Stale partial lists that would win every merge: keys +1e30, id 0, where the call lays its keys and ids out."""
    base = (-ws.t.data_ptr()) % 256
    m = nq * 2 * splits * K
    ws.t[base:base + 4 * m].view(torch.float32).fill_(1e30)
    ws.t[base + 4 * m:base + 8 * m].view(torch.int32).fill_(0)


def search_once(q_t, index, k, variant, ws=None):
    """One guarded call -> (D float32 (nq, k), I int32 (nq, k)) numpy.  variant 0: NaN workspace, aligned; 1: attractive, + 8."""
    L, lib = _lib()
    nq = int(q_t.shape[0])
    need = int(lib.nafp_search_workspace_bytes(nq, index.n, k))
    assert need > 0
    if ws is None:
        ws = Guarded(need, shift=8 if variant else 0, fill=0xFF)
        if variant:
            _fill_attractive(ws, nq, n_splits(nq, index.n, k), sr.template_k(k))
    D, I = Guarded(nq * k * 4), Guarded(nq * k * 4)
    L.check(lib.nafp_search_topk_l2(L.ptr(q_t), nq, L.ptr(index.x), L.ptr(index.aux.t), index.n, index.d, k, L.ptr(D.t), L.ptr(I.t),
                                    L.ptr(ws.t), need, L.current_stream()), 'search_topk_l2')
    torch.cuda.synchronize()
    assert D.intact() and I.intact() and ws.intact() and index.aux.intact(), 'a guard was written'
    return (D.t.view(torch.float32).reshape(nq, k).cpu().numpy(), I.t.view(torch.int32).reshape(nq, k).cpu().numpy())


def search(q, index, k):
    """Both workspace variants; they must agree byte for byte."""
    q_t = q if torch.is_tensor(q) else _dev(q)
    a, b = search_once(q_t, index, k, 0), search_once(q_t, index, k, 1)
    assert _same(a, b), 'the result depends on the stale workspace contents or on the workspace alignment'
    return a


def _same(got, want):
    return np.array_equal(got[1], want[1]) and got[0].tobytes() == want[0].tobytes()


def _assert_same(got, want, what):
    if not _same(got, want):
        bad = np.nonzero((got[1] != want[1]).any(1) | (got[0].view(np.uint32) != want[0].view(np.uint32)).any(1))[0]
        r = bad[0]
        raise AssertionError(f'{what}: {len(bad)} query rows differ; row {r}: ids {got[1][r].tolist()} / want {want[1][r].tolist()}, '
                             f'dist {got[0][r].tolist()} / want {want[0][r].tolist()}')


# ---- exact arithmetic ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', sr.GEOMETRY, ids=lambda c: c.name)
def test_exact_geometry(nafp, case):
    q, x = sr.case_inputs(case)
    _assert_same(search(q, Index(x), case.k), sr.case_ref(case), case.name)


def test_split_plans_cover_one_two_ragged_and_capped(nafp):
    """The split counts the exact cases run at, read from the public workspace query: 1, 2, a ragged last split and the cap of
    either template.  Were the policy to change, this says that the coverage went with it (and the restatement in
    _search_ref.plan_splits, which the mutants of the host test follow, is held to the library)."""
    seen = {}
    for c in sr.GEOMETRY + list(sr.LARGE):
        s = n_splits(c.nq, c.n, c.k)
        assert s == sr.plan_splits(c.nq, c.n, sr.template_k(c.k))[0], c.name
        seen.setdefault(s, []).append(c)
    assert 1 in seen and 2 in seen and 3 in seen
    n_tiles = lambda c: (c.n + 63) // 64
    assert any(n_tiles(c) % sr.plan_splits(c.nq, c.n, sr.template_k(c.k))[1] for s in seen if s > 1 for c in seen[s]), 'no ragged last split'
    assert any(c.n % 64 for s in seen if s > 1 for c in seen[s]), 'no ragged last tile behind a split'
    assert n_splits(sr.LARGE[0].nq, sr.LARGE[0].n, 20) == sr.split_cap(20) == 102
    assert n_splits(sr.LARGE[1].nq, sr.LARGE[1].n, 32) == sr.split_cap(32) == 64
    many = n_splits(sr.LARGE_NQ_MANY, sr.LARGE[0].n, 20)
    assert 1 < many < 102                                          # the query blocks lower the split count
    print('split counts covered:', sorted(seen) + [many])


@pytest.fixture(scope='module')
def large_index(nafp):
    return Index(sr.case_inputs(sr.LARGE[0])[1])


def test_exact_large_index_at_the_split_cap_k20(nafp, large_index):
    c = sr.LARGE[0]
    _assert_same(search(sr.case_inputs(c)[0], large_index, c.k), sr.case_ref(c), c.name)


def test_exact_large_index_at_the_split_cap_k32(nafp):
    c = sr.LARGE[1]
    q, x = sr.case_inputs(c)
    _assert_same(search(q, Index(x), c.k), sr.case_ref(c), c.name)


def test_exact_large_index_many_query_blocks(nafp, large_index):
    """2700 queries: 22 query blocks, fewer splits than the cap; the reference for 64 rows, block edges among them."""
    q, sample = sr.large_many_queries()
    D, I = search(q, large_index, 20)
    want = sr.topk_exact(q[sample], large_index.x.cpu().numpy(), 20)
    _assert_same((D[sample], I[sample]), want, 'large-many')


def test_launch_independence_and_repeatability(nafp, large_index):
    """A query's row has the same bytes alone, in a block of 129 and in the full launch (three split plans or block layouts), and
    two calls on one workspace give the same bytes."""
    q, _ = sr.large_many_queries()
    q_t = _dev(q)
    full = search(q_t, large_index, 20)
    for r in (0, 127, 128, 1300, 2699):
        alone = search(q_t[r:r + 1].contiguous(), large_index, 20)
        _assert_same(alone, (full[0][r:r + 1], full[1][r:r + 1]), f'row {r} alone')
        r0 = min(max(0, r - 64), len(q) - 129)
        block = search(q_t[r0:r0 + 129].contiguous(), large_index, 20)
        _assert_same((block[0][r - r0:r - r0 + 1], block[1][r - r0:r - r0 + 1]), alone, f'row {r} in a block of 129')
    _, lib = _lib()
    ws = Guarded(int(lib.nafp_search_workspace_bytes(len(q), large_index.n, 20)), fill=0xFF)
    first = search_once(q_t, large_index, 20, 0, ws=ws)
    _assert_same(search_once(q_t, large_index, 20, 0, ws=ws), first, 'second call on the same workspace')
    _assert_same(first, full, 'reused workspace')


@pytest.mark.parametrize('d', sr.DIMS)
def test_placed_duplicates(nafp, d):
    """More than k copies of one row, placed so that equal keys meet inside one lane's list, across the lane halves, the 32-row
    blocks, tiles, splits and in the ragged last tile: the k smallest positions at distance exactly 0."""
    for k in (20, 32):
        assert n_splits(5, sr.PLACED_N, k) == 3
        for sc in sr.PLACED_SCENARIOS:
            q, x, pos = sr.placed_set(d, k, sc)
            D, I = search(q, Index(x), k)
            for r in (0, 4):
                assert np.array_equal(I[r], pos[:k]) and D[r].tobytes() == np.zeros(k, np.float32).tobytes(), (sc, k, I[r], D[r])
            _assert_same((D, I), sr.topk_exact(q, x, k), f'placed-{sc}-d{d}-k{k}')


def test_k_prefix_property_across_the_two_templates(nafp):
    """k = 1 .. 32 on one index: the result for k is the first k columns of the result for 32 (k <= 20 runs the 20-entry lists,
    k > 20 the 32-entry ones), ids and distance bytes."""
    q, x = sr.case_inputs(sr.PREFIX)
    index, q_t = Index(x), _dev(q)
    full = search(q_t, index, 32)
    _assert_same(full, sr.case_ref(sr.PREFIX), 'k = 32')
    for k in range(1, 32):
        got = search(q_t, index, k)
        _assert_same(got, (np.ascontiguousarray(full[0][:, :k]), np.ascontiguousarray(full[1][:, :k])), f'k = {k}')


@pytest.mark.parametrize('behind', ['queries', 'nan'])
def test_rows_behind_the_index_are_never_returned(nafp, behind):
    """The index is a prefix of a larger allocation whose following rows are copies of the queries (distance 0) or NaN rows; aux
    is prepared for n_index.  The partial last tile relies on the buffer bound of the tile loads and the +inf half norms."""
    for c in sr.BEHIND:
        q, x = sr.case_inputs(c)
        tail = q if behind == 'queries' else np.full((200, c.d), np.nan, np.float32)
        x_all = _dev(np.concatenate([x, tail, tail]))
        got = search(q, Index(x_all, n_index=c.n), c.k)
        assert (got[1] < c.n).all()
        _assert_same(got, sr.case_ref(c), c.name)


def test_short_index_pads_with_minus_one_and_inf(nafp):
    for c in sr.SHORT:
        q, x = sr.case_inputs(c)
        D, I = search(q, Index(x), c.k)
        _assert_same((D, I), sr.case_ref(c), c.name)
        m = min(c.n, c.k)
        assert (I[:, :m] >= 0).all() and (I[:, m:] == -1).all() and np.isposinf(D[:, m:]).all()


def _ivf_search(idx, q_t, k):
    """nafp_ivf_flat_search over the lists of `idx` with every list probed, guarded like the exact search."""
    L, lib = _lib()
    nq, lists = int(q_t.shape[0]), idx._prepare()
    need = int(lib.nafp_ivf_search_workspace_bytes(nq, idx.nlist, idx.nlist, k, 0))
    assert need > 0
    out = []
    for shift, fill in ((0, 0xFF), (8, 0x00)):
        ws, D, I = Guarded(need, shift=shift, fill=fill), Guarded(nq * k * 4), Guarded(nq * k * 4)
        L.check(lib.nafp_ivf_flat_search(L.ptr(q_t), nq, L.ptr(idx.centroids), idx.nlist, idx.d, idx.nlist, L.ptr(lists['rows']),
                                         L.ptr(lists['hn']), L.ptr(lists['row_off']), L.ptr(lists['row_ids']), k, L.ptr(D.t), L.ptr(I.t),
                                         L.ptr(ws.t), need, L.current_stream()), 'ivf_flat_search')
        torch.cuda.synchronize()
        assert D.intact() and I.intact() and ws.intact(), 'a guard was written'
        out.append((D.t.view(torch.float32).reshape(nq, k).cpu().numpy(), I.t.view(torch.int32).reshape(nq, k).cpu().numpy()))
    assert _same(*out)
    return out[0]


@pytest.mark.parametrize('case', sr.IVF, ids=lambda c: c.name)
def test_ivf_flat_with_every_list_probed_gives_the_exact_bytes(nafp, case):
    """The same scan body over inverted lists (built by the index class's own path), nprobe = nlist: the bytes of the exact
    search.  Last, a hand-made assignment deals the rows -- and so the copies of every duplicated row -- round the lists, which
    crosses the relative-row to global-id mapping of the merge."""
    from neural_audio_fp_amd.eval.ivf import IVFFlatIndex
    q, x = sr.case_inputs(case)
    want, q_t = sr.case_ref(case), _dev(q)
    for nlist in sr.IVF_NLIST:
        idx = IVFFlatIndex(case.d, nlist)
        idx.set_params(x[np.linspace(0, case.n - 1, nlist).astype(int)])      # index rows as centroids: integer arithmetic too
        idx.add(x)
        _assert_same(_ivf_search(idx, q_t, case.k), want, f'{case.name} nlist {nlist}')
    idx = IVFFlatIndex(case.d, 8)
    idx.set_params(x[:8])
    idx.add(x)
    idx._assign = torch.from_numpy((np.arange(case.n) * 5 % 8).astype(np.int32)).cuda()
    idx._lists = None
    _assert_same(_ivf_search(idx, q_t, case.k), want, f'{case.name} hand-made lists')
    q2, x2, pos = sr.placed_set(case.d, 20, 'scattered')                          # 24 copies of one row, dealt over 8 lists
    idx = IVFFlatIndex(case.d, 8)
    idx.set_params(x2[:8])
    idx.add(x2)
    idx._assign = torch.from_numpy((np.arange(len(x2)) % 8).astype(np.int32)).cuda()
    idx._lists = None
    assert len(set(pos % 8)) == 8
    got = _ivf_search(idx, _dev(q2), 20)
    assert np.array_equal(got[1][0], pos[:20]) and not got[0][0].any()
    _assert_same(got, sr.topk_exact(q2, x2, 20), 'placed copies in different lists')


# ---- float inputs ------------------------------------------------------------------------------------------------------

def _observe_all(observe, worst):
    for what, v in worst.items():
        observe(what + ' / bound', v, 1.0)


@pytest.mark.parametrize('case', sr.FLOAT_CASES, ids=lambda c: c.name)
def test_float_sets_within_the_derived_bound(nafp, observe, case):
    q, x = sr.float_inputs(case)
    D, I = search(q, Index(x), case.k)
    _observe_all(observe, sr.check(D, I, q, x, case.k))
    if case.kind == 'self':
        rows = np.asarray([np.nonzero((x == q[r]).all(1))[0][0] for r in range(len(q))])
        assert (I == rows[:, None]).any(1).all(), 'a row queried with itself is not among its results'
        b0 = sr.dist_bound(q, x)[np.arange(len(q)), rows]
        assert (D[:, 0] >= 0).all()
        observe('self distance / bound', float((D[:, 0] / b0).max()), 1.0)
    if case.kind == 'norms':
        ip = np.argmax(q.astype(np.float64) @ x.astype(np.float64).T, axis=1)
        assert (ip != I[:, 0]).mean() > 0.5                        # the order is L2, not inner product


def test_power_of_two_scaling_is_exact(nafp):
    """q and x scaled by 2^10 and by 2^-10: identical ids, and distances whose bits are the unscaled ones times 2^20 and 2^-20
    (scaling by a power of two is exact in float32 where nothing under- or overflows)."""
    for case in (sr.FLOAT_CASES[2], sr.FLOAT_CASES[4], sr.FLOAT_CASES[6]):
        q, x = sr.float_inputs(case)
        D, I = search(q, Index(x), case.k)
        for e in (10, -10):
            s = np.float32(2.0 ** e)
            Ds, Is = search(q * s, Index(x * s), case.k)
            _assert_same((Ds, Is), (D * np.float32(2.0 ** (2 * e)), I), f'{case.name} scaled by 2^{e}')


def test_non_finite_rows_and_queries(nafp, observe):
    """What the kernel does, pinned: a key that is NaN or -inf never passes `key > sc[K-1]`, so an index row with a NaN or an
    infinite element is never returned and leaves every other row's result alone; a query row with a NaN gets k times id -1,
    +inf, and the other queries' bytes are unchanged."""
    case = sr.FLOAT_CASES[2]
    q, x = sr.float_inputs(case)
    x = x.copy()
    x[70] = np.nan
    x[1088, 5] = np.inf
    x[300, 17] = -np.inf
    D, I = search(q, Index(x), case.k)
    assert not np.isin(I, (70, 300, 1088)).any()
    _observe_all(observe, sr.check(D, I, q, x, case.k))           # the reference leaves the non-finite rows out
    qn = q.copy()
    qn[3, 9] = np.nan
    qn[128] = np.nan
    Dn, In = search(qn, Index(x), case.k)
    for r in (3, 128):
        assert (In[r] == -1).all() and np.isposinf(Dn[r]).all()
    keep = np.setdiff1d(np.arange(len(q)), (3, 128))
    _assert_same((Dn[keep], In[keep]), (D[keep], I[keep]), 'the other queries next to a NaN query')


def test_status_codes_leave_the_outputs_untouched(nafp):
    L, lib = _lib()
    q, x = sr.case_inputs(sr.PREFIX)
    index, q_t = Index(x), _dev(q)
    nq, k = len(q), 20
    need = int(lib.nafp_search_workspace_bytes(nq, index.n, k))
    ws = Guarded(need)

    def call(nq_, dim, k_, ws_bytes):
        D, I = Guarded(nq * 33 * 4), Guarded(nq * 33 * 4)
        rc = lib.nafp_search_topk_l2(L.ptr(q_t), nq_, L.ptr(index.x), L.ptr(index.aux.t), index.n, dim, k_, L.ptr(D.t), L.ptr(I.t),
                                     L.ptr(ws.t), ws_bytes, L.current_stream())
        torch.cuda.synchronize()
        assert bool((D.raw == GUARD_BYTE).all()) and bool((I.raw == GUARD_BYTE).all()) and bool((ws.raw == GUARD_BYTE).all())
        return rc

    assert call(nq, 96, k, need) == UNSUPPORTED
    assert call(nq, 128, 33, need) == UNSUPPORTED and lib.nafp_search_workspace_bytes(nq, index.n, 33) == -1
    assert call(nq, 128, k, need - 1) == WORKSPACE
    assert call(0, 128, k, need) == OK


def test_equal_output_distances_follow_the_key_order(nafp):
    """The contract's wording (include/nafp.h).  Results are ordered by the float32 key q.x - |x|^2/2, descending, then by id;
    two distinct keys can round to the same written distance, so equal adjacent distances are not always in id order.  Over ALL
    queries of one 20,001 x 128 unit-vector index: the distances are non-decreasing, and wherever two adjacent distances are
    equal with descending ids the float64 distances confirm the order within the bound (a legitimate key order, not a flipped
    tie-break).  The number of such pairs is printed."""
    n, d, k = 20001, 128, 32
    x = sr.unit_rows(n, d, 11)
    index = Index(x)
    D, I = search(x, index, k)
    assert (np.diff(D, axis=1) >= 0).all() and (I >= 0).all() and (I[:, 0] == np.arange(n)).mean() > 0.99
    eq = D[:, 1:] == D[:, :-1]
    desc = eq & (I[:, 1:] < I[:, :-1])
    rows, cols = np.nonzero(desc)
    print(f'adjacent equal distances: {int(eq.sum())}, of which with descending ids: {len(rows)} (of {n * (k - 1)} pairs)')
    x64 = x.astype(np.float64)
    for r, c in zip(rows, cols):
        a, b = I[r, c], I[r, c + 1]
        da, db = ((x64[r] - x64[a]) ** 2).sum(), ((x64[r] - x64[b]) ** 2).sum()
        bound = sr.dist_bound(x[r:r + 1], x[[a, b]])[0]
        assert da - db <= bound.sum(), (r, c, a, b, da, db)
