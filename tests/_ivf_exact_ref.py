"""Exact integer references, input sets, the restated launch plan and mutants for the approximate indexes' selection code
(csrc/ivf.hip: the three IVF-PQ scans, ivf_merge_kernel, ivf_pqr_rerank_kernel, ivf_probe_kernel and the arg-mins of
ivf_pq_encode_kernel / ivf_refine_encode_kernel; nafp_ivf_flat_search with nprobe < nlist).  Plain numpy, no GPU code: imported
by tests/test_ivf_exact_ref_host.py (CPU) and tests/test_gpu_ivf_edges.py (GPU), so both see the same arrays.  Modelled on
tests/_search_ref.py, whose selection (`_select`) and flat reference (`topk_exact`) it reuses.

EXACT ARITHMETIC.  Queries, coarse centroids, PQ codewords and refine codewords are small integers, times one power of two
2^s per case (s = 0, -3, -10).  In units of 2^s (2^2s for squares) the residual q - c, every ADC table entry sum_u (rr - P)^2,
the 64-entry row sum, the re-rank's (c + P) + R and its squared differences are integers far below 2^24: float32 computes them
without rounding in any order, with or without FMA contraction.  Every table entry is at most 2048 units, i.e. it has at most
11 significant bits (2048 itself has one), and at s = -10 it is a multiple of 2^-20 >= the binary16 subnormal spacing 2^-24:
binary16 holds it exactly too, so NAFP_IVF_LUT_F16 must return the bytes of NAFP_IVF_LUT_F32.  The result of every entry point is
then determined bit for bit; the references compute in int64, order by (distance, id) and rescale.  The comparison (`same`) is
np.array_equal on the ids and on the BYTES of the distances, +0.0 for a distance of zero included.  `exactness_margin` returns
the magnitudes this rests on.

THE PLAN.  `ivf_parts`, `part_rows`, `workspace_total` restate ivf_parts / ivf_scan_prologue / ivf_search_layout; the host test
holds them to nafp_ivf_search_workspace_bytes and nafp_ivf_pq_wide_workspace_bytes (host-only computations).

MUTANTS.  `mutate=NAME` makes one deliberate error of a kind the kernels could make; the host test asserts that every mutant
fails `same` on every run it `applies` to (computed from the geometry and the unmutated reference alone):
  tie_larger_id                ties go to the larger id
  kth_keeps_later              of the rows tied with the k-th place the later ones are kept
  part_last_row_dropped        r1 one short in every part of every list
  merge_ties_by_probe_order    the merge orders equal distances by probe rank before id
  wide_threshold_tie_rejected  the wide scan tests `key > thr_key` where it must test `key >= thr_key`: a row that ties the prune
                               threshold's key never reaches the id comparison.  The wave schedule is simulated (rows 64 w ..
                               64 w + 63 of every 256 are wave w's, buffer 240).  In a list in nafp_ivf_bucket's order (ids
                               ascending) a later row has the larger id and loses the tie anyway, so there the mutant changes
                               nothing; it shows on WIDE_PRUNE's `relabelled` order, whose row labels do not ascend
  padding_unwritten            the -1 / +inf padding is not written: the output keeps what it held
  probe_tie_larger_list        equidistant centroids: the larger list id first
  encode_tie_larger_code       equidistant codewords: the larger code
  zero_distance_negative       a distance of exactly zero written as -0.0
  k20_truncated                k in 21 .. 32 served from 20-entry partial lists
  partial_padding_stale        a part with fewer than K rows leaves the rest of its K partial slots unwritten, and they hold an
                               attractive stale entry (key +1e30, i.e. distance -1e30, with the valid id 0), which the GPU test
                               writes into the workspace before one of its two runs of every search
"""
import collections
import functools

import numpy as np

import _search_ref as sr

MUTANTS = ('tie_larger_id', 'kth_keeps_later', 'part_last_row_dropped', 'merge_ties_by_probe_order', 'wide_threshold_tie_rejected',
           'padding_unwritten', 'probe_tie_larger_list', 'encode_tie_larger_code', 'zero_distance_negative', 'k20_truncated',
           'partial_padding_stale')
SEARCH_MUTANTS = ('tie_larger_id', 'kth_keeps_later', 'part_last_row_dropped', 'merge_ties_by_probe_order',
                  'wide_threshold_tie_rejected', 'padding_unwritten', 'zero_distance_negative', 'k20_truncated', 'partial_padding_stale')
STALE_KEY = 1e30                                                  # the stale partial key of the attractive workspace (key = -distance)
RERANK_MUTANTS = ('tie_larger_id', 'kth_keeps_later', 'padding_unwritten', 'zero_distance_negative')
M, KS = 64, 256
RF_M, RF_KS = 4, 16
WAVE_BUFFER = 240
ENTRY_MAX = 2048
DIMS = (64, 128, 256)
SENT_I = np.int32(-0x5A5A5A5B)                                    # what the GPU test pre-fills its outputs with
SENT_D = np.array([0x7FC0DEAD], np.uint32).view(np.float32)[0]


def same(got, want):
    """The comparison of the GPU tests: every array of `got` has the shape, type and BYTES of its counterpart."""
    got = got if isinstance(got, (tuple, list)) else (got,)
    want = want if isinstance(want, (tuple, list)) else (want,)
    return len(got) == len(want) and all(np.asarray(g).shape == np.asarray(w).shape and np.asarray(g).dtype == np.asarray(w).dtype
                                         and np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


def ints(a, s=0):
    """int64 array of a / 2^s, which must be integers."""
    v = np.asarray(a, np.float64) * 2.0 ** -s
    out = np.rint(v).astype(np.int64)
    assert np.array_equal(out, v), 'the exact references take integers times 2^s'
    return out


def _rescale(dist, s):
    """float32 of integer distances (float64 array, +inf = none) times 2^2s: exact."""
    return (np.asarray(dist, np.float64) * 4.0 ** s).astype(np.float32)


# ---- the plan --------------------------------------------------------------------------------------------------------

def template_k(k, wide=False):
    """The partial-list length that serves k results: 20 / 32 compiled into the narrow scans, k1 itself in the wide one."""
    return k if wide else (20 if k <= 20 else 32)


def ivf_parts(n_pairs, np_, K, kind=1):
    """Parts per list of a search (ivf_parts in csrc/ivf.hip)."""
    slots = 2 if kind == 0 else 1
    cap = max(1, 16384 // (np_ * slots * K))
    base = (n_pairs + 127) // 128 if kind == 0 else n_pairs
    want = -(-2048 // base) if base > 0 else 1
    return max(1, min(cap, want))


def part_rows(length, parts, part):
    """[r0, r1) of a list of `length` rows that part `part` of `parts` scans (ivf_scan_prologue)."""
    per = -(-length // parts)
    r0 = min(length, part * per)
    return r0, min(length, r0 + per)


def _align256(b):
    return (b + 255) // 256 * 256


def bucket_workspace(n, nb, batch):
    n_tiles = max(1, -(-n // 4096))
    return _align256(batch * n_tiles * nb * 4) + _align256(batch * nb * 4) + 256


def workspace_total(nq, nlist, nprobe, k, kind=1, wide=False):
    """(bytes, parts) of ivf_search_layout: probe, pair offsets, sorted, qmap, plist, inv (n_pairs ints each but the offsets),
    query-block offsets, the partial keys and ids (n_pairs x slots x parts x K), the bucketing workspace, 256 spare."""
    np_ = min(nprobe, nlist)
    K = template_k(k, wide)
    n_pairs = nq * np_
    parts = ivf_parts(n_pairs, np_, K, kind)
    slotsK = (2 if kind == 0 else 1) * parts * K
    total = 5 * _align256(n_pairs * 4) + 2 * _align256((nlist + 1) * 4) + 2 * _align256(n_pairs * slotsK * 4)
    return total + _align256(bucket_workspace(n_pairs, nlist, 1)) + 256, parts


def partial_lists_at(nq, nlist, nprobe, k, kind=1, wide=False):
    """(byte offset of the partial keys, of the partial ids, their count) in the 256-byte aligned workspace of a search."""
    np_ = min(nprobe, nlist)
    n_pairs = nq * np_
    m = n_pairs * (2 if kind == 0 else 1) * ivf_parts(n_pairs, np_, template_k(k, wide), kind) * template_k(k, wide)
    o_pk = 5 * _align256(n_pairs * 4) + 2 * _align256((nlist + 1) * 4)
    return o_pk, o_pk + _align256(m * 4), m


# ---- integer references ------------------------------------------------------------------------------------------------

def decode(pq, codes):
    """(n, d) the codewords the codes (n, m) name, pq (m, ks, dsub)."""
    m = pq.shape[0]
    return np.concatenate([pq[j][np.asarray(codes)[:, j].astype(np.int64)] for j in range(m)], 1)


def sq_distances(a, b):
    """(na, nb) int64 |a - b|^2 of int64 rows."""
    return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)


def probe_exact(q, cent, nprobe, scale=0, mutate=None):
    """(nq, min(nprobe, nlist)) int32: the nearest lists by (distance, list id)."""
    dist = sq_distances(ints(q, scale), ints(cent, scale))
    lid = np.broadcast_to(np.arange(dist.shape[1]), dist.shape)
    order = np.lexsort((-lid if mutate == 'probe_tie_larger_list' else lid, dist), axis=1)
    return order[:, :min(nprobe, dist.shape[1])].astype(np.int32)


def adc_tables_exact(q, cent, pq, pair_q, pair_l, scale=0):
    """(n_pairs, 64, 256) float32: entry [m][c] = sum_u (q - cent[l] - pq[m][c])_u^2; and the largest entry in units."""
    qi, ci, pi = ints(q, scale), ints(cent, scale), ints(pq, scale)
    rr = (qi[pair_q] - ci[pair_l]).reshape(len(pair_q), M, 1, -1)
    T = ((rr - pi[None]) ** 2).sum(-1)
    return _rescale(T, scale), int(T.max())


def _finish(D, I, k, scale, mutate):
    D, I = _rescale(D, scale), I.astype(np.int32)
    if mutate == 'padding_unwritten':
        D, I = np.where(I >= 0, D, SENT_D), np.where(I >= 0, I, SENT_I)
    if mutate == 'zero_distance_negative':
        D = np.where(D == 0, np.float32(-0.0), D)
    return np.ascontiguousarray(D, np.float32), np.ascontiguousarray(I, np.int32)


def wave_filter(dist, lab, K, strict=False):
    """One workgroup of the wide scan over a part's rows (distances and labels in list order): (kept row indices, best first;
    prunes of each of the 4 waves; indices taken although they only TIE the threshold's distance, on their smaller label).
    strict: the mutant `key > thr_key`."""
    n = len(dist)
    final, prunes, by_tie = [], [], set()
    for w in range(4):
        held, thr, npr = [], None, 0
        for rb in range(0, n, 256):
            take = []
            for i in range(rb + 64 * w, min(n, rb + 64 * w + 64)):
                if thr is None or dist[i] < thr[0]:
                    take.append(i)
                elif dist[i] == thr[0] and lab[i] < thr[1] and not strict:
                    take.append(i)
                    by_tie.add(i)
            if take and len(held) + len(take) > WAVE_BUFFER:
                held = sorted(held)[:K]
                thr, npr = held[-1][:2], npr + 1
            held += [(dist[i], lab[i], i) for i in take]          # one that no longer beats the new threshold falls at the next prune
        final += sorted(held)[:K]
        prunes.append(npr)
    return [t[2] for t in sorted(final)[:K]], prunes, by_tie


def _simulate(drow, lab, probes_q, rows_of_list, parts, K, k, mutate, wide):
    """One query through the partial lists as the kernels build them: per probed list and part its K best by (distance, label),
    then the merge to k.  Returns (D float64 (k,), I int64 (k,), row indices of the results taken on a threshold tie)."""
    cands, by_tie = [], set()
    for rank, l in enumerate(probes_q):
        rows = rows_of_list[l]
        for p in range(parts):
            r0, r1 = part_rows(len(rows), parts, p)
            if mutate == 'part_last_row_dropped' and r1 > r0:
                r1 -= 1
            seg = rows[r0:r1]
            if wide and len(seg) > WAVE_BUFFER:
                kept, _, tied = wave_filter(drow[seg], lab[seg], K, strict=mutate == 'wide_threshold_tie_rejected')
                by_tie |= {int(seg[i]) for i in tied}
                seg = seg[kept]
            else:
                seg = seg[np.lexsort((lab[seg], drow[seg]))[:K]]
            cands += [(drow[i], rank if mutate == 'merge_ties_by_probe_order' else 0, lab[i], i) for i in seg]
            if mutate == 'partial_padding_stale':
                cands += [(-STALE_KEY, 0, 0, -1)] * (K - len(seg))
    cands = sorted(cands)[:k]
    D, I = np.full(k, np.inf), np.full(k, -1, np.int64)
    D[:len(cands)] = [c[0] for c in cands]
    I[:len(cands)] = [c[2] for c in cands]
    return D, I, by_tie & {int(c[3]) for c in cands}


_SIMULATED = ('part_last_row_dropped', 'merge_ties_by_probe_order', 'wide_threshold_tie_rejected', 'k20_truncated', 'partial_padding_stale')


def adc_topk_exact(q, cent, pq, codes, list_of_row, probes, k, scale=0, mutate=None, nq_launch=None, wide=False, labels=None,
                   simulate=False):
    """(D float32, I int32), (nq, k): the k nearest rows of the probed lists by (ADC distance, row id) in int64, +inf / -1
    padding.  nq_launch: the number of queries of the launch q is a sample of (it decides `parts`); wide: the wide scan's plan;
    labels: the id each row goes by (default: its index); simulate: go through the partial lists even without a mutant."""
    assert mutate is None or mutate in SEARCH_MUTANTS, mutate
    qi = ints(q, scale)
    y = ints(cent, scale)[list_of_row] + decode(ints(pq, scale), codes)
    dist = sq_distances(qi, y).astype(np.float64)
    nq, n = dist.shape
    nlist = len(cent)
    lab = np.arange(n) if labels is None else np.asarray(labels, np.int64)
    probed = np.zeros((nq, nlist), bool)
    np.put_along_axis(probed, np.asarray(probes, np.int64), True, 1)
    dist = np.where(probed[:, list_of_row], dist, np.inf)
    if mutate in _SIMULATED or simulate:
        np_ = probes.shape[1]
        K = 20 if mutate == 'k20_truncated' and not wide else template_k(k, wide)
        parts = ivf_parts((nq if nq_launch is None else nq_launch) * np_, np_, template_k(k, wide))
        rows_of_list = [np.nonzero(np.asarray(list_of_row) == l)[0] for l in range(nlist)]
        out = [_simulate(dist[r], lab, probes[r], rows_of_list, parts, K, k, mutate, wide) for r in range(nq)]
        D, I = np.array([o[0] for o in out]), np.array([o[1] for o in out])
    else:
        by_label = np.empty_like(dist)
        by_label[:, lab] = dist
        D, I = sr._select(by_label, k, mutate if mutate in ('tie_larger_id', 'kth_keeps_later') else None)
    return _finish(D, I, k, scale, mutate)


def flat_topk_exact(q, x, list_of_row, probes, k):
    """IVF-Flat with nprobe < nlist: _search_ref.topk_exact restricted to the rows of each query's probed lists."""
    D, I = np.full((len(q), k), np.inf, np.float32), np.full((len(q), k), -1, np.int32)
    for r in range(len(q)):
        rows = np.nonzero(np.isin(list_of_row, probes[r]))[0]
        if len(rows):
            d, i = sr.topk_exact(q[r:r + 1], x[rows], k)
            D[r], I[r] = d[0], np.where(i[0] >= 0, rows[np.maximum(i[0], 0)], -1)
    return D, I


def reconstruct(cent, pq, refine, codes, rcodes, list_of_row, scale=0):
    """(n, d) int64 (centroid + PQ codewords) + refine codewords; rcodes (n, 2) nibble-packed."""
    rc = np.stack([rcodes[:, 0] & 15, rcodes[:, 0] >> 4, rcodes[:, 1] & 15, rcodes[:, 1] >> 4], 1)
    return ints(cent, scale)[list_of_row] + decode(ints(pq, scale), codes) + decode(ints(refine, scale), rc)


def rerank_exact(q, cand, cent, pq, refine, codes, rcodes, list_of_row, n_rows, k, scale=0, mutate=None):
    """nafp_ivf_pqr_rerank: per query the candidates cand (nq, k1) -- -1 holes skipped, ids >= n_rows ignored, a candidate named
    twice twice, the earlier slot first -- by (|q - reconstruction|^2, id); the k smallest, +inf / -1 padding."""
    assert mutate is None or mutate in RERANK_MUTANTS, mutate
    qi = ints(q, scale)
    rec = reconstruct(cent, pq, refine, codes, rcodes, list_of_row, scale)
    D, I = np.full((len(qi), k), np.inf), np.full((len(qi), k), -1, np.int64)
    for r in range(len(qi)):
        c = np.asarray(cand[r], np.int64)
        c = c[(c >= 0) & (c < n_rows)]
        if not len(c):
            continue
        d = ((qi[r] - rec[c]) ** 2).sum(1)
        order = np.lexsort((np.arange(len(c)), -c if mutate == 'tie_larger_id' else c, d))
        if mutate == 'kth_keeps_later' and len(c) > k:
            tied = order[d[order] == d[order[k - 1]]]
            m = int((d[order[:k]] == d[order[k - 1]]).sum())
            order = np.concatenate([order[:k - m], tied[len(tied) - m:]])
        order = order[:k]
        D[r, :len(order)], I[r, :len(order)] = d[order], c[order]
    return _finish(D, I, k, scale, mutate)


def _argmin(dist, mutate):
    """arg-min along the last axis, the smaller index on equal distance (mutant: the larger)."""
    if mutate == 'encode_tie_larger_code':
        return dist.shape[-1] - 1 - np.argmin(dist[..., ::-1], axis=-1)
    return np.argmin(dist, axis=-1)


def encode_exact(x, pq, assign=None, coarse=None, scale=0, mutate=None):
    """(n, 64) uint8: per sub-space the nearest codeword of x - coarse[assign] (of x itself without assign)."""
    r = ints(x, scale) - (0 if assign is None else ints(coarse, scale)[assign])
    pi = ints(pq, scale)
    dist = ((r.reshape(len(r), M, 1, -1) - pi[None]) ** 2).sum(-1)
    return _argmin(dist, mutate).astype(np.uint8)


def refine_encode_exact(x, refine, packed, scale=0, mutate=None):
    """(n, 4) codes, or (n, 2) bytes c0 | c1 << 4, c2 | c3 << 4: per refine sub-space the nearest of 16 codewords."""
    xi, ri = ints(x, scale), ints(refine, scale)
    c = _argmin(((xi.reshape(len(xi), RF_M, 1, -1) - ri[None]) ** 2).sum(-1), mutate).astype(np.uint8)
    return np.stack([c[:, 0] | (c[:, 1] << 4), c[:, 2] | (c[:, 3] << 4)], 1).astype(np.uint8) if packed else c


# ---- input sets --------------------------------------------------------------------------------------------------------

class Case:
    """An index and its queries as integers (int64) with the scale exponent s, the float32 arrays a call gets (`f`), and the
    searches to run: narrow (nq, nprobe, k), wide (nq, nprobe, k1).  labels: the id a row goes by in the wide searches (None:
    its index, i.e. lists as nafp_ivf_bucket leaves them)."""

    def __init__(self, name, s, q, cent, pq, refine, codes, rcodes, lists, narrow=(), wide=(), labels=None, x=None):
        self.name, self.s = name, s
        self.q, self.cent, self.pq, self.refine = (np.asarray(a, np.int64) for a in (q, cent, pq, refine))
        self.codes, self.rcodes = np.ascontiguousarray(codes, np.uint8), np.ascontiguousarray(rcodes, np.uint8)
        self.lists = np.ascontiguousarray(lists, np.int32)
        self.narrow, self.wide, self.labels = tuple(narrow), tuple(wide), labels
        self.d, self.nlist, self.n = self.q.shape[1], len(self.cent), len(self.codes)
        self.x = x                                                # encoder cases: the rows to encode

    def f(self, what):
        return np.ascontiguousarray(getattr(self, what) * 2.0 ** self.s, np.float32)

    def recon(self):
        return self.cent[self.lists] + decode(self.pq, self.codes)

    @functools.lru_cache(maxsize=None)
    def probes(self, nq, nprobe):
        return probe_exact(self.f('q')[:nq], self.f('cent'), nprobe, self.s)

    @functools.lru_cache(maxsize=None)
    def ref(self, nq, nprobe, k, wide=False):
        """The unmutated reference of one search (shared by the tests; nobody modifies it)."""
        lab = self.labels if wide else None
        return adc_topk_exact(self.f('q')[:nq], self.f('cent'), self.f('pq'), self.codes, self.lists, self.probes(nq, nprobe), k,
                              self.s, wide=wide, labels=lab)

    def __repr__(self):
        return self.name


def _book(rng, d, amax=3):
    """PQ codewords in {-amax .. amax} and refine codewords in {-1, 0, 1}: many duplicates, so equidistant codes abound."""
    return rng.integers(-amax, amax + 1, size=(M, KS, d // M)), rng.integers(-1, 2, size=(RF_M, RF_KS, d // RF_M))


def _rcodes(rng, n):
    return rng.integers(0, 256, size=(n, 2)).astype(np.uint8)


# distinct sums of two squares: the `level` a row's codes in sub-spaces 0 and 1 give it, whatever the query
_AB = sorted({a * a + b * b: (a, b) for a in range(30) for b in range(a + 1)}.items())
LEVELS = np.array([v for v, _ in _AB][:64])
_LEVEL_AB = np.array([ab for _, ab in _AB][:64])


def _levelled(rng, d, nlist, n, nq, level):
    """Rows whose ADC distance to query j is const(j) + LEVELS[level[i]], in EVERY list: sub-spaces 0 and 1 hold codeword j =
    (j, 0 ..) and no residual (queries and centroids are 0 there), sub-space 63 holds codeword 0 in every row, and the centroids
    differ only in the last coordinate, by +-1 around the queries' 0; all other codes are one shared row."""
    dsub = d // M
    pq, refine = _book(rng, d)
    pq[0] = pq[1] = 0
    pq[0, :, 0] = pq[1, :, 0] = np.minimum(np.arange(KS), 31)
    pq[63, 0] = 0
    cent = np.tile(rng.integers(-2, 3, size=d), (nlist, 1))
    cent[:, :2 * dsub] = 0
    cent[:, -dsub:] = 0
    cent[:, -1] = np.where(np.arange(nlist) % 2 == 0, -1, 1)
    q = cent[0] + rng.integers(-1, 2, size=(nq, d))
    q[:, :2 * dsub] = 0
    q[:, -dsub:] = 0
    codes = np.tile(rng.integers(0, KS, size=M), (n, 1))
    codes[:, 0], codes[:, 1], codes[:, 63] = _LEVEL_AB[level, 0], _LEVEL_AB[level, 1], 0
    return q, cent, pq, refine, codes


@functools.lru_cache(maxsize=None)
def all_tied():
    """One list of 785 = 3 x 256 + 17 rows with identical codes: every answer is the k smallest ids.  nq = 1: 819 parts for 785
    rows (empty parts); nq = 2048: one part; wide k1 = 128 with nq = 1: 128 parts of 7 rows."""
    rng = np.random.default_rng(1)
    n, d = 785, 64
    pq, refine = _book(rng, d)
    cent = rng.integers(-2, 3, size=(1, d))
    q = rng.integers(-2, 3, size=(2048, d))
    codes = np.tile(rng.integers(0, KS, size=M), (n, 1))
    return Case('all_tied', 0, q, cent, pq, refine, codes, _rcodes(rng, n), np.zeros(n), labels=None,
                narrow=((1, 1, 20), (3, 1, 20), (3, 1, 32), (2048, 1, 20), (2048, 1, 32)), wide=((1, 1, 128), (3, 1, 33), (2048, 1, 128)))


@functools.lru_cache(maxsize=None)
def few_values(d, s=0):
    """1 003 rows dealt to 8 lists as i % 8 (ids interleave across lists: the merge must order by global id).  The centroids are
    c0 +- 1 in three coordinates whose sub-spaces hold a zero codeword in every row, and three further sub-spaces hold one of two
    codewords: for the even queries (which equal c0 in those coordinates) every list is equally far and a row's distance takes 8
    values; the odd queries are perturbed there, so their lists differ and the values multiply.  Ties are everywhere."""
    rng = np.random.default_rng([2, d])
    n, nlist, nq, dsub = 1003, 8, 131, d // M
    pq, refine = _book(rng, d)
    c0 = rng.integers(-1, 2, size=d)
    cent = np.tile(c0, (nlist, 1))
    codes = np.tile(rng.integers(0, KS, size=M), (n, 1))
    q = c0 + rng.integers(-1, 2, size=(nq, d))
    for j in range(3):
        cent[:, -1 - j * dsub] += np.where((np.arange(nlist) >> j) & 1, 1, -1)
        pq[63 - j, codes[0, 63 - j]] = 0
        q[0::2, -1 - j * dsub] = c0[-1 - j * dsub]
    two = rng.integers(0, KS, size=(3, 2))
    for j in range(3):
        codes[:, j] = two[j, rng.integers(0, 2, size=n)]
    name = f'few_values-d{d}' + (f'-s{s}' if s else '')
    return Case(name, s, q, cent, pq, refine, codes, _rcodes(rng, n), np.arange(n) % nlist,
                narrow=((131, 1, 20), (131, 3, 21), (131, 8, 32), (5, 3, 20)), wide=((131, 3, 80), (131, 8, 128), (5, 1, 33)))


KTH_T = 12                                                        # rows per level: no k of the tests is a multiple of it


@functools.lru_cache(maxsize=None)
def kth_tie():
    """Levels of T = 12 rows, 11 of them, scattered over 1 201 rows in two lists (i % 2) that tie exactly (the query lies halfway
    between the two centroids); all other rows are far.  The k-th place of every k in 1, 20, 21, 32, 33, 64, 127, 128 falls
    inside a level, which straddles lanes, waves, parts and both lists: only its smallest ids may appear."""
    rng = np.random.default_rng(3)
    n, d = 1201, 128
    level = np.full(n, 63)
    level[rng.permutation(n)[:11 * KTH_T]] = np.repeat(np.arange(11), KTH_T)
    q, cent, pq, refine, codes = _levelled(rng, d, 2, n, 131, level)
    return Case('kth_tie', 0, q, cent, pq, refine, codes, _rcodes(rng, n), np.arange(n) % 2,
                narrow=tuple((nq, 2, k) for nq in (5, 131) for k in (1, 20, 21, 32)),
                wide=tuple((nq, 2, k1) for nq in (5, 131) for k1 in (33, 64, 127, 128)))


WIDE_PRUNE_N = 2003
WIDE_PRUNE_K1 = (5, 20, 80, 128)


@functools.lru_cache(maxsize=None)
def wide_prune(order):
    """One list of 2 003 rows scanned in ONE part (2 048 queries x 1 probe), 9 levels (11 in the shuffled order).
    late: along EACH WAVE's sequence t (rows 64 w .. 64 w + 63 of every 256) the level falls every 24 rows up to t = 192 and
    stays at its lowest from there, for 1 235 rows of which the k1 smallest ids are the answer: a wave prunes at t = 192 and again
    once that level has filled its buffer, which puts the threshold INSIDE the level with batches of it still to come;
    shuffled: the rows of t < 192 in a drawn order among themselves and the later ones at one of three low levels, drawn: the
    threshold moves down through those three, so every wave still prunes at least twice at every k1, on distances that neither
    fall nor rise along the list; relabelled: the late order under drawn row labels, so rows that tie the prune
    threshold arrive with smaller AND larger ids than the threshold's (module docstring, wide_threshold_tie_rejected)."""
    rng = np.random.default_rng(4)
    n, d = WIDE_PRUNE_N, 64
    t = np.arange(n) // 256 * 64 + np.arange(n) % 64
    level = np.where(t < 192, 62 - t // 24, 54)
    labels = None
    if order == 'shuffled':
        r41 = np.random.default_rng(41)
        head = np.nonzero(t < 192)[0]
        level[head] = level[r41.permutation(head)]
        level[t >= 192] = r41.integers(52, 55, size=int((t >= 192).sum()))
    elif order == 'relabelled':
        labels = np.random.default_rng(42).permutation(n)
    else:
        assert order == 'late'
    q, cent, pq, refine, codes = _levelled(rng, d, 1, n, 2048, level)
    return Case(f'wide_prune-{order}', 0, q, cent, pq, refine, codes, _rcodes(rng, n), np.zeros(n), labels=labels,
                narrow=() if labels is not None else ((2048, 1, 20), (2048, 1, 32)), wide=tuple((2048, 1, k1) for k1 in WIDE_PRUNE_K1))


@functools.lru_cache(maxsize=None)
def short_lists(nlist=6):
    """Lists of 7, 0, 5, 0, 11, 0 rows: fewer than k rows in all, empty probed lists, and queries 1 and 3 sit on the centroids of
    empty lists whose neighbour is empty too (nprobe <= 2: a row of padding only).  nlist = 1: nprobe 5 is clamped to 1."""
    rng = np.random.default_rng([5, nlist])
    d = 256
    pq, refine = _book(rng, d)
    if nlist == 1:
        cent, lists = rng.integers(-2, 3, size=(1, d)), np.zeros(9)
        q = cent[0] + rng.integers(-1, 2, size=(4, d))
        runs, wruns = ((4, 5, 20), (1, 1, 32)), ((4, 5, 100),)
    else:
        cent = rng.integers(-2, 3, size=(nlist, d))
        cent[3] = cent[1]                                         # the two empty lists are each other's nearest
        cent[3, 0] += 1
        lists = np.repeat([0, 2, 4], [7, 5, 11])
        q = np.concatenate([cent, cent[:1] + rng.integers(-1, 2, size=(3, d))])
        runs, wruns = ((9, 1, 20), (9, 2, 32), (9, 3, 21), (9, 6, 32)), ((9, 2, 100), (9, 6, 128))
    n = len(lists)
    codes = rng.integers(0, KS, size=(n, M))
    return Case(f'short_lists-nlist{nlist}', 0, q, cent, pq, refine, codes, _rcodes(rng, n), lists, narrow=runs, wide=wruns)


@functools.lru_cache(maxsize=None)
def zero_distance():
    """Queries equal to centroid + decoded codes of rows 0 .. 19; rows 300 .. 339 are copies of rows 0 .. 39 (same list): distance
    exactly 0 at the first places, tied."""
    rng = np.random.default_rng(6)
    n, d, nlist = 340, 128, 4
    pq, refine = _book(rng, d)
    cent = rng.integers(-2, 3, size=(nlist, d))
    codes, lists = rng.integers(0, KS, size=(n, M)), rng.integers(0, nlist, size=n)
    codes[300:], lists[300:] = codes[:40], lists[:40]
    q = (cent[lists] + decode(pq, codes))[:20]
    return Case('zero_distance', 0, q, cent, pq, refine, codes, _rcodes(rng, n), lists,
                narrow=((20, 4, 20), (20, 2, 32), (1, 4, 1)), wide=((20, 4, 80), (20, 1, 33)))


@functools.lru_cache(maxsize=None)
def spread(d, s=0):
    """Drawn small integers with few ties: the plain arithmetic (table fill with u ascending, the 64-lookup sum, the residual)
    on the same exact footing."""
    rng = np.random.default_rng([7, d])
    n, nlist, nq = 1500, 8, 131
    pq, refine = _book(rng, d)
    cent = rng.integers(-2, 3, size=(nlist, d))
    codes, lists = rng.integers(0, KS, size=(n, M)), rng.integers(0, nlist, size=n)
    q = rng.integers(-2, 3, size=(nq, d))
    name = f'spread-d{d}' + (f'-s{s}' if s else '')
    return Case(name, s, q, cent, pq, refine, codes, _rcodes(rng, n), lists, narrow=((131, 3, 20), (131, 8, 32), (1, 3, 21)),
                wide=((131, 3, 100), (1, 8, 128)))


@functools.lru_cache(maxsize=None)
def probe_ties():
    """12 centroids: +-e_0 .. +-e_3 (equidistant from the query 0 and, in pairs, from others), and four copies of one further
    centroid.  Query 0 is the origin: 8 lists tie at distance 1, so nprobe = 5 cuts inside the tie group."""
    rng = np.random.default_rng(8)
    n, d, nlist = 400, 64, 12
    pq, refine = _book(rng, d)
    cent = np.zeros((nlist, d), np.int64)
    for j in range(4):
        cent[2 * j, j], cent[2 * j + 1, j] = 1, -1
    cent[8:] = rng.integers(-1, 2, size=d)
    q = np.concatenate([np.zeros((1, d), np.int64), cent[8:9], rng.integers(-1, 2, size=(19, d))])
    q[3:8, :4] = 0                                               # equidistant from the eight unit centroids again
    codes, lists = rng.integers(0, KS, size=(n, M)), rng.integers(0, nlist, size=n)
    return Case('probe_ties', 0, q, cent, pq, refine, codes, _rcodes(rng, n), lists, narrow=((21, 1, 20), (21, 5, 20), (21, 12, 32)),
                wide=((21, 5, 80),))


PROBE_TIES_NPROBE = (1, 5, 12)


@functools.lru_cache(maxsize=None)
def encode_ties(d):
    """257 rows (one workgroup and one row) with entries in -3 .. 3 against codewords in {-2, 0, 2}: duplicate codewords, and every
    odd residual lies exactly halfway between two of them."""
    rng = np.random.default_rng([9, d])
    n, nlist = 257, 5
    pq = 2 * rng.integers(-1, 2, size=(M, KS, d // M))
    refine = 2 * rng.integers(-1, 2, size=(RF_M, RF_KS, d // RF_M))
    cent = rng.integers(-2, 3, size=(nlist, d))
    lists = rng.integers(0, nlist, size=n)
    x = cent[lists] + rng.integers(-3, 4, size=(n, d))
    return Case(f'encode_ties-d{d}', 0, x[:1], cent, pq, refine, np.zeros((n, M)), np.zeros((n, 2)), lists, x=x)


RERANK_RUNS = ((1, 1), (100, 32), (100, 20), (128, 32), (128, 1), (20, 20))      # (k1, k)


@functools.lru_cache(maxsize=None)
def rerank(d):
    """400 rows of which 300 .. 399 repeat rows 0 .. 99 (tied reconstructions); candidates (9, 128), of which a run uses the first
    k1 columns: drawn rows, -1 holes, row 3 all -1, ids >= n_rows in row 5, a candidate named twice in rows 0 and 6, row 7 with 3
    valid candidates (fewer than k), row 8 = query equal to a reconstruction (distance 0)."""
    rng = np.random.default_rng([10, d])
    n, nlist = 400, 4
    pq, refine = _book(rng, d)
    cent = rng.integers(-2, 3, size=(nlist, d))
    codes, lists, rcodes = rng.integers(0, KS, size=(n, M)), rng.integers(0, nlist, size=n), _rcodes(rng, n)
    codes[300:], lists[300:], rcodes[300:] = codes[:100], lists[:100], rcodes[:100]
    case = Case(f'rerank-d{d}', 0, np.zeros((9, d)), cent, pq, refine, codes, rcodes, lists)
    rec = reconstruct(cent, pq, refine, case.codes, case.rcodes, case.lists)
    case.q = rec[rng.integers(0, n, size=9)] + rng.integers(-1, 2, size=(9, d))
    case.q[8] = rec[17]
    cand = np.stack([rng.permutation(n)[:128] for _ in range(9)])
    cand[:, :40] = np.where(cand[:, :40] < 100, cand[:, :40] + 300, cand[:, :40])    # copies first: a row and its copy both named
    cand[:, 7::9] = -1
    cand[0, 0] = cand[0, 5] = 1                                  # k1 = 1 included: slot 0 holds a candidate
    cand[3] = -1
    cand[5, 90:] = n + np.arange(38)
    cand[6, 2:30:3] = cand[6, 1]
    cand[7, 3:] = -1
    cand[8, 0], cand[8, 1] = 317, 17
    case.cand = np.ascontiguousarray(cand, np.int32)
    return case


def search_cases():
    """Every case the search entry points run on."""
    return ([all_tied()] + [few_values(d) for d in DIMS] + [few_values(64, -3), few_values(128, -10), kth_tie()]
            + [wide_prune(o) for o in ('late', 'shuffled', 'relabelled')] + [short_lists(6), short_lists(1), zero_distance()]
            + [spread(128), spread(256), spread(128, -3), spread(256, -10), spread(64, -10), probe_ties()])


def flat_cases():
    """(case, nprobe, k) of nafp_ivf_flat_search with nprobe < nlist; the rows are the cases' reconstructions cent + decode."""
    return [(few_values(64), 3, 20), (few_values(128), 1, 32), (short_lists(6), 2, 20), (short_lists(6), 3, 32), (probe_ties(), 5, 20),
            (probe_ties(), 1, 21)]


BATCH_NQ = (1, 131, 2048)                                         # batching independence: three different `parts`


# ---- margins and regimes -------------------------------------------------------------------------------------------------

def exactness_margin(case):
    """{'entry': the largest ADC table entry over all (query, list) pairs in units (<= 2048), 'row': the largest 64-entry sum,
    'rerank': the largest re-rank sum (both < 2^24), 'f16_exact': every entry times 4^s is a multiple of the binary16 spacing at
    its magnitude}."""
    rr = (case.q[:, None, :] - case.cent[None, :, :]).reshape(-1, M, 1, case.d // M)
    entry = 0
    f16_exact = True
    for c0 in range(0, len(rr), 64):
        T = ((rr[c0:c0 + 64] - case.pq[None]) ** 2).sum(-1)
        entry = max(entry, int(T.max()))
        v = T.astype(np.float64) * 4.0 ** case.s
        spacing = 2.0 ** np.maximum(np.floor(np.log2(np.maximum(v, 2.0 ** -30))) - 10, -24)
        f16_exact &= bool((v / spacing == np.floor(v / spacing)).all() and v.max() <= 65504)
    row = int(entry * M)
    rec = reconstruct(case.cent, case.pq, case.refine, case.codes, case.rcodes, case.lists)
    lo, hi = np.minimum(case.q.min(0), rec.min(0)), np.maximum(case.q.max(0), rec.max(0))
    return {'entry': entry, 'row': row, 'rerank': int(((hi - lo) ** 2).sum()), 'f16_exact': f16_exact}


def simulated_prunes(case, k1, query=0):
    """Prunes per wave of the one-part wide scan of `query` over list 0."""
    rows = np.nonzero(case.lists == 0)[0]
    dist = sq_distances(case.q[query:query + 1], case.recon()[rows])[0]
    lab = rows if case.labels is None else case.labels[rows]
    return wave_filter(dist, lab, k1)[1]


def applies(mutant, case, nq, nprobe, k, wide, sample=None):
    """Whether `mutant` must change the result of the run (nq, nprobe, k) of `case` on the query rows `sample` (default: all): from
    the plan, the lists and the unmutated reference alone."""
    sample = np.arange(nq) if sample is None else np.asarray(sample)
    D, I = (a[sample] for a in case.ref(nq, nprobe, k, wide))
    probes = case.probes(nq, nprobe)[sample]
    np_ = probes.shape[1]
    lab = case.labels if wide and case.labels is not None else np.arange(case.n)
    row_of = np.argsort(lab)                                      # label -> row
    dist = sq_distances(case.q[:nq][sample], case.recon()).astype(np.float64)
    probed = np.zeros((len(sample), case.nlist), bool)
    np.put_along_axis(probed, probes.astype(np.int64), True, 1)
    dist = np.where(probed[:, case.lists], dist, np.inf) * 4.0 ** case.s
    kth = D[:, -1].astype(np.float64)
    n_tied = (dist == kth[:, None]).sum(1)                        # rows at the k-th distance (0 where the k-th place is padding)
    kept_tied = (D.astype(np.float64) == kth[:, None]).sum(1)
    straddle = bool((np.isfinite(kth) & (n_tied > kept_tied)).any())
    inside = bool((np.isfinite(D[:, 1:]) & (D[:, 1:] == D[:, :-1])).any())
    parts = ivf_parts(nq * np_, np_, template_k(k, wide))
    pos = np.zeros(case.n, np.int64)                              # position of a row in its list
    length = np.bincount(case.lists, minlength=case.nlist)
    for l in range(case.nlist):
        rows = np.nonzero(case.lists == l)[0]
        pos[rows] = np.arange(len(rows))
    got = I >= 0
    rows_got = row_of[np.maximum(I, 0)]
    per = np.maximum(1, -(-length[case.lists[rows_got]] // parts))
    part = pos[rows_got] // per
    if mutant == 'tie_larger_id':
        return inside or straddle
    if mutant == 'kth_keeps_later':
        return straddle
    if mutant == 'padding_unwritten':
        return bool((~got).any())
    if mutant == 'partial_padding_stale':                         # some probed list has a part of fewer than K rows
        K = template_k(k, wide)
        short = np.array([any(part_rows(int(L), parts, p)[1] - part_rows(int(L), parts, p)[0] < K for p in {0, parts - 1}) for L in length])
        return bool(short[probes.astype(np.int64)].any())
    if mutant == 'zero_distance_negative':
        return bool((D == 0).any())
    if mutant == 'part_last_row_dropped':
        last = np.minimum(length[case.lists[rows_got]], (part + 1) * per) - 1
        return bool((got & (pos[rows_got] == last)).any())
    if mutant == 'k20_truncated':
        if wide or k <= 20:
            return False
        key = np.where(got, case.lists[rows_got] * (parts + 1) + part, -1)
        return any(np.bincount(key[r][key[r] >= 0]).max(initial=0) > 20 for r in range(len(sample)))
    if mutant == 'merge_ties_by_probe_order':
        rank = np.full((len(sample), case.nlist), -1)
        np.put_along_axis(rank, probes.astype(np.int64), np.broadcast_to(np.arange(np_), probes.shape), 1)
        for r in range(len(sample)):
            for v in np.unique(D[r][got[r]]):
                grp = np.nonzero(dist[r] == np.float64(v))[0]     # the whole tie group, rows in id order (labels: by label)
                grp = grp[np.argsort(lab[grp])]
                m = int((D[r] == v).sum())
                by_rank = grp[np.lexsort((lab[grp], rank[r, case.lists[grp]]))]
                if not np.array_equal(grp[:m], by_rank[:m]):
                    return True
        return False
    if mutant == 'wide_threshold_tie_rejected':
        if not wide or parts != 1 or length.max() <= WAVE_BUFFER:
            return False
        if case.labels is None:
            return False                                          # ids ascend along a list: a later row never wins a tie
        for r in range(len(sample)):
            for l in probes[r]:
                rows = np.nonzero(case.lists == l)[0]
                kept, _, by_tie = wave_filter(dist[r][rows], lab[rows], k)
                if {int(lab[rows[i]]) for i in by_tie} & set(I[r].tolist()):
                    return True
        return False
    raise ValueError(mutant)


def probe_applies(case, nq, nprobe):
    """probe_tie_larger_list changes the probes iff a tie group of centroid distances reaches a query's first nprobe places."""
    dist = sq_distances(case.q[:nq], case.cent)
    srt = np.sort(dist, axis=1)
    npr = min(nprobe, case.nlist)
    inside = (np.diff(srt[:, :npr], axis=1) == 0).any() if npr > 1 else False
    straddle = npr < case.nlist and (srt[:, npr - 1] == srt[:, npr]).any()
    return bool(inside or straddle)


def encode_applies(x_res, book):
    """encode_tie_larger_code changes a code iff some (row, sub-space) has two codewords at the smallest distance."""
    m = book.shape[0]
    dist = ((x_res.reshape(len(x_res), m, 1, -1) - book[None]) ** 2).sum(-1)
    return bool(((dist == dist.min(-1, keepdims=True)).sum(-1) > 1).any())


def rerank_applies(mutant, case, k1, k):
    """As `applies`, for nafp_ivf_pqr_rerank on the first k1 candidate columns."""
    D, I = rerank_exact(case.f('q'), case.cand[:, :k1], case.f('cent'), case.f('pq'), case.f('refine'), case.codes, case.rcodes,
                        case.lists, case.n, k, case.s)
    if mutant == 'padding_unwritten':
        return bool((I < 0).any())
    if mutant == 'zero_distance_negative':
        return bool((D == 0).any())
    rec = reconstruct(case.cent, case.pq, case.refine, case.codes, case.rcodes, case.lists)
    for r in range(len(case.q)):
        c = case.cand[r, :k1].astype(np.int64)
        c = c[(c >= 0) & (c < case.n)]
        d = ((case.q[r] - rec[c]) ** 2).sum(1)
        for v in np.unique(D[r][I[r] >= 0]):
            grp = np.sort(c[d == int(v)])
            m = int((D[r] == v).sum())
            other = grp[::-1][:m] if mutant == 'tie_larger_id' else grp[len(grp) - m:]
            if not np.array_equal(grp[:m], other):
                return True
    return False
