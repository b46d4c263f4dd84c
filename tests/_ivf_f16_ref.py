"""float64 numpy restatement of the IVF-PQ search with binary16 ADC tables (include/nafp.h NAFP_IVF_LUT_F16, csrc/ivf.hip
ivf_pq_scan_f16_kernel), next to tests/_ivf_ref.py.  The residual is taken in fp32 (one rounding per component: exactly what
the kernel does), everything after it in float64; lut = 'f16' rounds each table entry once with astype(np.float16) (nearest
even, subnormals kept) and a row's distance is the float64 sum of the 64 rounded entries."""
import numpy as np

import _ivf_ref as R

BAND = 2.0 ** -20          # relative half-width of the band around a rounding midpoint in which the kernel may round the other way


def adc_tables(q, coarse, pq, pair_query, pair_list, lut):
    """(n_pairs, M, 256) tables of the pairs (q[pair_query[p]], coarse[pair_list[p]]): float64 for lut 'f32', float16 for 'f16'."""
    if lut not in ('f32', 'f16'):
        raise ValueError(lut)
    q, coarse = np.asarray(q, np.float32), np.asarray(coarse, np.float32)
    pq = np.asarray(pq, np.float64)
    M, ks, dsub = pq.shape
    rr = (q[np.asarray(pair_query)] - coarse[np.asarray(pair_list)]).astype(np.float32)         # fp32 subtraction
    assert rr.dtype == np.float32
    t = ((rr.astype(np.float64).reshape(-1, M, 1, dsub) - pq[None]) ** 2).sum(-1)
    return t.astype(np.float16) if lut == 'f16' else t


def search_with_tables(table_of, nq, codes, list_of_row, probes, k):
    """_ivf_ref.adc_search with the (M, 256) table of (query i, list l) given by table_of(i, l), summed in float64.
    Returns (D, I) padded with +inf / -1."""
    codes = np.asarray(codes).astype(np.int64)
    M = codes.shape[1]
    Ds, Is = [], []
    for i in range(nq):
        dist, ids = [], []
        for l in probes[i]:
            rows = np.nonzero(list_of_row == l)[0]
            if not len(rows):
                continue
            lut = np.asarray(table_of(i, l), np.float64)
            dist.append(lut[np.arange(M)[None, :], codes[rows]].sum(1))
            ids.append(rows)
        dist = np.concatenate(dist) if dist else np.zeros(0)
        ids = np.concatenate(ids) if ids else np.zeros(0, np.int64)
        D, I = R._topk(dist, ids, k)
        Ds.append(D); Is.append(I)
    return np.array(Ds), np.array(Is)


def adc_search_f16(q, coarse, pq, codes, list_of_row, probes, k):
    """_ivf_ref.adc_search with binary16 tables and a float64 sum."""
    return search_with_tables(lambda i, l: adc_tables(q, coarse, pq, [i], [l], 'f16')[0], len(q), codes, list_of_row, probes, k)


def near_midpoint(v):
    """Mask of the float64 values v >= 0 that lie within BAND (relative) of the midpoint between the two adjacent binary16 values
    around them: the entries whose binary16 rounding an fp32 computation of v may legitimately flip."""
    v = np.asarray(v, np.float64)
    h = v.astype(np.float16)
    hf = h.astype(np.float64)
    other = np.where(hf <= v, np.nextafter(h, np.float16(np.inf)), np.nextafter(h, np.float16(-np.inf))).astype(np.float64)
    mid = 0.5 * (hf + other)
    return np.abs(v - mid) <= BAND * np.abs(mid)


def table_inputs(x, coarse, pq, codes, list_of_row, seed):
    """Queries and (query, list) pairs of the table test: 12 noisy copies of rows, and one query that is a coarse centroid plus a
    row's decoded code (residual = codewords: entries at and next to zero); each against every second list, near and far.
    Returns (q float32, pair_query, pair_list)."""
    rng = np.random.default_rng(seed)
    n, d = x.shape
    q = (x[rng.permutation(n)[:12]] + 0.05 * rng.normal(size=(12, d)) / np.sqrt(d)).astype(np.float32)
    row = int(rng.integers(0, n))
    exact = (np.asarray(coarse, np.float32)[list_of_row[row]] + R.pq_decode(np.asarray(codes)[row:row + 1], np.asarray(pq, np.float32))[0]).astype(np.float32)
    q = np.concatenate([q, exact[None]])
    nlist = len(coarse)
    lists = np.unique(np.concatenate([np.arange(0, nlist, 2), [list_of_row[row]]]))
    pair_query = np.repeat(np.arange(len(q)), len(lists)).astype(np.int32)
    pair_list = np.tile(lists, len(q)).astype(np.int32)
    return q, pair_query, pair_list
