"""float64 numpy restatement of the IVFPQ-RR contract (faiss's CPU IndexIVFPQR; eval/ivf.py IVFPQRIndex, include/nafp.h
"IVFPQ-RR"), built on tests/_ivf_ref.py: an IVF-PQ index plus a refine product quantizer (4 sub-spaces x 16 codewords) of the
second-level residuals x - centroid[list] - pq_decode(code), stored as two nibble-packed bytes per row, and a search in two
stages -- the IVF-PQ ADC search for k * k_factor candidates, then those re-ranked by the distance to the refined reconstruction
centroid[list] + pq_decode(code) + refine_decode(rcode).  Ties everywhere: the smaller id (codeword, row) first."""
import numpy as np

import _ivf_ref as R

M_REFINE = 4
KS_REFINE = 16


def pack_codes(c):
    """(n, 4) codes 0..15 -> (n, 2) bytes: byte0 = c0 | c1 << 4, byte1 = c2 | c3 << 4."""
    c = np.asarray(c).astype(np.uint8)
    assert c.ndim == 2 and c.shape[1] == M_REFINE and (c < KS_REFINE).all()
    return np.stack([c[:, 0] | (c[:, 1] << 4), c[:, 2] | (c[:, 3] << 4)], 1).astype(np.uint8)


def unpack_codes(b):
    """(n, 2) bytes -> (n, 4) codes."""
    b = np.asarray(b).astype(np.uint8)
    assert b.ndim == 2 and b.shape[1] == 2
    return np.stack([b[:, 0] & 15, b[:, 0] >> 4, b[:, 1] & 15, b[:, 1] >> 4], 1).astype(np.uint8)


def second_residuals(r, pq, codes=None):
    """r - decode(codes) (codes: the PQ codes of r, encoded here when not given)."""
    r = np.asarray(r, np.float64)
    pq = np.asarray(pq, np.float64)
    codes = R.pq_encode(r, pq) if codes is None else np.asarray(codes)
    return r - R.pq_decode(codes.astype(np.int64), pq)


def refine_kmeans(r2, init, niter, rng):
    """The 4 refine sub-quantizers trained side by side: _ivf_ref.pq_kmeans with init (4, 16, d / 4)."""
    init = np.asarray(init, np.float64)
    assert init.shape[:2] == (M_REFINE, KS_REFINE)
    return R.pq_kmeans(r2, init, niter, rng)


def refine_encode(r2, refine):
    """(n, 4) refine codes of the rows r2 (arg-min per sub-space; ties: the smaller code)."""
    return R.pq_encode(r2, np.asarray(refine, np.float64))


def reconstruct(ids, coarse, pq, refine, codes, rcodes, list_of_row):
    """centroid[list] + pq_decode(code) + refine_decode(rcode) of the rows ids, float64.  rcodes: (n, 2) packed bytes."""
    ids = np.asarray(ids, np.int64)
    coarse, pq, refine = (np.asarray(a, np.float64) for a in (coarse, pq, refine))
    return (coarse[np.asarray(list_of_row)[ids]] + R.pq_decode(np.asarray(codes)[ids].astype(np.int64), pq)
            + R.pq_decode(unpack_codes(np.asarray(rcodes)[ids]).astype(np.int64), refine))


def rerank(q, I1, coarse, pq, refine, codes, rcodes, list_of_row, k):
    """Stage 2: the candidates I1 (nq, k1; -1 = none) by |q - reconstruction|^2, the k smallest by (distance, id), +inf / -1
    padding.  Returns (D, I)."""
    q = np.asarray(q, np.float64)
    Ds, Is = [], []
    for i in range(len(q)):
        ids = np.asarray(I1[i], np.int64)
        ids = ids[ids >= 0]
        rec = reconstruct(ids, coarse, pq, refine, codes, rcodes, list_of_row)
        D, I = R._topk(((q[i] - rec) ** 2).sum(1), ids, k)
        Ds.append(D); Is.append(I)
    return np.array(Ds), np.array(Is)


def search(q, coarse, pq, refine, codes, rcodes, list_of_row, probes, k, k_factor=4):
    """Both stages: (D1, I1, D, I)."""
    D1, I1 = R.adc_search(q, coarse, pq, codes, list_of_row, probes, k * k_factor)
    D, I = rerank(q, I1, coarse, pq, refine, codes, rcodes, list_of_row, k)
    return D1, I1, D, I


def train_and_add(x, xt, coarse_init, pq_init, refine_init, coarse_iters, pq_iters, rngs):
    """A small end-to-end index in float64 from explicit initialisations: coarse k-means on xt, PQ on the residuals of xt, refine on
    their second-level residuals; then the codes of the rows x.  rngs: (coarse split, PQ split, refine split) generators.
    Returns dict(coarse, pq, refine, lists, codes, rcodes (packed))."""
    coarse, _ = R.kmeans(xt, coarse_init, coarse_iters, rngs[0])
    at, _ = R.assign(xt, coarse)
    r = np.asarray(xt, np.float64) - coarse[at]
    pq, _ = R.pq_kmeans(r, np.asarray(pq_init, np.float64), pq_iters, rngs[1])
    refine, _ = refine_kmeans(second_residuals(r, pq), refine_init, pq_iters, rngs[2])
    lists, _ = R.assign(x, coarse)
    rx = np.asarray(x, np.float64) - coarse[lists]
    codes = R.pq_encode(rx, pq)
    rcodes = pack_codes(refine_encode(second_residuals(rx, pq, codes), refine))
    return dict(coarse=coarse, pq=pq, refine=refine, lists=lists, codes=codes, rcodes=rcodes)
