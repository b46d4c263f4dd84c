"""GPU: the IVFPQ-RR index (csrc/ivf.hip ivf_pq_scan_wide_kernel / ivf_refine_encode_kernel / ivf_pqr_rerank_kernel, eval/ivf.py
IVFPQRIndex, NAFP_IVFPQ_RR=1 in the evaluation) against the float64 restatement tests/_ivf_rr_ref.py.  Data, cases and the tie
rule are those of tests/test_gpu_ivf.py / test_gpu_ivf_f16.py / test_gpu_ivf_eval.py.  The two stages are held separately: the
first against the ADC restatement at k1 = k * k_factor, the second against the restatement fed the GPU's OWN first-stage ids --
gaps of 1e-7 occur at the k1 | k1 + 1 boundary, so end-to-end ids are never compared with the restatement's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _ivf_f16_ref as F
import _ivf_ref as R
import _ivf_rr_ref as RR
from test_gpu_ivf import TIE, _check_ids, _clustered, _dev, _probe_check
from test_gpu_ivf_eval import ROOT, _data, _write

pytestmark = pytest.mark.gpu

_CACHE = {}


def _build_rr(d, nlist, x, seed=1234, pieces=2):
    from neural_audio_fp_amd.eval import ivf
    idx = ivf.IVFPQRIndex(d, nlist, seed=seed)
    idx.train(x)
    for p in np.array_split(np.arange(len(x)), pieces):
        idx.add(x[p])
    return idx


def _case(d, nlist):
    """One trained index per (d, nlist) for the stage tests, with its parameters on the host."""
    if (d, nlist) not in _CACHE:
        x = _clustered(5000, d, 30, d + nlist)
        q = (x[np.random.default_rng(7).permutation(5000)[:131]] + 0.05 * np.random.default_rng(8).normal(size=(131, d)) / np.sqrt(d)).astype(np.float32)
        idx = _build_rr(d, nlist, x)
        par = dict(cent=idx.centroids.cpu().numpy(), pq=idx.pq_centroids.cpu().numpy(), refine=idx.refine_centroids.cpu().numpy(),
                   codes=idx.codes().cpu().numpy(), rcodes=idx.refine_codes().cpu().numpy(), lists=idx.list_assignments().cpu().numpy())
        _CACHE.clear()                                            # one at a time
        _CACHE[(d, nlist)] = (x, q, idx, par)
    return _CACHE[(d, nlist)]


@pytest.mark.parametrize('d', [64, 128, 256])
def test_refine_kmeans_matches_restatement(nafp, d):
    """The refine quantizer's k-means (batch = 4, 16 buckets) from an explicit initialisation: 16 well-separated points per
    sub-space, so no assignment is near a tie and the float64 restatement makes the same choices."""
    from neural_audio_fp_amd.eval import ivf
    dev = _dev()
    dr = d // 4
    rng = np.random.default_rng(d)
    pts = 2.0 * rng.normal(size=(4, 16, dr))
    choice = rng.integers(0, 16, size=(6000, 4))
    r2 = (pts[np.arange(4)[None, :], choice] + 1e-3 * rng.normal(size=(6000, 4, dr))).reshape(6000, d).astype(np.float32)
    init = (pts + 0.05).astype(np.float32)
    rd = torch.from_numpy(r2).cuda()
    cent = torch.from_numpy(init).cuda().clone()
    keys = dev.refine_encode(rd, cent, False)
    assert keys.shape == (6000, 4) and np.array_equal(keys.cpu().numpy(), choice)
    assert np.array_equal(dev.refine_encode(rd, cent, True).cpu().numpy(), RR.pack_codes(choice))
    counts = dev.kmeans(rd, cent, 16, 4, 3, ivf.rng_for(0, 9), lambda c: (dev.refine_encode(rd, c, False), 1))
    cw, countsw = RR.refine_kmeans(r2, init.astype(np.float64), 3, ivf.rng_for(0, 9))
    assert np.array_equal(counts, countsw)
    err = np.abs(cent.cpu().numpy() - cw).max()
    print(f'd = {d}: refine k-means, max |centroid - restatement| = {err:.3e} (bound {1e-5 * np.abs(cw).max():.3e})')
    assert err <= 1e-5 * np.abs(cw).max()


def test_train_with_explicit_initialisations_runs_the_refine_stage_on_the_pq_residuals(nafp, monkeypatch):
    """train(x, init=, pq_init=, refine_init=) with ONE k-means iteration per stage: the refine centroids are the means of the
    second-level residuals r - decode(encode(r)) grouped by their nearest initial codeword.  Rows are added afterwards, so the
    index's own lists and codes are the training assignment and codes (same kernels, same inputs); the grouping is the
    device's own encoding of those residuals under the initial codewords, held to be arg-mins within TIE."""
    from neural_audio_fp_amd.eval import ivf
    monkeypatch.setattr(ivf, 'COARSE_ITERS', 1)
    monkeypatch.setattr(ivf, 'PQ_ITERS', 1)
    d, n = 128, 4000
    x = _clustered(n, d, 30, 21)
    rng = np.random.default_rng(22)
    init = x[rng.permutation(n)[:16]]
    pq_init = (0.3 * rng.normal(size=(64, 256, 2)) / np.sqrt(d)).astype(np.float32)
    refine_init = (0.05 * rng.normal(size=(4, 16, 32)) / np.sqrt(d)).astype(np.float32)
    idx = ivf.IVFPQRIndex(d, 16)
    idx.train(x, init=init, pq_init=pq_init, refine_init=refine_init)
    assert idx.is_trained and tuple(idx.refine_centroids.shape) == (4, 16, 32)
    idx.add(x)
    cent, pq = idx.centroids.cpu().numpy().astype(np.float64), idx.pq_centroids.cpu().numpy()
    r = x.astype(np.float64) - cent[idx.list_assignments().cpu().numpy()]
    r2 = RR.second_residuals(r, pq, idx.codes().cpu().numpy())
    got = idx.refine_centroids.cpu().numpy()
    want = np.array(refine_init, np.float64)
    # the grouping: the device's own codes of those residuals under the initial codewords, held to be arg-mins
    dev = _dev()
    xd = torch.from_numpy(x).cuda()
    r2d = dev.pq_residuals(dev.residuals(xd, idx.list_assignments(), idx.centroids), idx.pq_centroids, idx.codes())
    assert np.abs(r2d.cpu().numpy() - r2).max() < 1e-6
    a = dev.refine_encode(r2d, torch.from_numpy(refine_init).cuda(), False).cpu().numpy()
    counts = np.zeros((4, 16), np.int64)
    for mr in range(4):
        dist = R.sqdist(r2[:, mr * 32:(mr + 1) * 32], refine_init[mr])
        assert (dist[np.arange(n), a[:, mr]] - dist.min(1) < TIE).all(), mr
        counts[mr] = np.bincount(a[:, mr], minlength=16)
        for c in range(16):
            if counts[mr, c]:
                want[mr, c] = r2[a[:, mr] == c, mr * 32:(mr + 1) * 32].mean(0)
    split_rng = ivf.rng_for(ivf.DEFAULT_SEED, ivf.STREAM_REFINE_SPLIT)       # empty clusters: the split, sub-space after sub-space
    for mr in range(4):
        if (counts[mr] == 0).any():
            R.split_empty(want[mr], counts[mr], split_rng)
    err = np.abs(got - want).max()
    print(f'refine stage of train(): max |centroid - mean of its second-level residuals| = {err:.3e}')
    assert err <= 1e-5 * max(np.abs(want).max(), np.abs(r2).max())
    other = ivf.IVFPQRIndex(d, 16)
    other.train(x, init=init, pq_init=pq_init, refine_init=refine_init)
    assert torch.equal(other.refine_centroids, idx.refine_centroids)
    # set_params takes the three tables; other refine shapes are refused
    third = ivf.IVFPQRIndex(d, 16)
    third.set_params(idx.centroids, idx.pq_centroids, idx.refine_centroids)
    third.add(x)
    assert torch.equal(third.refine_codes(), idx.refine_codes()) and torch.equal(third.codes(), idx.codes())
    with pytest.raises(NotImplementedError):
        ivf.IVFPQRIndex(d, 16, M_refine=8)
    with pytest.raises(NotImplementedError):
        ivf.IVFPQRIndex(d, 16, nbits_refine=8)
    with pytest.raises(NotImplementedError):
        idx.k_factor = 5
    assert idx.k_factor == 4


@pytest.mark.parametrize('d', [64, 128, 256])
def test_refine_codes_are_arg_mins(nafp, d):
    x, q, idx, par = _case(d, 50)
    assert par['rcodes'].shape == (5000, 2) and par['rcodes'].dtype == np.uint8
    rc = RR.unpack_codes(par['rcodes'])
    r2 = RR.second_residuals(x.astype(np.float64) - par['cent'][par['lists']].astype(np.float64), par['pq'], par['codes'])
    want = RR.refine_encode(r2, par['refine'])
    dr = d // 4
    worst = 0.0
    for mr in range(4):
        dist = R.sqdist(r2[:, mr * dr:(mr + 1) * dr], par['refine'][mr])
        gap = dist[np.arange(5000), rc[:, mr]] - dist.min(1)
        worst = max(worst, gap.max())
        assert (gap < TIE).all(), mr
    print(f'd = {d}: {(rc != want).sum()} of {rc.size} refine codes differ from the restatement (ties), worst gap {worst:.3e}')
    assert (rc != want).mean() < 0.01


CASES = [(128, 50, 20, 40), (128, 50, 32, 50), (64, 50, 20, 40), (256, 50, 32, 40), (128, 400, 32, 1), (64, 400, 20, 40), (256, 12, 20, 12)]


@pytest.mark.parametrize('lut', ['f32', 'f16'])
@pytest.mark.parametrize('d,nlist,k,nprobe', CASES)
def test_first_stage_matches_the_adc_restatement(nafp, d, nlist, k, nprobe, lut):
    """I1 / D1 at k1 = 4 k = 80 and 128 against adc_search (adc_search_f16) at that k, as test_search_matches_restatement and
    test_f16_search_matches_its_own_tables_and_the_restatement do at 20 / 32."""
    x, q, idx, par = _case(d, nlist)
    idx.nprobe, idx.lut, idx.k_factor = nprobe, lut, 4
    k1 = 4 * k
    P = _probe_check(idx, q)
    cent, pq, codes, lists = par['cent'], par['pq'], par['codes'], par['lists']
    D1, I1, D, I = idx.search_stages(q, k)
    assert D1.shape == I1.shape == (131, k1) and D.shape == I.shape == (131, k) and I1.dtype == np.int64
    if lut == 'f32':
        Dw, Iw = R.adc_search(q, cent, pq, codes, lists, P, k1)

        def dist_of(r, i):
            res = q[r].astype(np.float64) - cent[lists[i]]
            return float(sum(((res[m * (d // 64):(m + 1) * (d // 64)] - pq[m, codes[i, m]]) ** 2).sum() for m in range(64)))
    else:
        Dw, Iw = F.adc_search_f16(q, cent, pq, codes, lists, P, k1)
        npr = P.shape[1]
        T = idx.adc_tables(torch.from_numpy(q).cuda(), np.repeat(np.arange(131), npr), P.reshape(-1)).cpu().numpy()
        slot = {(i, int(l)): i * npr + j for i in range(131) for j, l in enumerate(P[i])}
        m_idx = np.arange(64)

        def dist_of(r, i):                                                   # float64 sum of the exported entries the row's codes pick
            return float(T[slot[(r, int(lists[i]))]][m_idx, codes[i]].astype(np.float64).sum())
    fin = np.isfinite(Dw)
    assert np.array_equal(np.isfinite(D1), fin) and ((I1 == -1) == ~fin).all()       # -1 / +inf padding where the lists run out
    if lut == 'f32':
        assert (np.abs(D1[fin] - Dw[fin]) <= TIE * np.maximum(1.0, np.abs(Dw[fin]))).all()
        n_bad = _check_ids(I1, Iw, dist_of, Dw)
    else:
        for r, c in np.argwhere(fin):
            dd = dist_of(r, I1[r, c])
            assert abs(D1[r, c] - dd) <= TIE * max(1.0, dd), (r, c)
        n_bad = 0
        for r, c in np.argwhere(I1 != Iw):                                   # ids: the restatement's, or a tie under that same sum
            assert I1[r, c] >= 0 and Iw[r, c] >= 0, (r, c)
            assert abs(dist_of(r, I1[r, c]) - dist_of(r, Iw[r, c])) < TIE, (r, c)
            n_bad += 1
    print(f'd {d} nlist {nlist} k1 {k1} nprobe {nprobe} {lut}: {n_bad} of {I1.size} first-stage ids differ from the restatement (ties)')
    assert np.all(np.diff(np.where(fin, D1, np.float32(3e38)), axis=1) >= 0)
    for r in range(131):
        got = I1[r][I1[r] >= 0]
        assert len(np.unique(got)) == len(got)
    if nprobe == 1:
        assert (~fin).any()                                                  # lists shorter than k1
    if nlist == 50 and lut == 'f32':
        # the first stage at k1 <= 32 is the plain IVF-PQ search of the same index, byte for byte: one contract, two selections
        from neural_audio_fp_amd.eval.ivf import IVFPQIndex
        idx.k_factor = 1
        Da, Ia, _, _ = idx.search_stages(q, k)
        Db, Ib = IVFPQIndex.search_device(idx, torch.from_numpy(q).cuda(), k)
        idx.k_factor = 4
        assert np.array_equal(Ia, Ib.cpu().numpy()) and Da.tobytes() == Db.cpu().numpy().tobytes()


@pytest.mark.parametrize('lut', ['f32', 'f16'])
@pytest.mark.parametrize('d,nlist,k,nprobe', CASES)
def test_second_stage_matches_the_restatement_on_the_gpus_own_candidates(nafp, d, nlist, k, nprobe, lut):
    x, q, idx, par = _case(d, nlist)
    idx.nprobe, idx.lut, idx.k_factor = nprobe, lut, 4
    D1, I1, D, I = idx.search_stages(q, k)
    Dw, Iw = RR.rerank(q, I1, par['cent'], par['pq'], par['refine'], par['codes'], par['rcodes'], par['lists'], k)
    rec = RR.reconstruct(np.arange(5000), par['cent'], par['pq'], par['refine'], par['codes'], par['rcodes'], par['lists'])
    dist_of = lambda r, i: float(((q[r].astype(np.float64) - rec[i]) ** 2).sum())
    fin = np.isfinite(Dw)
    assert np.array_equal(np.isfinite(D), fin) and ((I == -1) == ~fin).all()
    err = np.abs(D[fin] - Dw[fin]) / np.maximum(1.0, np.abs(Dw[fin]))
    n_bad = _check_ids(I, Iw, dist_of, Dw)
    print(f'd {d} nlist {nlist} k {k} nprobe {nprobe} {lut}: max |D - restatement| / max(1, D) = {err.max():.3e} (bound {TIE:.0e}); '
          f'{n_bad} of {I.size} ids differ (ties)')
    assert (err <= TIE).all()
    assert np.all(np.diff(np.where(fin, D, np.float32(3e38)), axis=1) >= 0)
    for r in range(131):                                                     # stage 2 chooses among stage 1, each row once
        got = I[r][I[r] >= 0]
        assert np.isin(got, I1[r]).all() and len(np.unique(got)) == len(got)
    if nprobe == 1:
        assert (~fin).any()
    # the re-rank on its own, with k_factor = 1: a re-ordering of the first stage
    idx.k_factor = 1
    Da, Ia, Dr, Ir = idx.search_stages(q, k)
    idx.k_factor = 4
    assert np.array_equal(np.sort(Ia, axis=1), np.sort(Ir, axis=1))


def _raw_rerank(idx, q, cand, k):
    from neural_audio_fp_amd import _lib
    lib = _lib.load()
    qd, cd = torch.from_numpy(q).cuda(), torch.from_numpy(np.ascontiguousarray(cand, dtype=np.int32)).cuda()
    D = torch.empty((len(q), k), dtype=torch.float32, device='cuda')
    I = torch.empty((len(q), k), dtype=torch.int32, device='cuda')
    _lib.check(lib.nafp_ivf_pqr_rerank(_lib.ptr(qd), len(q), idx.d, _lib.ptr(cd), cand.shape[1], _lib.ptr(idx.centroids),
                                       _lib.ptr(idx.list_assignments()), _lib.ptr(idx.pq_centroids), idx.M, _lib.ptr(idx.codes()),
                                       _lib.ptr(idx.refine_centroids), 4, 4, _lib.ptr(idx.refine_codes()), idx.ntotal, k, _lib.ptr(D),
                                       _lib.ptr(I), _lib.current_stream()), 'ivf_pqr_rerank')
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy()


def test_rerank_entry_point_with_arbitrary_candidates(nafp):
    """nafp_ivf_pqr_rerank as a building block: candidates that no search produced (random rows, -1 holes, ids past the table)."""
    x, q, idx, par = _case(128, 50)
    rng = np.random.default_rng(31)
    cand = rng.integers(0, 5000, size=(131, 100))
    for r in range(131):
        cand[r] = rng.permutation(5000)[:100]
    cand[:, 7::9] = -1
    cand[3, :] = -1
    cand[5, 95:] = 5000 + np.arange(5)                                       # outside the table: ignored
    D, I = _raw_rerank(idx, q, cand, 32)
    Dw, Iw = RR.rerank(q, np.where(cand < 5000, cand, -1), par['cent'], par['pq'], par['refine'], par['codes'], par['rcodes'], par['lists'], 32)
    rec = RR.reconstruct(np.arange(5000), par['cent'], par['pq'], par['refine'], par['codes'], par['rcodes'], par['lists'])
    fin = np.isfinite(Dw)
    assert np.array_equal(np.isfinite(D), fin) and ((I == -1) == ~fin).all() and (I[3] == -1).all()
    assert (np.abs(D[fin] - Dw[fin]) <= TIE * np.maximum(1.0, Dw[fin])).all()
    _check_ids(I, Iw, lambda r, i: float(((q[r].astype(np.float64) - rec[i]) ** 2).sum()), Dw)


def test_results_are_reproducible_and_independent_of_batching(nafp):
    x, q = _clustered(20000, 128, 40, 13), _clustered(301, 128, 40, 14)
    a = _build_rr(128, 64, x, pieces=1)
    b = _build_rr(128, 64, x, pieces=3)
    assert torch.equal(a.refine_centroids, b.refine_centroids) and torch.equal(a.refine_codes(), b.refine_codes())
    assert torch.equal(a.codes(), b.codes()) and torch.equal(a.list_assignments(), b.list_assignments())
    same = lambda s, t: all(u.tobytes() == v.tobytes() for u, v in zip(s, t))
    for lut in ('f32', 'f16'):
        for k in (20, 32):
            for idx in (a, b):
                idx.nprobe, idx.lut = 10, lut
            ra = a.search_stages(q, k)
            assert same(ra, b.search_stages(q, k)), (lut, k)
            assert same(ra, a.search_stages(q, k)) and same(ra, a.search_stages(q, k)), (lut, k)
            parts = [a.search_stages(q[s], k) for s in (slice(0, 1), slice(1, 130), slice(130, 301))]
            assert same(ra, [np.concatenate([p[j] for p in parts]) for j in range(4)]), (lut, k)
            D, I = a.search(q, k)
            assert D.tobytes() == ra[2].tobytes() and np.array_equal(I, ra[3])
    with pytest.raises(NotImplementedError):
        a.search(q[:2], 33)


def test_the_ivfpq_path_is_untouched(nafp):
    """An IVFPQRIndex and an IVFPQIndex trained with one seed share centroids, PQ centroids and codes bit for bit (the refine
    stage draws from its own two random streams), and IVFPQIndex keeps refusing k > 32."""
    from neural_audio_fp_amd.eval import ivf
    x = _clustered(20000, 128, 40, 13)
    q = _clustered(64, 128, 40, 14)
    rr = _build_rr(128, 64, x, seed=77)
    pq = ivf.IVFPQIndex(128, 64, 64, seed=77)
    pq.train(x)
    for p in np.array_split(np.arange(len(x)), 2):
        pq.add(x[p])
    assert torch.equal(rr.centroids, pq.centroids) and torch.equal(rr.pq_centroids, pq.pq_centroids) and torch.equal(rr.codes(), pq.codes())
    assert torch.equal(rr.list_assignments(), pq.list_assignments())
    assert np.array_equal(rr.reconstruct_n(5, 3), x[5:8])                    # the true rows, as the evaluation needs
    pq.nprobe = rr.nprobe = 10
    rr.k_factor = 1
    D1, I1, _, _ = rr.search_stages(q, 20)
    Dp, Ip = pq.search(q, 20)
    assert np.array_equal(I1, Ip) and D1.tobytes() == Dp.tobytes()
    with pytest.raises(NotImplementedError):
        pq.search(q[:2], 33)
    lib = nafp._lib.load()
    assert lib.nafp_ivf_search_workspace_bytes(64, 64, 10, 33, 1) == -1


def _eval_setup(tmp_path, monkeypatch, rr=True):
    monkeypatch.setenv('NAFP_APPROX_INDEX', '1')
    if rr:
        monkeypatch.setenv('NAFP_IVFPQ_RR', '1')
    else:
        monkeypatch.delenv('NAFP_IVFPQ_RR', raising=False)
    dummy, db, query = _data(2)
    out = str(tmp_path) + '/'
    _write(out, {'query': query, 'db': db, 'dummy_db': dummy})
    test_ids = np.sort(np.random.default_rng(3).choice(1000 - 5, size=150, replace=False))
    np.save(out + 'ids.npy', test_ids)
    return dummy, db, query, out, test_ids


def test_the_rerank_changes_the_results_and_eval_faiss_uses_it(nafp, monkeypatch, tmp_path):
    from neural_audio_fp_amd.eval import eval_faiss as E
    from neural_audio_fp_amd.eval.ivf import IVFPQRIndex
    dummy, db, query, out, test_ids = _eval_setup(tmp_path, monkeypatch)
    lens = (1, 3, 5)
    rates = E.eval_faiss(out, index_type='ivfpq-rr', test_ids=out + 'ids.npy', test_seq_len='1 3 5')
    used = json.load(open(out + 'index_used.json'))
    assert used['substituted'] is False and used['index_type_requested'] == 'ivfpq-rr'
    assert used['index_type_used'] == 'IVFPQR (HIP; nlist 256, M 64, nbits 8, refine 4 x 4 bits, k_factor 4, nprobe 40)'
    raw = np.load(out + 'raw_score.npy')
    idx = E.get_index('ivfpq-rr', dummy, dummy.shape)
    assert isinstance(idx, IVFPQRIndex) and (idx.nlist, idx.M, idx.nbits, idx.nprobe, idx.k_factor, idx.lut) == (256, 64, 8, 40, 4, 'f32')
    idx.add(dummy); idx.add(db)
    D1, I1, D, I = idx.search_stages(query, 20)
    # the feature is live: the re-ranked top-20 set is not the first stage's first 20 (float64 sketch of the contract: 56 %)
    differs = np.mean([set(I[r]) != set(I1[r, :20]) for r in range(len(query))])
    top1 = np.mean(I[:, 0] != I1[:, 0])
    print(f're-ranked top-20 set differs from the first stage\'s first 20 for {100 * differs:.1f} % of the queries, top-1 for {100 * top1:.1f} %')
    assert differs >= 0.25
    table = np.concatenate([dummy, db])
    want = R.evaluate_from_ids(query, table, len(dummy), test_ids, lens, I, 20)
    assert np.array_equal(raw, np.concatenate(want[:4], axis=1))
    # hit rates against the restatement's own two-stage search with the same trained parameters
    P = idx.probe_device(torch.from_numpy(query).cuda()).cpu().numpy()
    _, _, _, Iw = RR.search(query, idx.centroids.cpu().numpy(), idx.pq_centroids.cpu().numpy(), idx.refine_centroids.cpu().numpy(),
                            idx.codes().cpu().numpy(), idx.refine_codes().cpu().numpy(), idx.list_assignments().cpu().numpy(), P, 20, 4)
    bound = R.evaluate_from_ids(query, table, len(dummy), test_ids, lens, Iw, 20)
    for got, ref in zip(rates, bound[:4]):
        print('hit rates', got, 'restatement', 100. * ref.mean(0))
        assert (got >= 100. * ref.mean(0) - 2.0).all(), (got, 100. * ref.mean(0))
    assert 5 < rates[0][0] < 100
    # the table precision applies to the first stage
    monkeypatch.setenv('NAFP_IVFPQ_LUT', 'f16')
    small = dummy[:3000]
    h = E.get_index('IVFPQ-RR', small, small.shape)
    assert isinstance(h, IVFPQRIndex) and h.lut == 'f16'
    assert h.index_description == 'IVFPQR (HIP; nlist 256, M 64, nbits 8, refine 4 x 4 bits, k_factor 4, nprobe 40, fp16 tables)'


def test_without_the_second_variable_the_exact_search_serves_ivfpq_rr(nafp, monkeypatch, tmp_path, capsys):
    from neural_audio_fp_amd.eval import eval_faiss as E
    dummy, db, query, out, test_ids = _eval_setup(tmp_path, monkeypatch, rr=False)
    small = dummy[:3000]
    idx = E.get_index('ivfpq-rr', small, small.shape)
    assert type(idx) is E.FlatL2Index and 'not built here' in capsys.readouterr().err
    monkeypatch.delenv('NAFP_APPROX_INDEX')
    monkeypatch.setenv('NAFP_IVFPQ_RR', '1')                                  # the second variable alone opts into nothing
    assert type(E.get_index('ivfpq-rr', small, small.shape)) is E.FlatL2Index
    E.eval_faiss(out, index_type='ivfpq-rr', test_ids=out + 'ids.npy', test_seq_len='1 3')
    used = json.load(open(out + 'index_used.json'))
    assert used['substituted'] is True and used['index_type_used'].startswith('L2')


def test_run_evaluate_records_ivfpq_rr(nafp, tmp_path):
    import yaml
    dummy, db, query = _data(4, n_dummy=5000, n_db=300)
    work = tmp_path / 'work'
    (work / 'config').mkdir(parents=True)
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'config', 'default.yaml')))
    cfg['DIR'].update({'OUTPUT_ROOT_DIR': str(work) + '/logs/emb/', 'LOG_ROOT_DIR': str(work) + '/logs/'})
    yaml.safe_dump(cfg, open(work / 'config' / 'tiny.yaml', 'w'))
    emb = work / 'logs' / 'emb' / 'EXP' / '1'
    emb.mkdir(parents=True)
    _write(str(emb) + '/', {'query': query, 'db': db, 'dummy_db': dummy})
    np.save(work / 'ids.npy', np.arange(0, 290))
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), 'evaluate', 'EXP', '1', '-c', 'tiny', '-i', 'ivfpq-rr', '-t', str(work / 'ids.npy'),
           '--test_seq_len', '1 3']
    env = dict(os.environ, PYTHONPATH=ROOT, NAFP_APPROX_INDEX='1', NAFP_IVFPQ_RR='1')
    r = subprocess.run(cmd, cwd=work, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    used = json.load(open(emb / 'index_used.json'))
    assert used['substituted'] is False
    assert used['index_type_used'] == 'IVFPQR (HIP; nlist 256, M 64, nbits 8, refine 4 x 4 bits, k_factor 4, nprobe 40)'
    assert np.load(emb / 'raw_score.npy').shape == (290, 8)
    env.pop('NAFP_IVFPQ_RR')                                                  # unset: served by the exact search, as before
    r = subprocess.run(cmd, cwd=work, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    used = json.load(open(emb / 'index_used.json'))
    assert used['substituted'] is True and 'not built here' in r.stderr


# ---- the first stage where the filter really filters -------------------------------------------------------------------------
# A wave of the wide scan takes every row until it holds 240 candidates; only then does it prune to its K best and reject rows by a
# threshold.  The cases above have a few hundred rows per (list, part), i.e. under 240 per wave: nothing is ever pruned or rejected
# there.  Here: 20 000 rows in 4 lists and 512 queries x 4 probes = 2 048 pairs, for which the library scans every list in ONE
# part, so a wave sees a quarter of ~5 000 rows.  Two row orders: 'shuffled', and 'late' -- rows sorted by falling distance to the
# point all queries lie around, so that in list (= id) order nearly every row beats what came before: the threshold is beaten
# again and again and a wave prunes every hundred-odd rows.  _simulated_prunes replays one wave's filter in numpy to hold that.
PRUNE_N, PRUNE_NLIST, PRUNE_NQ, WAVE_BUFFER = 20000, 4, 512, 240
_PRUNE = {}


def _prune_case(order, lut):
    if (order,) not in _PRUNE:
        _PRUNE.clear()
        d = 128
        x = _clustered(PRUNE_N, d, 40, 41)
        rng = np.random.default_rng(42)
        centre = x[:50].mean(0)
        if order == 'late':
            x = x[np.argsort(-((x - centre) ** 2).sum(1), kind='stable')]
        q = (centre + 0.15 * rng.normal(size=(PRUNE_NQ, d)) / np.sqrt(d)).astype(np.float32)
        idx = _build_rr(d, PRUNE_NLIST, x)
        idx.nprobe = PRUNE_NLIST
        par = dict(cent=idx.centroids.cpu().numpy(), pq=idx.pq_centroids.cpu().numpy(), codes=idx.codes().cpu().numpy(),
                   lists=idx.list_assignments().cpu().numpy())
        _PRUNE[(order,)] = (x, q, idx, par)
    x, q, idx, par = _PRUNE[(order,)]
    if (order, lut) not in _PRUNE:
        idx.lut = lut
        P = _probe_check(idx, q)
        fn = R.adc_search if lut == 'f32' else F.adc_search_f16
        _PRUNE[(order, lut)] = (P,) + fn(q, par['cent'], par['pq'], par['codes'], par['lists'], P, 128)
    return (x, q, idx, par) + _PRUNE[(order, lut)]


def _simulated_prunes(dist, K):
    """Prunes of each of the 4 waves over one list's float64 distances in list order (one part): rows 64 w .. 64 w + 63 of every
    256 are wave w's; a row is appended when it beats the K-th best at the last prune; a prune when an append would pass 240."""
    out = []
    for w in range(4):
        held, thr, n = np.zeros(0), np.inf, 0
        for rb in range(0, len(dist), 256):
            rows = dist[rb + 64 * w: rb + 64 * w + 64]
            take = rows[rows < thr]
            if len(take) and len(held) + len(take) > WAVE_BUFFER:
                held = np.sort(held)[:K]
                thr, n = held[-1], n + 1
            held = np.concatenate([held, take])
        out.append(n)
    return out


@pytest.mark.parametrize('lut', ['f32', 'f16'])
@pytest.mark.parametrize('order', ['shuffled', 'late'])
def test_first_stage_where_every_wave_prunes_and_rejects(nafp, order, lut):
    x, q, idx, par, P, Dw, Iw = _prune_case(order, lut)
    cent, pq, codes, lists = par['cent'], par['pq'], par['codes'], par['lists']
    d = 128
    # the regime: one part per list (2 048 pairs), every list far beyond 4 wave buffers
    sizes = np.bincount(lists, minlength=PRUNE_NLIST)
    assert PRUNE_NQ * P.shape[1] >= 2048 and sizes.min() >= 8 * WAVE_BUFFER, sizes
    l0 = int(np.argmax(sizes))                                               # every list is probed: the longest one
    rows0 = np.nonzero(lists == l0)[0]
    res0 = q[0].astype(np.float64) - cent[l0]
    lut0 = ((res0.reshape(64, 1, d // 64) - pq.astype(np.float64)) ** 2).sum(-1)
    dist0 = lut0[np.arange(64)[None, :], codes[rows0].astype(np.int64)].sum(1)
    sims = {K: _simulated_prunes(dist0, K) for K in (5, 20, 80, 128)}
    print(f'{order} {lut}: list sizes {sizes.tolist()}; prunes per wave of (query 0, list {l0}, {len(rows0)} rows) by K: {sims}')
    assert all(min(v) >= 1 for v in sims.values())
    if order == 'late':
        assert min(sims[80]) >= 4 and min(sims[128]) >= 4 and min(sims[20]) >= 3, sims
    if lut == 'f32':
        def dist_of(r, i):
            res = q[r].astype(np.float64) - cent[lists[i]]
            return float(sum(((res[m * (d // 64):(m + 1) * (d // 64)] - pq[m, codes[i, m]]) ** 2).sum() for m in range(64)))
    else:
        npr = P.shape[1]
        T = idx.adc_tables(torch.from_numpy(q).cuda(), np.repeat(np.arange(PRUNE_NQ), npr), P.reshape(-1)).cpu().numpy()
        slot = {(i, int(l)): i * npr + j for i in range(PRUNE_NQ) for j, l in enumerate(P[i])}
        m_idx = np.arange(64)

        def dist_of(r, i):
            return float(T[slot[(r, int(lists[i]))]][m_idx, codes[i]].astype(np.float64).sum())
        # binary16 tables: the restatement's tables and the kernel's may differ by one binary16 ulp in entries near a rounding
        # midpoint (test_tables_match_restatement holds exactly that), and with ~5 000 rows per list two rows do lie closer than
        # such an ulp (~1e-5 here).  So the ids are held to the exact float64 search over the kernel's OWN exported tables, and the
        # distances to adc_search_f16's rank by rank within the rounding of 64 entries <= 4 (test_gpu_ivf_f16's bound)
        Dx, Ix = F.search_with_tables(lambda i, l: T[slot[(i, int(l))]], PRUNE_NQ, codes, lists, P, 128)
    idx.lut = lut
    for k, kf in ((20, 4), (32, 4), (20, 1), (5, 1)):                        # K = 80, 128 and, with k_factor 1, 20 and 5
        idx.k_factor = kf
        k1 = k * kf
        D1, I1, D, I = idx.search_stages(q, k)
        idx.k_factor = 4
        assert D1.shape == (PRUNE_NQ, k1) and np.isfinite(D1).all() and (I1 >= 0).all()
        Dk, Ik = (Dw[:, :k1], Iw[:, :k1]) if lut == 'f32' else (Dx[:, :k1], Ix[:, :k1])      # the first k1 of 128: the top k1
        n_bad = 0
        for r, c in np.argwhere(I1 != Ik):                                   # ids: the reference's, or a tie under the same sum
            assert abs(dist_of(r, I1[r, c]) - dist_of(r, Ik[r, c])) < TIE, (k1, r, c)
            n_bad += 1
        err = np.abs(D1 - Dk) / np.maximum(1.0, np.abs(Dk))
        note = ''
        if lut == 'f16':
            assert (np.abs(D1 - Dw[:, :k1]) <= 64 * 2.0 ** -11 * 4).all()
            note = f'; {(I1 != Iw[:, :k1]).sum()} differ from adc_search_f16 (its tables are not the kernel\'s to the last ulp)'
        print(f'{order} {lut} K {k1}: {n_bad} of {I1.size} ids differ from the reference (ties){note}; max distance error {err.max():.3e} (bound {TIE:.0e})')
        assert (err <= TIE).all()
        assert np.all(np.diff(D1, axis=1) >= 0)
        assert all(len(np.unique(I1[r])) == k1 for r in range(PRUNE_NQ))
        assert all(np.isin(I[r], I1[r]).all() for r in range(PRUNE_NQ))


def test_train_is_the_refine_kmeans_building_block_on_the_pq_stage_residuals(nafp):
    """IVFPQRIndex.train with all its iterations against the building block test_refine_kmeans_matches_restatement holds to the
    restatement: the refine centroids are, bit for bit, dev.kmeans over the second-level residuals of the training rows from the
    same initialisation and split stream.  The rows are added afterwards, so the index's lists and codes are the training ones."""
    from neural_audio_fp_amd.eval import ivf
    d, n = 64, 6000
    x = _clustered(n, d, 30, 51)
    rng = np.random.default_rng(52)
    refine_init = (0.05 * rng.normal(size=(4, 16, 16)) / np.sqrt(d)).astype(np.float32)
    idx = ivf.IVFPQRIndex(d, 16, seed=5)
    idx.train(x, refine_init=refine_init)
    idx.add(x)
    dev = _dev()
    xd = torch.from_numpy(x).cuda()
    r2 = dev.pq_residuals(dev.residuals(xd, idx.list_assignments(), idx.centroids), idx.pq_centroids, idx.codes())
    cent = torch.from_numpy(refine_init).cuda().clone()
    dev.kmeans(r2, cent, 16, 4, ivf.PQ_ITERS, ivf.rng_for(5, ivf.STREAM_REFINE_SPLIT), lambda c: (dev.refine_encode(r2, c, False), 1))
    assert torch.equal(cent, idx.refine_centroids)
    assert not torch.equal(cent, torch.from_numpy(refine_init).cuda())
    # the seeded pick: 16 rows of those residuals drawn from the refine stream
    seeded = ivf.IVFPQRIndex(d, 16, seed=5)
    seeded.train(x)
    pick = torch.from_numpy(ivf.rng_for(5, ivf.STREAM_REFINE).permutation(n)[:16]).cuda()
    cent2 = r2[pick].reshape(16, 4, 16).transpose(0, 1).contiguous()
    dev.kmeans(r2, cent2, 16, 4, ivf.PQ_ITERS, ivf.rng_for(5, ivf.STREAM_REFINE_SPLIT), lambda c: (dev.refine_encode(r2, c, False), 1))
    assert torch.equal(seeded.centroids, idx.centroids) and torch.equal(seeded.pq_centroids, idx.pq_centroids)
    assert torch.equal(cent2, seeded.refine_centroids)
