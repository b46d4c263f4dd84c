"""GPU: the IVF-Flat / IVF-PQ kernels and indexes (csrc/ivf.hip, eval/ivf.py) against the float64 restatement
(tests/_ivf_ref.py).  Tie tolerance as tests/test_gpu_search.py's _check_topk: an id may differ only where the float64
distances of the two ids differ by < 1e-5."""
import numpy as np
import pytest
import torch

import _ivf_ref as R

pytestmark = pytest.mark.gpu

TIE = 1e-5


def _clustered(n, d, n_centers, seed, spread=0.15):
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(n_centers, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[rng.integers(0, n_centers, size=n)] + spread * rng.normal(size=(n, d)) / np.sqrt(d)
    return x.astype(np.float32)


def _dev():
    from neural_audio_fp_amd.eval import ivf
    return ivf._Dev(torch.device('cuda', 0))


def _check_ids(I, Iw, dist_of, Dw):
    """I (GPU) vs Iw (restatement): equal, or the GPU id's float64 distance ties the restatement's at that rank."""
    bad = np.argwhere(I != Iw)
    for r, c in bad:
        assert I[r, c] >= 0 and Iw[r, c] >= 0, (r, c, I[r], Iw[r])
        assert abs(dist_of(r, I[r, c]) - Dw[r, c]) < TIE, (r, c)
    return len(bad)


@pytest.mark.parametrize('d', [64, 128, 256])
def test_assignment_and_encoding_are_arg_mins(nafp, d):
    dev = _dev()
    x = _clustered(3001, d, 37, d)
    cent = x[np.random.default_rng(1).permutation(3001)[:37]]
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(cent).cuda()
    a = dev.assign(xd, cd).cpu().numpy()
    dist = R.sqdist(x, cent)
    assert (dist[np.arange(len(x)), a] - dist.min(1) < TIE).all()
    # well separated: the choices are the restatement's
    rng = np.random.default_rng(d + 1)
    cs = rng.normal(size=(37, d))
    xs = (cs[rng.integers(0, 37, size=2000)] + 0.01 * rng.normal(size=(2000, d))).astype(np.float32)
    aw, _ = R.assign(xs, cs.astype(np.float32))
    assert np.array_equal(dev.assign(torch.from_numpy(xs).cuda(), torch.from_numpy(cs.astype(np.float32)).cuda()).cpu().numpy(), aw)
    # PQ: residual to the assigned centroid, nearest codeword per sub-space
    dsub = d // 64
    pq = (0.3 * np.random.default_rng(2).normal(size=(64, 256, dsub)) / np.sqrt(d)).astype(np.float32)
    codes = dev.pq_encode(xd, torch.from_numpy(a).cuda(), cd, torch.from_numpy(pq).cuda()).cpu().numpy()
    r = x.astype(np.float64) - cent[a]
    for m in range(64):
        dm = R.sqdist(r[:, m * dsub:(m + 1) * dsub], pq[m])
        assert (dm[np.arange(len(x)), codes[:, m]] - dm.min(1) < TIE).all(), m
    # residuals given explicitly (the training path): the same codes
    rd = dev.residuals(xd, torch.from_numpy(a).cuda(), cd)
    assert np.array_equal(dev.pq_encode(rd, None, None, torch.from_numpy(pq).cuda()).cpu().numpy(), codes)


@pytest.mark.parametrize('nlist,n', [(1, 5000), (256, 1000), (256, 100003), (400, 3_000_000), (4096, 1000), (4096, 200001)])
def test_bucketing_is_a_stable_argsort(nafp, nlist, n):
    dev = _dev()
    rng = np.random.default_rng(nlist + n)
    keys = rng.integers(0, nlist, size=n).astype(np.int32)
    if nlist > 4:
        keys[keys % 5 == 3] = 2                                   # some lists empty, some long
    off, ids = dev.bucket(torch.from_numpy(keys).cuda(), 4, n, nlist)
    off, ids = off.cpu().numpy()[0], ids.cpu().numpy()[0]
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=nlist))]))
    assert np.array_equal(ids, np.argsort(keys, kind='stable'))


def test_batched_bucketing_of_byte_keys(nafp):
    dev = _dev()
    codes = np.random.default_rng(3).integers(0, 256, size=(5001, 64)).astype(np.uint8)
    codes[:, 5] = 7                                               # one sub-space with a single bucket
    off, ids = dev.bucket(torch.from_numpy(codes).cuda(), 1, 5001, 256, 64)
    off, ids = off.cpu().numpy(), ids.cpu().numpy()
    for m in range(64):
        assert np.array_equal(off[m], np.concatenate([[0], np.cumsum(np.bincount(codes[:, m], minlength=256))]))
        assert np.array_equal(ids[m], np.argsort(codes[:, m], kind='stable'))


def test_kmeans_matches_restatement_and_splits_empty_clusters(nafp):
    from neural_audio_fp_amd.eval import ivf
    rng = np.random.default_rng(4)                                # 16 well-separated clusters, one initial point in each:
    centers = rng.normal(size=(16, 128))                          # no assignment is near a tie, so the float64 restatement
    label = rng.integers(0, 16, size=4000)                        # makes the same choices
    x = (centers[label] + 0.05 * rng.normal(size=(4000, 128))).astype(np.float32)
    init = x[[int(np.nonzero(label == c)[0][0]) for c in range(16)]]
    c, counts = ivf.kmeans(x, init, 10)
    cw, countsw = R.kmeans(x, init, 10, ivf.rng_for(ivf.DEFAULT_SEED, ivf.STREAM_COARSE_SPLIT))
    assert np.abs(c - cw).max() <= 1e-5 * np.abs(cw).max() and np.array_equal(counts, countsw)
    # duplicated initial centroids force empty clusters: the split must follow the rule (same donor draws as the restatement)
    init2 = np.concatenate([init[:8], init[:4]])
    c2, counts2 = ivf.kmeans(x, init2, 1)
    cw2, countsw2 = R.kmeans(x, init2, 1, ivf.rng_for(ivf.DEFAULT_SEED, ivf.STREAM_COARSE_SPLIT))
    assert np.array_equal(counts2, countsw2) and (counts2 > 0).all()
    assert np.abs(c2 - cw2).max() <= 1e-5 * np.abs(cw2).max()
    sign = np.where(np.arange(128) % 2 == 0, 1.0, -1.0)           # the last split's donor is not touched after it: its twin
    twin = c2[11].astype(np.float64) / (1 + sign / 1024) * (1 - sign / 1024)
    assert np.abs(c2[:11] - twin).max(1).min() < 1e-5 * np.abs(c2).max()
    # seeded training twice: bit-identical
    a1, a2 = ivf.IVFPQIndex(128, 16, 64), ivf.IVFPQIndex(128, 16, 64)
    a1.train(x); a2.train(x)
    assert torch.equal(a1.centroids, a2.centroids) and torch.equal(a1.pq_centroids, a2.pq_centroids)


def test_batched_pq_kmeans_matches_restatement(nafp):
    from neural_audio_fp_amd.eval import ivf
    dev = _dev()
    rng = np.random.default_rng(6)
    grid = np.stack(np.meshgrid(np.arange(16.0), np.arange(16.0), indexing='ij'), -1).reshape(256, 2)
    pts = grid[None] + 0.1 * rng.normal(size=(64, 256, 2))       # 256 well-separated points per sub-space
    choice = rng.integers(0, 256, size=(6000, 64))
    r = (pts[np.arange(64)[None, :], choice] + 1e-3 * rng.normal(size=(6000, 64, 2))).reshape(6000, 128).astype(np.float32)
    init = (pts + 0.05).astype(np.float32)
    rd = torch.from_numpy(r).cuda()
    cent = torch.from_numpy(init).cuda().clone()
    rs = ivf.rng_for(0, 9)
    counts = dev.kmeans(rd, cent, 256, 64, 3, rs, lambda c: (dev.pq_encode(rd, None, None, c), 1))
    cw, countsw = R.pq_kmeans(r, init.astype(np.float64), 3, ivf.rng_for(0, 9))
    assert np.array_equal(counts, countsw)
    assert np.abs(cent.cpu().numpy() - cw).max() <= 1e-5 * np.abs(cw).max()


def _build(kind, d, nlist, x, seed=1234, pieces=2):
    from neural_audio_fp_amd.eval import ivf
    idx = ivf.IVFFlatIndex(d, nlist, seed=seed) if kind == 'flat' else ivf.IVFPQIndex(d, nlist, 64, seed=seed)
    idx.train(x)
    for p in np.array_split(np.arange(len(x)), pieces):
        idx.add(x[p])
    return idx


def _probe_check(idx, q):
    P = idx.probe_device(torch.from_numpy(q).cuda()).cpu().numpy()
    Pw, dist = R.probe(q, idx.centroids.cpu().numpy(), idx.nprobe)
    for i in range(len(q)):
        if not np.array_equal(P[i], Pw[i]):
            assert np.abs(np.sort(dist[i, P[i]]) - np.sort(dist[i, Pw[i]])).max() < TIE, i
    return P


@pytest.mark.parametrize('kind', ['flat', 'pq'])
@pytest.mark.parametrize('d,nlist,k,nprobe', [(128, 50, 20, 40), (128, 50, 32, 50), (64, 50, 1, 1), (256, 50, 20, 40),
                                              (128, 400, 32, 1), (64, 400, 20, 40), (256, 12, 32, 12)])
def test_search_matches_restatement(nafp, kind, d, nlist, k, nprobe):
    x = _clustered(5000, d, 30, d + nlist)
    q = (x[np.random.default_rng(7).permutation(5000)[:131]] + 0.05 * np.random.default_rng(8).normal(size=(131, d)) / np.sqrt(d)).astype(np.float32)
    idx = _build(kind, d, nlist, x)
    idx.nprobe = nprobe
    P = _probe_check(idx, q)
    lists = idx.list_assignments().cpu().numpy()
    D, I = idx.search(q, k)
    assert D.shape == (131, k) and I.dtype == np.int64
    if kind == 'flat':
        Dw, Iw = R.ivf_flat_search(q, x, lists, P, k)
        dist_of = lambda r, i: float(((x[i].astype(np.float64) - q[r]) ** 2).sum())
    else:
        cent, pq, codes = idx.centroids.cpu().numpy(), idx.pq_centroids.cpu().numpy(), idx.codes().cpu().numpy()
        Dw, Iw = R.adc_search(q, cent, pq, codes, lists, P, k)

        def dist_of(r, i):
            res = q[r].astype(np.float64) - cent[lists[i]]
            return float(sum(((res[m * (d // 64):(m + 1) * (d // 64)] - pq[m, codes[i, m]]) ** 2).sum() for m in range(64)))
    fin = np.isfinite(Dw)
    assert np.array_equal(np.isfinite(D), fin) and ((I == -1) == ~fin).all()     # -1 / +inf padding where the lists run out
    assert (np.abs(D[fin] - Dw[fin]) <= TIE * np.maximum(1.0, np.abs(Dw[fin]))).all()
    _check_ids(I, Iw, dist_of, Dw)
    assert np.all(np.diff(np.where(fin, D, np.float32(3e38)), axis=1) >= 0)
    if nlist == 400 and nprobe == 1:
        assert (~fin).any()                                       # lists shorter than k


def test_ivf_flat_probing_every_list_is_the_exact_index(nafp):
    from neural_audio_fp_amd.eval.eval_faiss import FlatL2Index
    x = _clustered(7000, 128, 20, 11)
    q = _clustered(77, 128, 20, 12)
    idx = _build('flat', 128, 8, x)
    idx.nprobe = 8
    ex = FlatL2Index(128); ex.add(x)
    D, I = idx.search(q, 20)
    De, Ie = ex.search(q, 20)
    assert np.array_equal(I, Ie) and np.array_equal(D, De)


@pytest.mark.parametrize('kind', ['flat', 'pq'])
def test_results_are_reproducible_and_independent_of_batching(nafp, kind):
    x = _clustered(20000, 128, 40, 13)
    q = _clustered(301, 128, 40, 14)
    a = _build(kind, 128, 64, x, pieces=1)
    b = _build(kind, 128, 64, x, pieces=3)
    for idx in (a, b):
        idx.nprobe = 10
    Da, Ia = a.search(q, 20)
    Db, Ib = b.search(q, 20)
    assert np.array_equal(Ia, Ib) and Da.tobytes() == Db.tobytes()
    assert torch.equal(a.list_assignments(), b.list_assignments())
    oa, ia = a.lists(); ob, ib = b.lists()
    assert torch.equal(oa, ob) and torch.equal(ia, ib)
    if kind == 'pq':
        assert torch.equal(a.codes(), b.codes())
    parts = [a.search(q[s], 20) for s in (slice(0, 1), slice(1, 130), slice(130, 301))]
    assert np.array_equal(np.concatenate([p[1] for p in parts]), Ia)
    assert np.concatenate([p[0] for p in parts]).tobytes() == Da.tobytes()
    # k > 32 is refused like the exact index
    with pytest.raises(NotImplementedError):
        a.search(q[:2], 33)
