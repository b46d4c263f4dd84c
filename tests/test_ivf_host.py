"""CPU: the float64 restatement of the IVF contract (tests/_ivf_ref.py) on its own, and the argument checks of the IVF entry
points of the C ABI (include/nafp.h "Approximate indexes"), which return before any GPU call."""
import ctypes

import numpy as np
import pytest

import _ivf_ref as R
from oracle import search as S

NULL = None
FAKE = ctypes.c_void_p(4096)          # a non-null pointer that is never dereferenced: every check below fails before use


def test_ivf_flat_with_every_list_probed_is_the_exact_search():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(500, 16))
    q = rng.normal(size=(23, 16))
    cent = x[rng.permutation(500)[:7]]
    lists, _ = R.assign(x, cent)
    probes, _ = R.probe(q, cent, 7)
    D, I = R.ivf_flat_search(q, x, lists, probes, 20)
    Dw, Iw = S.flat_l2_search(q, x, 20)
    assert np.array_equal(I, Iw) and np.allclose(D, Dw)
    # one probe: only rows of the nearest list; fewer rows than k -> -1 / +inf
    probes1, _ = R.probe(q, cent, 1)
    D1, I1 = R.ivf_flat_search(q, x, lists, probes1, 300)
    for i in range(len(q)):
        n_in = (lists == probes1[i, 0]).sum()
        assert (lists[I1[i, :n_in]] == probes1[i, 0]).all() and (I1[i, n_in:] == -1).all() and np.isinf(D1[i, n_in:]).all()


def test_pq_with_one_codeword_per_distinct_value_reconstructs_exactly():
    rng = np.random.default_rng(1)
    vals = np.arange(256, dtype=np.float64) * 0.25 - 32.0          # 256 distinct values per sub-space (dsub = 1)
    r = rng.choice(vals, size=(300, 64))
    pq = np.repeat(vals[None, :, None], 64, axis=0)                 # (M, 256, 1): codeword j = value j
    codes = R.pq_encode(r, pq)
    assert np.array_equal(R.pq_decode(codes, pq), r)
    # ADC distance of a query that is a stored row (zero coarse centroid) is 0 for that row
    D, I = R.adc_search(r[:3], np.zeros((1, 64)), pq, codes, np.zeros(300, np.int64), np.zeros((3, 1), np.int64), 1)
    assert np.array_equal(I[:, 0], [0, 1, 2]) or (D[:, 0] == 0).all()


def test_kmeans_objective_never_increases_and_split_fills_empty_clusters():
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.normal(size=(200, 8)) + 6 * c for c in rng.normal(size=(5, 8))])
    hist = []
    init = x[rng.permutation(len(x))[:12]]
    cent, counts = R.kmeans(x, init, 10, np.random.default_rng(3), history=hist)
    assert all(b <= a * (1 + 1e-12) for a, b in zip(hist, hist[1:]))
    assert counts.sum() == len(x)
    # duplicated initial centroids: the duplicate is empty after the first assignment and gets split from a donor
    init2 = np.concatenate([x[:3], x[:1]])
    cent2, counts2 = R.kmeans(x, init2, 1, np.random.default_rng(4))
    assert (counts2 > 0).all() and counts2.sum() == len(x)
    sign = np.where(np.arange(8) % 2 == 0, 1.0, -1.0)
    twin = cent2[3] / (1 + sign / 1024) * (1 - sign / 1024)          # the donor's centroid after the split
    assert min(np.abs(cent2[:3] - twin).max(1)) < 1e-12


def test_split_rule():
    cent = np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [4.0, 5.0, 6.0]])
    counts = np.array([1, 0, 9])                                    # only cluster 2 can donate (size - 1 > 0)
    R.split_empty(cent, counts, np.random.default_rng(0))
    e = 1.0 / 1024
    assert np.allclose(cent[1], [4 * (1 + e), 5 * (1 - e), 6 * (1 + e)])
    assert np.allclose(cent[2], [4 * (1 - e), 5 * (1 + e), 6 * (1 - e)])
    assert list(counts) == [1, 4, 5]


def test_ivf_entry_points_check_arguments_without_gpu(nafp):
    lib = nafp._lib.load()
    INV, UNS = 1, 2
    # workspace queries
    assert lib.nafp_ivf_bucket_workspace_bytes(1000, 400, 1) > 0
    assert lib.nafp_ivf_bucket_workspace_bytes(-1, 400, 1) == -1 and lib.nafp_ivf_bucket_workspace_bytes(10, 16385, 1) == -1
    assert lib.nafp_ivf_search_workspace_bytes(100, 256, 40, 20, 1) > 0 and lib.nafp_ivf_search_workspace_bytes(100, 400, 40, 32, 0) > 0
    assert lib.nafp_ivf_search_workspace_bytes(100, 256, 40, 33, 1) == -1          # k > 32
    assert lib.nafp_ivf_search_workspace_bytes(100, 256, 129, 20, 0) == -1         # nprobe > 128
    assert lib.nafp_ivf_flat_rows_bound(1000, 10) == 1630 and lib.nafp_ivf_flat_rows_bound(-1, 10) == -1
    # null pointers -> INVALID_ARG
    assert lib.nafp_ivf_bucket(NULL, 4, 10, 4, 1, NULL, NULL, NULL, 0, NULL) == INV
    assert lib.nafp_ivf_kmeans_update(NULL, 10, 128, 1, NULL, NULL, 4, NULL, NULL, NULL) == INV
    assert lib.nafp_ivf_residuals(NULL, 10, 128, NULL, NULL, NULL, NULL) == INV
    assert lib.nafp_ivf_pq_encode(NULL, 10, 128, NULL, NULL, NULL, 64, NULL, NULL) == INV
    assert lib.nafp_ivf_probe(NULL, 10, NULL, 8, 128, 4, NULL, NULL) == INV
    assert lib.nafp_ivf_flat_lists(NULL, 10, 128, NULL, NULL, 4, NULL, NULL, NULL, NULL, NULL) == INV
    assert lib.nafp_ivf_pq_lists(NULL, 10, 64, NULL, NULL, NULL) == INV
    assert lib.nafp_ivf_flat_search(NULL, 1, NULL, 8, 128, 4, NULL, NULL, NULL, NULL, 20, NULL, NULL, NULL, 0, NULL) == INV
    assert lib.nafp_ivf_pq_search(NULL, 1, NULL, 8, 128, 4, NULL, 64, NULL, NULL, NULL, 20, NULL, NULL, NULL, 0, NULL) == INV
    # pq_encode: assign and coarse come together
    assert lib.nafp_ivf_pq_encode(FAKE, 10, 128, FAKE, NULL, FAKE, 64, FAKE, NULL) == INV
    # bad d, M, k, nprobe -> UNSUPPORTED (non-null pointers: nothing is launched)
    P = [FAKE] * 4
    assert lib.nafp_ivf_probe(FAKE, 10, FAKE, 8, 96, 4, FAKE, NULL) == UNS
    assert lib.nafp_ivf_probe(FAKE, 10, FAKE, 256, 128, 129, FAKE, NULL) == UNS
    assert lib.nafp_ivf_residuals(FAKE, 10, 100, FAKE, FAKE, FAKE, NULL) == UNS
    assert lib.nafp_ivf_pq_encode(FAKE, 10, 96, NULL, NULL, FAKE, 64, FAKE, NULL) == UNS
    assert lib.nafp_ivf_pq_encode(FAKE, 10, 128, NULL, NULL, FAKE, 32, FAKE, NULL) == UNS
    assert lib.nafp_ivf_pq_lists(FAKE, 10, 32, FAKE, FAKE, NULL) == UNS
    assert lib.nafp_ivf_bucket(FAKE, 2, 10, 4, 1, FAKE, FAKE, FAKE, 1 << 20, NULL) == UNS
    assert lib.nafp_ivf_flat_lists(FAKE, 10, 32, FAKE, FAKE, 4, *P, NULL) == UNS
    for dim, k, nprobe in ((96, 20, 4), (128, 33, 4), (128, 20, 129)):
        assert lib.nafp_ivf_flat_search(FAKE, 5, FAKE, 256, dim, nprobe, *P, k, FAKE, FAKE, FAKE, 1 << 30, NULL) == UNS
        assert lib.nafp_ivf_pq_search(FAKE, 5, FAKE, 256, dim, nprobe, FAKE, 64, FAKE, FAKE, FAKE, k, FAKE, FAKE, FAKE, 1 << 30, NULL) == UNS
    # too small a workspace -> NAFP_ERR_WORKSPACE before any launch
    assert lib.nafp_ivf_bucket(FAKE, 4, 10, 4, 1, FAKE, FAKE, FAKE, 0, NULL) not in (0, INV, UNS)


def test_index_classes_refuse_unsupported_shapes_without_gpu(nafp):
    from neural_audio_fp_amd.eval import ivf
    assert ivf.MAX_K == 32 and ivf.MAX_NPROBE == 128
    with pytest.raises(NotImplementedError):
        ivf.IVFPQIndex(128, 256, M=32)
    with pytest.raises(NotImplementedError):
        ivf.IVFFlatIndex(100, 16)
