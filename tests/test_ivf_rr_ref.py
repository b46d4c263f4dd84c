"""CPU: the float64 restatement of the IVFPQ-RR contract (tests/_ivf_rr_ref.py) on its own, the new entry points of the C ABI
(include/nafp.h "IVFPQ-RR": declared, bound, arguments checked before any GPU call) and what must not have moved (the random
streams of eval/ivf.py, the k <= 32 refusal of the plain IVF-PQ search)."""
import ctypes

import numpy as np

import _ivf_ref as R
import _ivf_rr_ref as RR

FAKE = ctypes.c_void_p(4096)          # a non-null pointer that is never dereferenced: every check below fails before use


def _small_index(seed=0, n=1500, d=64, nlist=8):
    rng = np.random.default_rng(seed)
    centers = rng.normal(size=(12, d))
    x = centers[rng.integers(0, 12, n)] + 0.4 * rng.normal(size=(n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    dsub = d // 64
    coarse_init = x[rng.permutation(n)[:nlist]]
    pq_init = 0.2 * rng.normal(size=(64, 256, dsub))
    refine_init = 0.02 * rng.normal(size=(4, 16, d // 4))
    idx = RR.train_and_add(x, x, coarse_init, pq_init, refine_init, 4, 3, [np.random.default_rng(s) for s in (1, 2, 3)])
    q = x[rng.permutation(n)[:40]] + 0.05 * rng.normal(size=(40, d))
    return x, q, idx


def test_nibble_packing_round_trips():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 16, size=(1000, 4)).astype(np.uint8)
    b = RR.pack_codes(c)
    assert b.shape == (1000, 2) and b.dtype == np.uint8
    assert np.array_equal(RR.unpack_codes(b), c)
    assert np.array_equal(RR.pack_codes(np.array([[1, 2, 3, 4], [15, 0, 0, 15]])), [[0x21, 0x43], [0x0f, 0xf0]])
    every = np.arange(65536, dtype=np.uint32)                     # every pair of bytes is a code row and comes back
    allb = np.stack([every & 255, every >> 8], 1).astype(np.uint8)
    assert np.array_equal(RR.pack_codes(RR.unpack_codes(allb)), allb)


def test_reranked_distances_are_reconstruction_distances_and_refine_lowers_the_error():
    x, q, idx = _small_index()
    P, _ = R.probe(q, idx['coarse'], 4)
    D1, I1, D, I = RR.search(q, idx['coarse'], idx['pq'], idx['refine'], idx['codes'], idx['rcodes'], idx['lists'], P, 5, 4)
    assert D1.shape == (40, 20) and D.shape == (40, 5)
    rec = RR.reconstruct(np.arange(len(x)), idx['coarse'], idx['pq'], idx['refine'], idx['codes'], idx['rcodes'], idx['lists'])
    for i in range(len(q)):
        fin = I[i] >= 0
        true = ((q[i] - rec[I[i][fin]]) ** 2).sum(1)              # recomputed from scratch
        assert (D[i][fin] >= true - 1e-12).all() and np.allclose(D[i][fin], true, rtol=0, atol=1e-12)
        assert np.isin(I[i][fin], I1[i]).all()                    # stage 2 only chooses among stage 1
        assert (np.diff(D[i][fin]) >= 0).all()
    # the refine codes are arg-mins per sub-space, so the refined reconstruction is never farther from the row than the PQ one
    rec_pq = idx['coarse'][idx['lists']] + R.pq_decode(idx['codes'].astype(np.int64), idx['pq'])
    e_pq, e_rr = ((x - rec_pq) ** 2).sum(1), ((x - rec) ** 2).sum(1)
    r2 = RR.second_residuals(x - idx['coarse'][idx['lists']], idx['pq'], idx['codes'])
    assert np.allclose(r2, x - rec_pq)
    zero_code = ((r2.reshape(len(x), 4, -1)[:, :, None, :] - idx['refine'][None]) ** 2).sum(-1)      # (n, 4, 16)
    best = zero_code.min(-1).sum(1)
    assert np.allclose(e_rr, best) and e_rr.mean() < e_pq.mean()


def test_stage_two_with_k_factor_one_only_reorders_stage_one():
    x, q, idx = _small_index(seed=5)
    P, _ = R.probe(q, idx['coarse'], 3)
    D1, I1, D, I = RR.search(q, idx['coarse'], idx['pq'], idx['refine'], idx['codes'], idx['rcodes'], idx['lists'], P, 12, 1)
    assert I1.shape == I.shape == (40, 12)
    assert np.array_equal(np.sort(I, axis=1), np.sort(I1, axis=1))
    assert (np.diff(np.where(np.isfinite(D), D, 1e300), axis=1) >= 0).all()
    assert (I != I1).any()                                        # ... and it does re-order
    # padding: a single short list probed, more candidates asked than it has
    short = int(np.argmin(np.bincount(idx['lists'], minlength=len(idx['coarse']))))
    n_in = int((idx['lists'] == short).sum())
    D1s, I1s, Ds, Is = RR.search(q[:3], idx['coarse'], idx['pq'], idx['refine'], idx['codes'], idx['rcodes'], idx['lists'],
                                 np.full((3, 1), short), 32, 4)
    assert n_in < 128 and (I1s[:, n_in:] == -1).all() and np.isinf(D1s[:, n_in:]).all()
    m = min(n_in, 32)
    assert (Is[:, :m] >= 0).all() and (Is[:, m:] == -1).all() and np.isinf(Ds[:, m:]).all()


def test_new_header_symbols_are_declared_and_bound(nafp):
    import test_abi
    lib = nafp._lib.load()
    declared = test_abi._declared()
    for name in ('nafp_ivf_pq_residuals', 'nafp_ivf_refine_encode', 'nafp_ivf_pq_wide_workspace_bytes', 'nafp_ivf_pq_search_wide',
                 'nafp_ivf_pqr_rerank', 'nafp_ivf_pqr_search'):
        assert name in declared, f'{name} is not declared in include/nafp.h'
        assert name in nafp._lib.PROTOTYPES, f'{name} is not bound in _lib.py'
        assert getattr(lib, name) is not None
    assert lib.nafp_abi_version() == 1


def test_argument_checks_of_the_new_entry_points_and_the_old_refusals(nafp):
    lib = nafp._lib.load()
    INVALID, UNSUPPORTED, WORKSPACE = 1, 2, 4
    # the plain IVF-PQ search keeps refusing k > 32; the wide one goes to 128
    assert lib.nafp_ivf_search_workspace_bytes(10, 256, 40, 33, 1) == -1 and lib.nafp_ivf_search_workspace_bytes(10, 256, 40, 32, 1) > 0
    assert lib.nafp_ivf_pq_search_ex(FAKE, 10, FAKE, 256, 128, 40, FAKE, 64, FAKE, FAKE, FAKE, 33, FAKE, FAKE, 0, FAKE, 1 << 40, None) == UNSUPPORTED
    small, big = lib.nafp_ivf_pq_wide_workspace_bytes(10, 256, 40, 80), lib.nafp_ivf_pq_wide_workspace_bytes(10, 256, 40, 128)
    assert small > 0 and big > 0
    assert lib.nafp_ivf_pq_wide_workspace_bytes(10, 256, 40, 129) == -1 and lib.nafp_ivf_pq_wide_workspace_bytes(10, 256, 129, 80) == -1
    assert lib.nafp_ivf_pq_wide_workspace_bytes(38000, 256, 40, 128) > 0 and lib.nafp_ivf_pq_wide_workspace_bytes(1, 16384, 128, 128) > 0
    wide = lambda **kw: lib.nafp_ivf_pq_search_wide(kw.get('q', FAKE), 10, FAKE, 256, kw.get('dim', 128), 40, FAKE, kw.get('M', 64), FAKE, FAKE,
                                                    FAKE, kw.get('k1', 80), FAKE, FAKE, kw.get('lut', 0), FAKE, kw.get('ws', 1 << 40), None)
    assert wide(q=None) == INVALID and wide(k1=0) == INVALID
    assert wide(k1=129) == UNSUPPORTED and wide(dim=96) == UNSUPPORTED and wide(M=32) == UNSUPPORTED and wide(lut=2) == UNSUPPORTED
    assert wide(ws=small - 1) == WORKSPACE
    enc = lambda **kw: lib.nafp_ivf_refine_encode(kw.get('x', FAKE), 10, kw.get('dim', 128), FAKE, kw.get('mr', 4), kw.get('nb', 4),
                                                  kw.get('packed', 1), FAKE, None)
    assert enc(x=None) == INVALID
    assert enc(mr=8) == UNSUPPORTED and enc(nb=8) == UNSUPPORTED and enc(dim=32) == UNSUPPORTED and enc(packed=2) == UNSUPPORTED
    assert lib.nafp_ivf_refine_encode(FAKE, 0, 128, FAKE, 4, 4, 1, FAKE, None) == 0
    assert lib.nafp_ivf_pq_residuals(None, 10, 128, FAKE, 64, FAKE, FAKE, None) == INVALID
    assert lib.nafp_ivf_pq_residuals(FAKE, 10, 128, FAKE, 16, FAKE, FAKE, None) == UNSUPPORTED
    assert lib.nafp_ivf_pq_residuals(FAKE, 1 << 24, 256, FAKE, 64, FAKE, FAKE, None) == UNSUPPORTED
    assert lib.nafp_ivf_pq_residuals(FAKE, (1 << 31) - 1, 256, FAKE, 64, FAKE, FAKE, None) == UNSUPPORTED     # 2^32 elements or more: not one launch
    rr = lambda **kw: lib.nafp_ivf_pqr_rerank(FAKE, 10, kw.get('dim', 128), kw.get('cand', FAKE), kw.get('k1', 80), FAKE, FAKE, FAKE, 64, FAKE,
                                              FAKE, kw.get('mr', 4), 4, FAKE, 1000, kw.get('k', 20), FAKE, FAKE, None)
    assert rr(cand=None) == INVALID
    assert rr(k1=129) == UNSUPPORTED and rr(k=33) == UNSUPPORTED and rr(k=20, k1=10) == UNSUPPORTED and rr(mr=2) == UNSUPPORTED
    both = lambda **kw: lib.nafp_ivf_pqr_search(FAKE, 10, FAKE, 256, 128, 40, FAKE, 64, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 4, kw.get('nb', 4), FAKE,
                                                1000, kw.get('k', 20), kw.get('kf', 4), FAKE, FAKE, kw.get('d1', FAKE), FAKE, 0, FAKE,
                                                kw.get('ws', 1 << 40), None)
    assert both(d1=None) == INVALID and both(kf=0) == INVALID
    assert both(k=33) == UNSUPPORTED and both(kf=5) == UNSUPPORTED and both(nb=8) == UNSUPPORTED
    assert both(ws=small - 1) == WORKSPACE


def test_the_five_earlier_random_streams_keep_their_numbers(nafp):
    from neural_audio_fp_amd.eval import ivf
    assert (ivf.STREAM_TRAIN_SUBSET, ivf.STREAM_COARSE, ivf.STREAM_COARSE_SPLIT, ivf.STREAM_PQ, ivf.STREAM_PQ_SPLIT) == (0, 1, 2, 3, 4)
    assert (ivf.STREAM_REFINE, ivf.STREAM_REFINE_SPLIT) == (5, 6)
    assert ivf.rng_for(1234, ivf.STREAM_PQ).integers(0, 1 << 30) == np.random.default_rng([1234, 3]).integers(0, 1 << 30)
