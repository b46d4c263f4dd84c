"""CPU: the binary16-table option of the IVF-PQ search (include/nafp.h NAFP_IVF_LUT_F16): the new entry points are exported,
bound and check their arguments before any GPU call; the Python surface refuses unknown precisions without a device; and the
float64 restatement (tests/_ivf_f16_ref.py) on its own."""
import ctypes

import numpy as np
import pytest

import _ivf_f16_ref as F
import _ivf_ref as R

NULL = None
FAKE = ctypes.c_void_p(4096)          # a non-null pointer that is never dereferenced: every check below fails before use
INV, UNS = 1, 2


def _search_ex(lib, q=FAKE, nq=5, nlist=256, dim=128, nprobe=4, M=64, k=20, lut=0, ws=FAKE, ws_bytes=1 << 30):
    return lib.nafp_ivf_pq_search_ex(q, nq, FAKE, nlist, dim, nprobe, FAKE, M, FAKE, FAKE, FAKE, k, FAKE, FAKE, lut, ws, ws_bytes, NULL)


def _tables(lib, q=FAKE, nq=5, n_pairs=7, nlist=256, dim=128, M=64, lut=0, out=FAKE):
    return lib.nafp_ivf_pq_adc_tables(q, nq, FAKE, FAKE, n_pairs, FAKE, nlist, dim, FAKE, M, lut, out, NULL)


def test_new_entry_points_are_bound_and_check_arguments_without_gpu(nafp):
    assert 'nafp_ivf_pq_search_ex' in nafp._lib.PROTOTYPES and 'nafp_ivf_pq_adc_tables' in nafp._lib.PROTOTYPES
    lib = nafp._lib.load()
    assert lib.nafp_abi_version() == 1
    # null pointers and negative sizes -> INVALID_ARG
    assert lib.nafp_ivf_pq_search_ex(NULL, 1, NULL, 8, 128, 4, NULL, 64, NULL, NULL, NULL, 20, NULL, NULL, 1, NULL, 0, NULL) == INV
    assert _search_ex(lib, q=NULL) == INV and _search_ex(lib, ws=NULL) == INV
    assert _search_ex(lib, nq=-1) == INV and _search_ex(lib, nlist=0) == INV and _search_ex(lib, k=0) == INV and _search_ex(lib, nprobe=-3) == INV
    assert lib.nafp_ivf_pq_adc_tables(NULL, 1, NULL, NULL, 1, NULL, 8, 128, NULL, 64, 1, NULL, NULL) == INV
    assert _tables(lib, q=NULL) == INV and _tables(lib, out=NULL) == INV
    assert _tables(lib, nq=-1) == INV and _tables(lib, n_pairs=-1) == INV and _tables(lib, nlist=0) == INV
    # unknown lut, M, dim, k, nprobe, nlist -> UNSUPPORTED, for either known lut otherwise
    for lut in (0, 1):
        assert _search_ex(lib, lut=lut, M=32) == UNS and _search_ex(lib, lut=lut, dim=96) == UNS
        assert _search_ex(lib, lut=lut, k=33) == UNS and _search_ex(lib, lut=lut, nprobe=129) == UNS
        assert _search_ex(lib, lut=lut, nlist=16385) == UNS
        assert _tables(lib, lut=lut, M=32) == UNS and _tables(lib, lut=lut, dim=96) == UNS and _tables(lib, lut=lut, nlist=16385) == UNS
    assert _search_ex(lib, lut=2) == UNS and _search_ex(lib, lut=-1) == UNS
    assert _tables(lib, lut=2) == UNS and _tables(lib, lut=-1) == UNS
    # too small a workspace -> NAFP_ERR_WORKSPACE before any launch; nothing to do -> OK
    assert _search_ex(lib, lut=1, ws_bytes=0) not in (0, INV, UNS)
    assert _search_ex(lib, lut=1, nq=0) == 0 and _tables(lib, lut=1, n_pairs=0) == 0
    assert lib.nafp_last_hip_error() == 0                                   # no HIP call was made in any of them


def test_python_surface_refuses_unknown_precisions_without_gpu(nafp, monkeypatch):
    from neural_audio_fp_amd.eval import eval_faiss as E
    from neural_audio_fp_amd.eval import ivf
    assert ivf.LUT_CODES == {'f32': 0, 'f16': 1}
    with pytest.raises(ValueError):
        ivf.IVFPQIndex(128, 256, lut='f8')
    with pytest.raises(NotImplementedError):
        ivf.IVFPQIndex(128, 256, M=32, lut='f16')
    x = np.zeros((300, 128), np.float32)
    monkeypatch.setenv('NAFP_APPROX_INDEX', '1')
    monkeypatch.setenv('NAFP_IVFPQ_LUT', 'half')
    with pytest.raises(ValueError):
        E.get_index('ivfpq', x, x.shape)
    monkeypatch.setenv('NAFP_IVFPQ_LUT', 'f16')
    assert E.ivfpq_lut() == 'f16'
    monkeypatch.setenv('NAFP_IVFPQ_LUT', 'f32')
    assert E.ivfpq_lut() == 'f32'
    monkeypatch.delenv('NAFP_IVFPQ_LUT')
    assert E.ivfpq_lut() == 'f32'


def test_f16_tables_equal_f32_tables_on_representable_inputs_and_differ_otherwise():
    rng = np.random.default_rng(0)
    for dsub in (1, 2, 4):
        d = 64 * dsub
        # everything on the grid of multiples of 2^-1 in [-2, 2]: residuals within [-4, 4], differences to a codeword within
        # [-6, 6], their squares multiples of 2^-2 up to 36, an entry (at most 4 of them) a multiple of 2^-2 up to 144:
        # 144 * 4 = 576 < 2^11, so every entry has at most 11 significant bits and binary16 holds it exactly
        q = rng.integers(-4, 5, size=(5, d)) / 2.0
        coarse = rng.integers(-4, 5, size=(3, d)) / 2.0
        pq = rng.integers(-4, 5, size=(64, 256, dsub)) / 2.0
        pairs = (np.array([0, 1, 2, 3, 4, 4]), np.array([0, 1, 2, 0, 1, 2]))
        t32 = F.adc_tables(q, coarse, pq, *pairs, 'f32')
        t16 = F.adc_tables(q, coarse, pq, *pairs, 'f16')
        assert t32.max() <= 144 and np.array_equal(t32 * 4, np.round(t32 * 4)) and len(np.unique(t32)) > 10
        assert t16.dtype == np.float16 and np.array_equal(t16.astype(np.float64), t32)
        # generic inputs: rounding to binary16 changes the entries
        q = rng.normal(size=(5, d)) / np.sqrt(d)
        coarse = rng.normal(size=(3, d)) / np.sqrt(d)
        pq = 0.3 * rng.normal(size=(64, 256, dsub)) / np.sqrt(d)
        t32 = F.adc_tables(q, coarse, pq, *pairs, 'f32')
        t16 = F.adc_tables(q, coarse, pq, *pairs, 'f16').astype(np.float64)
        assert (t16 != t32).mean() > 0.9
        nz = t32 > 2.0 ** -14                                               # normal range: half an ulp = 2^-11 relative
        assert (np.abs(t16 - t32)[nz] <= 2.0 ** -11 * t32[nz]).all()
        assert (np.abs(t16 - t32)[~nz] <= 2.0 ** -25).all()                # subnormal range: half of 2^-24
    with pytest.raises(ValueError):
        F.adc_tables(q, coarse, pq, *pairs, 'f8')


def test_f16_search_restatement_is_the_fp32_one_on_representable_tables():
    rng = np.random.default_rng(1)
    q = rng.integers(-4, 5, size=(6, 64)) / 2.0
    coarse = rng.integers(-4, 5, size=(4, 64)) / 2.0
    pq = np.repeat((np.arange(256) % 16 / 2.0 - 4.0)[None, :, None], 64, axis=0)
    codes = rng.integers(0, 256, size=(200, 64)).astype(np.uint8)
    lists = rng.integers(0, 4, size=200)
    probes = np.stack([rng.permutation(4)[:2] for _ in range(6)])
    D, I = R.adc_search(q, coarse, pq, codes, lists, probes, 10)
    Dh, Ih = F.adc_search_f16(q, coarse, pq, codes, lists, probes, 10)
    assert np.array_equal(I, Ih) and np.array_equal(D, Dh)


def test_near_midpoint_marks_rounding_midpoints_only():
    h = np.array([1.0, 1.5, 0.001, 3.0e-6, 2.0 ** -24, 100.0], np.float16)
    up = np.nextafter(h, np.float16(np.inf)).astype(np.float64)
    mid = 0.5 * (h.astype(np.float64) + up)
    assert F.near_midpoint(mid).all() and F.near_midpoint(mid * (1 + 0.9 * F.BAND)).all() and F.near_midpoint(mid * (1 - 0.9 * F.BAND)).all()
    assert not F.near_midpoint(mid * (1 + 3 * F.BAND)).any() and not F.near_midpoint(h.astype(np.float64)).any()
    assert F.near_midpoint(np.array([2.0 ** -25])).all() and not F.near_midpoint(np.array([0.0, 2.0 ** -26])).any()


@pytest.mark.parametrize('d', [64, 128, 256])
def test_table_test_inputs_have_few_entries_near_a_midpoint(d):
    """The GPU table test excepts entries within 2^-20 (relative) of a binary16 rounding midpoint; that exception may cover at
    most 0.5 % of the entries.  Here with the restatement alone, on the same rows and query / pair construction, with
    parameters trained by a short k-means of the restatement (the GPU test asserts the share on its own trained index)."""
    from test_gpu_ivf import _clustered
    x = _clustered(5000, d, 30, d)[:1500]
    rng = np.random.default_rng(d)
    coarse = x[rng.permutation(len(x))[:50]].astype(np.float64)
    for _ in range(2):
        a = np.argmin((coarse ** 2).sum(1)[None] - 2 * x.astype(np.float64) @ coarse.T, axis=1)
        for c in range(50):
            if (a == c).any():
                coarse[c] = x[a == c].mean(0)
    a = np.argmin((coarse ** 2).sum(1)[None] - 2 * x.astype(np.float64) @ coarse.T, axis=1)
    coarse = coarse.astype(np.float32)
    r = x - coarse[a]
    init = r[rng.permutation(len(r))[:256]].reshape(256, 64, d // 64).transpose(1, 0, 2).astype(np.float64)
    pq, _ = R.pq_kmeans(r, init, 2, np.random.default_rng(5))
    pq = pq.astype(np.float32)
    codes = R.pq_encode(r, pq)
    q, pair_query, pair_list = F.table_inputs(x, coarse, pq, codes, a, d)
    assert len(pair_query) >= 300
    t = F.adc_tables(q, coarse, pq, pair_query, pair_list, 'f32')
    share = F.near_midpoint(t).mean()
    print(f'd = {d}: {t.size} entries, {100 * share:.3f} % near a midpoint, {100 * (t < 2.0 ** -14).mean():.1f} % subnormal in binary16, '
          f'{100 * (t < 2.0 ** -25).mean():.2f} % rounding to zero')
    assert share <= 0.005
    assert (t < 2.0 ** -14).sum() > 100 and (t < 2.0 ** -25).any()                 # the subnormal range and zero are covered
