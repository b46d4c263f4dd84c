"""GPU: the IVF-PQ search with binary16 ADC tables (NAFP_IVF_LUT_F16: csrc/ivf.hip ivf_pq_scan_f16_kernel, eval/ivf.py
`lut='f16'`, NAFP_IVFPQ_LUT=f16 in the evaluation) against the restatement tests/_ivf_f16_ref.py.  Data, cases and the tie rule
are those of tests/test_gpu_ivf.py and tests/test_gpu_ivf_eval.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _ivf_f16_ref as F
import _ivf_ref as R
from test_gpu_ivf import TIE, _build, _clustered, _probe_check
from test_gpu_ivf_eval import ROOT, _data, _write

pytestmark = pytest.mark.gpu


def _params(idx):
    return (idx.centroids.cpu().numpy(), idx.pq_centroids.cpu().numpy(), idx.codes().cpu().numpy(), idx.list_assignments().cpu().numpy())


@pytest.mark.parametrize('d', [64, 128, 256])
def test_tables_match_restatement(nafp, d):
    """lut 0: within 2^-20 relative (+ 1e-30) of the float64 tables.  lut 1: EQUAL to the restatement's binary16 tables, except
    entries whose float64 value lies within 2^-20 (relative) of a rounding midpoint, which may be one binary16 ulp off: after the
    shared fp32 residual the kernel's fp32 entry errs by less than (dsub + 2) * 2^-24 <= 2^-21 relative.  The exception may
    cover at most 0.5 % of the entries (a band of +-2^-20 around midpoints 2^-10 .. 2^-11 apart holds ~0.2 %)."""
    x = _clustered(5000, d, 30, d)
    idx = _build('pq', d, 50, x)
    cent, pq, codes, lists = _params(idx)
    q, pair_query, pair_list = F.table_inputs(x, cent, pq, codes, lists, d)
    assert len(pair_query) >= 300
    qd = torch.from_numpy(q).cuda()
    want = F.adc_tables(q, cent, pq, pair_query, pair_list, 'f32')
    assert idx.lut == 'f32'
    t32 = idx.adc_tables(qd, pair_query, pair_list)
    assert t32.dtype == torch.float32 and tuple(t32.shape) == (len(pair_query), 64, 256)
    err = np.abs(t32.cpu().numpy().astype(np.float64) - want)
    print(f'd = {d}: fp32 tables, max relative error {np.max(err / np.maximum(want, 1e-300)):.3e} (bound {2.0 ** -20:.3e})')
    assert (err <= 2.0 ** -20 * want + 1e-30).all()
    idx.lut = 'f16'
    t16 = idx.adc_tables(qd, torch.from_numpy(pair_query).cuda(), torch.from_numpy(pair_list).cuda())
    assert t16.dtype == torch.float16 and tuple(t16.shape) == (len(pair_query), 64, 256)
    got = t16.cpu().numpy()
    want16 = want.astype(np.float16)
    band = F.near_midpoint(want)
    share = band.mean()
    diff = got != want16
    print(f'd = {d}: fp16 tables, {diff.sum()} of {diff.size} entries differ; {100 * share:.3f} % lie near a midpoint; '
          f'{100 * (want < 2.0 ** -14).mean():.2f} % subnormal, {(want16 == 0).sum()} zero')
    assert share <= 0.005
    assert (want < 2.0 ** -14).sum() > 100 and (want16 == 0).any()          # the subnormal range and zero are exercised
    assert not (diff & ~band).any()
    g, w = got[diff], want16[diff]                                           # the excepted ones: the neighbouring binary16 value
    assert ((g == np.nextafter(w, np.float16(np.inf))) | (g == np.nextafter(w, np.float16(-np.inf)))).all()
    assert np.isfinite(got).all()
    # a pair outside the arrays gets NaNs and nothing else is disturbed
    bad = idx.adc_tables(qd, [0, len(q), 0], [0, 0, 50]).cpu().numpy()
    assert np.array_equal(bad[0], got[0]) and np.isnan(bad[1:]).all()


@pytest.mark.parametrize('d,nlist,k,nprobe', [(128, 50, 20, 40), (128, 50, 32, 50), (64, 50, 1, 1), (256, 50, 20, 40),
                                              (128, 400, 32, 1), (64, 400, 20, 40), (256, 12, 32, 12)])
def test_f16_search_matches_its_own_tables_and_the_restatement(nafp, d, nlist, k, nprobe):
    x = _clustered(5000, d, 30, d + nlist)
    q = (x[np.random.default_rng(7).permutation(5000)[:131]] + 0.05 * np.random.default_rng(8).normal(size=(131, d)) / np.sqrt(d)).astype(np.float32)
    idx = _build('pq', d, nlist, x)
    idx.nprobe = nprobe
    idx.lut = 'f16'
    P = _probe_check(idx, q)
    cent, pq, codes, lists = _params(idx)
    D, I = idx.search(q, k)
    assert D.shape == (131, k) and I.dtype == np.int64
    Dw, Iw = F.adc_search_f16(q, cent, pq, codes, lists, P, k)
    fin = np.isfinite(Dw)
    assert np.array_equal(np.isfinite(D), fin) and ((I == -1) == ~fin).all()     # -1 / +inf padding where the lists run out
    # the kernel's own tables, exported: (131 * np, 64, 256) binary16
    npr = P.shape[1]
    T = idx.adc_tables(torch.from_numpy(q).cuda(), np.repeat(np.arange(131), npr), P.reshape(-1)).cpu().numpy()
    slot = {(i, int(l)): i * npr + j for i in range(131) for j, l in enumerate(P[i])}
    m_idx = np.arange(64)

    def dist_of(r, i):                                                       # float64 sum of the exported entries the row's codes pick
        return float(T[slot[(r, int(lists[i]))]][m_idx, codes[i]].astype(np.float64).sum())
    worst = 0.0
    for r, c in np.argwhere(fin):
        dd = dist_of(r, I[r, c])
        worst = max(worst, abs(D[r, c] - dd) / max(1.0, dd))
        assert abs(D[r, c] - dd) <= TIE * max(1.0, dd), (r, c)
    n_bad = 0
    for r, c in np.argwhere(I != Iw):                                        # ids: the restatement's, or a tie under that same sum
        assert I[r, c] >= 0 and Iw[r, c] >= 0, (r, c, I[r], Iw[r])
        assert abs(dist_of(r, I[r, c]) - dist_of(r, Iw[r, c])) < TIE, (r, c)
        n_bad += 1
    print(f'd {d} nlist {nlist} k {k} nprobe {nprobe}: max |D - sum of exported entries| / max(1, D) = {worst:.3e} (bound {TIE:.0e}); '
          f'{n_bad} of {I.size} ids differ from the restatement (ties)')
    assert np.all(np.diff(np.where(fin, D, np.float32(3e38)), axis=1) >= 0)
    if nlist == 400 and nprobe == 1:
        assert (~fin).any()                                                  # lists shorter than k


def _repro_data():
    return _clustered(20000, 128, 40, 13), _clustered(301, 128, 40, 14)


def _raw_search(idx, q, k, lut):
    """The C entry points directly: lut None = nafp_ivf_pq_search, else nafp_ivf_pq_search_ex(lut)."""
    from neural_audio_fp_amd import _lib
    lib = _lib.load()
    L = idx._prepare()
    qd = torch.from_numpy(q).cuda()
    D = torch.empty((len(q), k), dtype=torch.float32, device='cuda')
    I = torch.empty((len(q), k), dtype=torch.int32, device='cuda')
    need = int(lib.nafp_ivf_search_workspace_bytes(len(q), idx.nlist, idx.nprobe, k, 1))
    ws = torch.empty((need,), dtype=torch.uint8, device='cuda')
    head = (_lib.ptr(qd), len(q), _lib.ptr(idx.centroids), idx.nlist, idx.d, idx.nprobe, _lib.ptr(idx.pq_centroids), idx.M,
            _lib.ptr(L['codes']), _lib.ptr(L['offsets']), _lib.ptr(L['ids']), k, _lib.ptr(D), _lib.ptr(I))
    tail = (_lib.ptr(ws), need, _lib.current_stream())
    if lut is None:
        _lib.check(lib.nafp_ivf_pq_search(*head, *tail), 'ivf_pq_search')
    else:
        _lib.check(lib.nafp_ivf_pq_search_ex(*head, lut, *tail), 'ivf_pq_search_ex')
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy()


def test_lut_f32_is_the_plain_search_byte_for_byte_and_f16_is_not(nafp):
    x, q = _repro_data()
    idx = _build('pq', 128, 64, x, pieces=1)
    idx.nprobe = 10
    D0, I0 = _raw_search(idx, q, 20, None)
    D1, I1 = _raw_search(idx, q, 20, 0)
    assert D1.tobytes() == D0.tobytes() and I1.tobytes() == I0.tobytes()
    assert idx.lut == 'f32'
    Dd, Id = idx.search_device(torch.from_numpy(q).cuda(), 20)
    assert Dd.cpu().numpy().tobytes() == D0.tobytes() and Id.cpu().numpy().tobytes() == I0.tobytes()
    D2, I2 = _raw_search(idx, q, 20, 1)
    assert D2.tobytes() != D0.tobytes()
    idx.lut = 'f16'
    Dh, Ih = idx.search_device(torch.from_numpy(q).cuda(), 20)
    assert Dh.cpu().numpy().tobytes() == D2.tobytes() and Ih.cpu().numpy().tobytes() == I2.tobytes()
    assert np.abs(D2 - D0).max() < 64 * 2.0 ** -11 * 4                       # ... but only by the rounding of 64 entries <= 4
    from neural_audio_fp_amd import _lib
    with pytest.raises(_lib.NafpError):
        _raw_search(idx, q, 20, 2)


def test_f16_results_are_reproducible_and_independent_of_batching(nafp):
    x, q = _repro_data()
    a = _build('pq', 128, 64, x, pieces=1)
    b = _build('pq', 128, 64, x, pieces=3)
    for idx in (a, b):
        idx.nprobe = 10
    Df, If = a.search(q, 20)                                                 # fp32 first
    for idx in (a, b):
        idx.lut = 'f16'
    Da, Ia = a.search(q, 20)
    Db, Ib = b.search(q, 20)
    assert np.array_equal(Ia, Ib) and Da.tobytes() == Db.tobytes()
    assert Da.tobytes() != Df.tobytes()
    parts = [a.search(q[s], 20) for s in (slice(0, 1), slice(1, 130), slice(130, 301))]
    assert np.array_equal(np.concatenate([p[1] for p in parts]), Ia)
    assert np.concatenate([p[0] for p in parts]).tobytes() == Da.tobytes()
    assert np.array_equal(a.search(q, 20)[1], Ia) and a.search(q, 20)[0].tobytes() == Da.tobytes()
    # back and forth on one index, nothing re-added: both results come back
    lists_before = a._lists
    for lut, (Dw, Iw) in (('f32', (Df, If)), ('f16', (Da, Ia)), ('f32', (Df, If)), ('f16', (Da, Ia))):
        a.lut = lut
        D, I = a.search(q, 20)
        assert D.tobytes() == Dw.tobytes() and np.array_equal(I, Iw), lut
    assert a._lists is lists_before
    with pytest.raises(ValueError):
        a.lut = 'bf16'
    assert a.lut == 'f16'
    with pytest.raises(NotImplementedError):
        a.search(q[:2], 33)


def test_eval_faiss_with_fp16_tables(nafp, monkeypatch, tmp_path):
    from neural_audio_fp_amd.eval import eval_faiss as E
    from neural_audio_fp_amd.eval.ivf import IVFFlatIndex, IVFPQIndex
    monkeypatch.setenv('NAFP_APPROX_INDEX', '1')
    monkeypatch.setenv('NAFP_IVFPQ_LUT', 'f16')
    dummy, db, query = _data(2)
    out = str(tmp_path) + '/'
    _write(out, {'query': query, 'db': db, 'dummy_db': dummy})
    rng = np.random.default_rng(3)
    test_ids = np.sort(rng.choice(1000 - 5, size=150, replace=False))
    np.save(out + 'ids.npy', test_ids)
    lens = (1, 3, 5)
    rates = E.eval_faiss(out, index_type='ivfpq', test_ids=out + 'ids.npy', test_seq_len='1 3 5')
    used = json.load(open(out + 'index_used.json'))
    assert used['substituted'] is False and used['index_type_requested'] == 'ivfpq'
    assert used['index_type_used'] == 'IVFPQ (HIP; nlist 256, M 64, nbits 8, nprobe 40, fp16 tables)'
    raw = np.load(out + 'raw_score.npy')
    idx = E.get_index('ivfpq', dummy, dummy.shape)
    assert isinstance(idx, IVFPQIndex) and idx.lut == 'f16'
    idx.add(dummy); idx.add(db)
    _, I = idx.search(query, 20)
    table = np.concatenate([dummy, db])
    want = R.evaluate_from_ids(query, table, len(dummy), test_ids, lens, I, 20)
    assert np.array_equal(raw, np.concatenate(want[:4], axis=1))
    cent, pq, codes, lists = _params(idx)
    P = idx.probe_device(torch.from_numpy(query).cuda()).cpu().numpy()
    _, Iw = F.adc_search_f16(query, cent, pq, codes, lists, P, 20)
    bound = R.evaluate_from_ids(query, table, len(dummy), test_ids, lens, Iw, 20)
    for got, ref in zip(rates, bound[:4]):
        print('hit rates', got, 'restatement', 100. * ref.mean(0))
        assert (got >= 100. * ref.mean(0) - 2.0).all(), (got, 100. * ref.mean(0))
    assert 5 < rates[0][0] < 100
    # the other index types ignore the variable
    small = dummy[:3000]
    fl = E.get_index('ivf', small, small.shape)
    assert isinstance(fl, IVFFlatIndex) and fl.index_description == 'IVF-Flat (HIP; nlist 400, nprobe 40)'
    assert type(E.get_index('hnsw', small, small.shape)) is E.FlatL2Index and type(E.get_index('l2', small, small.shape)) is E.FlatL2Index
    monkeypatch.setenv('NAFP_IVFPQ_LUT', 'f32')
    assert E.get_index('ivfpq', small, small.shape).index_description == 'IVFPQ (HIP; nlist 256, M 64, nbits 8, nprobe 40)'


def test_run_evaluate_records_fp16_tables(nafp, tmp_path):
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
    env = dict(os.environ, PYTHONPATH=ROOT, NAFP_APPROX_INDEX='1', NAFP_IVFPQ_LUT='f16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), 'evaluate', 'EXP', '1', '-c', 'tiny', '-i', 'ivfpq', '-t',
                        str(work / 'ids.npy'), '--test_seq_len', '1 3'], cwd=work, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    used = json.load(open(emb / 'index_used.json'))
    assert used['substituted'] is False
    assert used['index_type_used'] == 'IVFPQ (HIP; nlist 256, M 64, nbits 8, nprobe 40, fp16 tables)'
    assert np.load(emb / 'raw_score.npy').shape == (290, 8)
