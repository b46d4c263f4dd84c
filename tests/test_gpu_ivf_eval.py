"""GPU: the opt-in approximate indexes in the evaluation (NAFP_APPROX_INDEX=1): get_index, eval_faiss's files and
`run.py evaluate -i ivfpq`, against the float64 restatement (tests/_ivf_ref.py + oracle.search)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _ivf_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _data(seed=0, n_dummy=20000, n_db=1000, d=128):
    rng = np.random.default_rng(seed)
    centers = rng.normal(size=(300, d))
    dummy = _unit(centers[rng.integers(0, 300, n_dummy)] + 0.6 * rng.normal(size=(n_dummy, d)))
    db = _unit(centers[rng.integers(0, 300, n_db)] + 0.6 * rng.normal(size=(n_db, d)))
    noise = rng.choice([0.1, 0.4, 0.8], size=(n_db, 1))
    query = _unit(db + noise * rng.normal(size=db.shape) / np.sqrt(d) * 3)
    return dummy, db, query


def _write(out, arrays):
    for name, arr in arrays.items():
        mm = np.memmap(out + name + '.mm', dtype='float32', mode='w+', shape=arr.shape); mm[:] = arr; mm.flush()
        np.save(out + name + '_shape.npy', arr.shape)


def test_get_index_types_under_the_opt_in(nafp, monkeypatch, capsys):
    from neural_audio_fp_amd.eval import eval_faiss as E
    from neural_audio_fp_amd.eval.ivf import IVFFlatIndex, IVFPQIndex
    x = _data(1, n_dummy=3000, n_db=10)[0]
    monkeypatch.setenv('NAFP_APPROX_INDEX', '1')
    pq = E.get_index('ivfpq', x, x.shape)
    assert isinstance(pq, IVFPQIndex) and (pq.nlist, pq.M, pq.nbits, pq.nprobe) == (256, 64, 8, 40) and pq.is_trained
    fl = E.get_index('IVF', x, x.shape)
    assert isinstance(fl, IVFFlatIndex) and (fl.nlist, fl.nprobe) == (400, 40) and fl.is_trained
    capsys.readouterr()
    for name in ('hnsw', 'ivfpq-rr', 'ivfpq-ondisk'):
        idx = E.get_index(name, x, x.shape)
        assert type(idx) is E.FlatL2Index
        assert 'not built here' in capsys.readouterr().err
    with pytest.raises(ValueError):
        E.get_index('ivf', x[:399], (399, 128))                 # fewer training rows than nlist
    with pytest.raises(ValueError):
        E.get_index('ivfpq', x[:255], (255, 128))
    # max_nitem_train: a seeded subset of the training rows
    a = E.get_index('ivfpq', x, x.shape, max_nitem_train=1000)
    b = E.get_index('ivfpq', x, x.shape, max_nitem_train=1000)
    assert torch.equal(a.centroids, b.centroids) and torch.equal(a.pq_centroids, b.pq_centroids)
    monkeypatch.delenv('NAFP_APPROX_INDEX')
    assert type(E.get_index('ivfpq', x, x.shape)) is E.FlatL2Index


@pytest.mark.parametrize('index_type', ['ivfpq', 'ivf'])
def test_eval_faiss_with_an_approximate_index(nafp, monkeypatch, tmp_path, index_type):
    from neural_audio_fp_amd.eval import eval_faiss as E
    monkeypatch.setenv('NAFP_APPROX_INDEX', '1')
    dummy, db, query = _data(2)
    out = str(tmp_path) + '/'
    _write(out, {'query': query, 'db': db, 'dummy_db': dummy})
    rng = np.random.default_rng(3)
    test_ids = np.sort(rng.choice(1000 - 5, size=150, replace=False))
    np.save(out + 'ids.npy', test_ids)
    lens = (1, 3, 5)
    rates = E.eval_faiss(out, index_type=index_type, test_ids=out + 'ids.npy', test_seq_len='1 3 5')
    used = json.load(open(out + 'index_used.json'))
    assert used['substituted'] is False and used['index_type_requested'] == index_type
    want_used = ('IVFPQ (HIP; nlist 256, M 64, nbits 8, nprobe 40)' if index_type == 'ivfpq'
                 else 'IVF-Flat (HIP; nlist 400, nprobe 40)')
    assert used['index_type_used'] == want_used and 'approximate' in used['note']
    raw = np.load(out + 'raw_score.npy')
    # the same index again (deterministic): its top-k ids through the restatement's candidate / score / ranking steps
    idx = E.get_index(index_type, dummy, dummy.shape)
    idx.add(dummy); idx.add(db)
    _, I = idx.search(query, 20)
    table = np.concatenate([dummy, db])
    want = R.evaluate_from_ids(query, table, len(dummy), test_ids, lens, I, 20)
    assert np.array_equal(raw, np.concatenate(want[:4], axis=1))
    # hit rates against a bound from the restatement's own search with the same trained parameters
    if index_type == 'ivfpq':
        lists = idx.list_assignments().cpu().numpy()
        P = idx.probe_device(torch.from_numpy(query).cuda()).cpu().numpy()
        _, Iw = R.adc_search(query, idx.centroids.cpu().numpy(), idx.pq_centroids.cpu().numpy(), idx.codes().cpu().numpy(),
                             lists, P, 20)
    else:
        lists = idx.list_assignments().cpu().numpy()
        P = idx.probe_device(torch.from_numpy(query).cuda()).cpu().numpy()
        _, Iw = R.ivf_flat_search(query, table, lists, P, 20)
    bound = R.evaluate_from_ids(query, table, len(dummy), test_ids, lens, Iw, 20)
    for got, ref in zip(rates, bound[:4]):
        assert (got >= 100. * ref.mean(0) - 2.0).all(), (got, 100. * ref.mean(0))
    assert 5 < rates[0][0] < 100


def test_run_evaluate_records_ivfpq(nafp, tmp_path):
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
    env = dict(os.environ, PYTHONPATH=ROOT, NAFP_APPROX_INDEX='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), 'evaluate', 'EXP', '1', '-c', 'tiny', '-i', 'ivfpq', '-t',
                        str(work / 'ids.npy'), '--test_seq_len', '1 3'], cwd=work, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    used = json.load(open(emb / 'index_used.json'))
    assert used['substituted'] is False and used['index_type_used'].startswith('IVFPQ (HIP; nlist 256, M 64, nbits 8, nprobe 40)')
    assert np.load(emb / 'raw_score.npy').shape == (290, 8)
