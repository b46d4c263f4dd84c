"""GPU: nafp_search_seq_match (csrc/search.hip) -- from the top-k ids of the segment search to the ranked predictions in one
launch -- against its numpy restatement (tests/_seq_match_ref.py), against nafp_search_seq_scores (the same bits per candidate),
and through `search_and_score(device_rank=True)` / NAFP_SEQ_MATCH=1 against the host ranking and the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _seq_match_ref as M
from oracle import search as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_TASKS = 257


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).cuda()


def _raw_match(nafp, query, index, n_index, topk, q0, ln, max_len, n_out, with_n_cand=True):
    """The C entry point itself, with an explicit n_index (device tensors in, numpy out)."""
    L = nafp._lib
    lib = L.load()
    T = len(q0)
    ids = torch.full((T, n_out), -7, dtype=torch.int32, device='cuda')
    sc = torch.full((T, n_out), 123.0, dtype=torch.float32, device='cuda')
    nc = torch.full((T,), -7, dtype=torch.int32, device='cuda')
    L.check(lib.nafp_search_seq_match(L.ptr(query), query.shape[0], L.ptr(index), int(n_index), query.shape[1], L.ptr(topk), topk.shape[1],
                                      L.ptr(q0), L.ptr(ln), T, int(max_len), int(n_out), L.ptr(ids), L.ptr(sc),
                                      L.ptr(nc) if with_n_cand else None, L.current_stream()), 'search_seq_match')
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy(), nc.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _lattice_launch(d, N, k, max_len, seed):
    """One launch of T_TASKS tasks on integer data (entries -2 .. 2: every fp32 sum is exact, so the restatement gives the kernel's
    bits), every length 1 .. max_len mixed, with synthetic top-k ids: random rows, -1 entries, ids below their row offset, ids next
    to the end of the table, planted runs, a repeated passage, and the three degenerate tasks."""
    rng = np.random.default_rng(seed)
    nq = 300
    table = rng.integers(-2, 3, size=(N, d)).astype(np.float32)
    if N >= 60:
        table[40:40 + 16] = table[10:10 + 16]                           # a repeated passage: distinct candidates tie exactly
    query = table[rng.integers(0, N, nq)].copy()
    redraw = rng.random(size=query.shape) < 0.15
    query[redraw] = rng.integers(-2, 3, size=int(redraw.sum())).astype(np.float32)
    topk = rng.integers(0, N, size=(nq, k)).astype(np.int32)
    if N < k:                                                           # fewer rows than k: the search pads with -1
        topk = np.stack([rng.permutation(N) for _ in range(nq)]).astype(np.int32)
        topk = np.concatenate([topk, -np.ones((nq, k - N), np.int32)], 1)
    small = rng.random(size=topk.shape) < 0.1                           # ids smaller than their row offset: negative after compensation
    topk[small] = rng.integers(0, min(N, max_len + 1), size=int(small.sum()))
    late = rng.random(size=topk.shape) < 0.1                            # c + len > N: the mean is shortened
    topk[late] = N - 1 - rng.integers(0, min(N, max_len + 1), size=int(late.sum()))
    topk[rng.random(size=topk.shape) < 0.03] = -1
    q0 = rng.integers(0, nq - max_len, size=T_TASKS).astype(np.int32)
    ln = (1 + np.arange(T_TASKS) % max_len).astype(np.int32)
    for t in range(0, T_TASKS, 5):                                      # planted runs: one candidate in every row of the task
        c = int(rng.integers(0, N))
        if N >= 60 and t % 10 == 0:
            c = 10 + int(rng.integers(0, 4))                            # ... inside the repeated passage, with its twin 30 rows on
        for i in range(int(ln[t])):
            if c + i < N:
                j = int(rng.integers(0, k))
                topk[q0[t] + i, j] = c + i
                if N >= 60 and t % 10 == 0 and k > 1:                   # ... both copies found, by a query that is the passage itself
                    topk[q0[t] + i, (j + 1) % k] = c + 30 + i
                    query[q0[t] + i] = table[c + i]
    ln[3] = 0                                                           # no rows
    q0[7] = nq                                                          # outside [0, n_query)
    q0[11] = -2
    q0[13], ln[13] = nq - 1 - (max_len > 1), max_len                    # rows run past n_query
    ln[17] = max_len + 5                                                # clipped by max_len
    return query, table, topk, q0, ln


@pytest.mark.parametrize('d,N,k,max_len,n_out', [(64, 300, 20, 19, 10), (128, 257, 1, 1, 10), (256, 500, 32, 64, 32),
                                                  (128, 7, 20, 3, 10), (128, 1000, 20, 19, 3)])
def test_lattice_launch_equals_the_restatement_bit_for_bit(nafp, d, N, k, max_len, n_out):
    query, table, topk, q0, ln = _lattice_launch(d, N, k, max_len, seed=d + N)
    want = M.seq_match(query, table, topk, q0, ln, max_len, n_out)
    got = _raw_match(nafp, _dev(query), _dev(table), N, _dev(topk), _dev(q0), _dev(ln), max_len, n_out)
    for name, g, w in zip(('ids', 'scores', 'n_cand'), got, want):
        assert _same_bits(g, w), (name, np.argwhere(g != w)[:5])
    # the launch holds what it is meant to hold
    ids, sc, nc = want
    assert nc[3] == 0 and nc[7] == 0 and nc[11] == 0 and (ids[[3, 7, 11]] == -1).all()
    if min(N, k * max_len) > n_out:
        assert (nc > n_out).any()                                                # more candidates than outputs
    if k > 1:
        assert (nc[ln > 0] < (k * ln.clip(0, max_len))[ln > 0]).any()            # duplicates (or absent slots) removed
    if N >= 60 and k > 1:
        assert ((sc[:, 1:] == sc[:, :-1]) & (ids[:, 1:] >= 0)).any()             # exactly equal scores of distinct candidates
    # the optional output may be left out
    again = _raw_match(nafp, _dev(query), _dev(table), N, _dev(topk), _dev(q0), _dev(ln), max_len, n_out, with_n_cand=False)
    assert _same_bits(again[0], got[0]) and _same_bits(again[1], got[1]) and (again[2] == -7).all()


def _unit(n, d, seed):
    x = np.random.default_rng(seed).normal(size=(n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _host_rank(cand, scores, n_out):
    """The host ranking of search_and_score on the full (T, S) candidate / score arrays."""
    c = cand.astype(np.int64)
    s = scores.astype(np.float64)
    order = np.argsort(c, axis=1, kind='stable')
    c = np.take_along_axis(c, order, 1); s = np.take_along_axis(s, order, 1)
    dup = np.zeros_like(c, dtype=bool)
    dup[:, 1:] = c[:, 1:] == c[:, :-1]
    s[dup | (c < 0)] = -np.inf
    rank = np.lexsort((c, -s), axis=1)[:, :n_out]
    p = np.take_along_axis(c, rank, 1)
    ps = np.take_along_axis(s, rank, 1)
    p[ps == -np.inf] = -1
    return p, ps.astype(np.float32)


@pytest.mark.parametrize('d', [64, 128, 256])
def test_scores_are_the_bits_of_seq_scores_and_ids_the_host_ranking(nafp, d):
    from neural_audio_fp_amd.eval.eval_faiss import FlatL2Index
    rng = np.random.default_rng(d)
    N, nq, k, max_len, T = 900, 140, 20, 19, 70
    table = _unit(N, d, d + 1)
    start = 300
    query = table[start:start + nq] + 0.6 * rng.normal(size=(nq, d)).astype(np.float32) / np.sqrt(d)
    query = (query / np.linalg.norm(query, axis=1, keepdims=True)).astype(np.float32)
    idx = FlatL2Index(d); idx.add(table)
    qd = _dev(query)
    _, I = idx.search_device(qd, k)
    q0 = rng.integers(0, nq - max_len, size=T).astype(np.int32)
    ln = rng.choice([1, 3, 5, 9, 11, 19], size=T).astype(np.int32)
    q0[-1], ln[-1] = nq - 4, 19                                           # clipped by the end of the queries
    ids, sc, nc = (t.cpu().numpy() for t in idx.sequence_match(qd, I, _dev(q0), _dev(ln), n_out=10))
    # the (T, S) candidate tensor of the host path, scored slot by slot by nafp_search_seq_scores
    Ih = I.cpu().numpy().astype(np.int64)
    ln_eff = np.minimum(ln, nq - q0).astype(np.int32)
    cand = -np.ones((T, max_len, k), np.int64)
    for t in range(T):
        for i in range(ln_eff[t]):
            c = Ih[q0[t] + i] - i
            cand[t, i] = np.where((Ih[q0[t] + i] >= 0) & (c >= 0), c, -1)
    cand = cand.reshape(T, max_len * k).astype(np.int32)
    full = idx.sequence_scores(qd, _dev(q0), _dev(ln_eff), _dev(cand)).cpu().numpy()
    p, ps = _host_rank(cand, full, 10)
    assert np.array_equal(ids, p)
    assert _same_bits(sc, ps)
    for t in range(T):
        assert nc[t] == len(np.unique(cand[t][cand[t] >= 0]))
    assert (ids[:, 0] == start + q0).mean() > 0.5                          # the sequences are found: the case is not noise


def test_edges(nafp):
    rng = np.random.default_rng(2)
    d, nq, k = 128, 40, 8
    table = rng.integers(-2, 3, size=(256, d)).astype(np.float32)
    query = rng.integers(-2, 3, size=(nq, d)).astype(np.float32)
    td, qd = _dev(table), _dev(query)

    def run(topk, q0, ln, max_len, n_out=10, n_index=256, tab=None, qry=None):
        args = (np.asarray(topk, np.int32), np.asarray(q0, np.int32), np.asarray(ln, np.int32))
        got = _raw_match(nafp, qd if qry is None else _dev(qry), td if tab is None else _dev(tab), n_index, *(_dev(a) for a in args),
                         max_len, n_out)
        want = M.seq_match(query if qry is None else qry, table if tab is None else tab, *args, max_len, n_out, n_index=n_index)
        for g, w in zip(got, want):
            assert _same_bits(g, w)
        return got

    # every slot names the same candidate
    same = np.tile(50 + np.arange(nq)[:, None], (1, k))
    ids, sc, nc = run(same, [0, 3], [5, 5], 5)
    assert nc.tolist() == [1, 1] and ids[:, 0].tolist() == [50, 53] and (ids[:, 1:] == -1).all() and np.isneginf(sc[:, 1:]).all()
    # fewer distinct candidates than n_out
    few = rng.integers(100, 104, size=(nq, k))
    ids, sc, nc = run(few, [0, 9], [1, 2], 2)
    assert (nc < 10).all() and (nc >= 1).all() and all((ids[t, nc[t]:] == -1).all() and (ids[t, :nc[t]] >= 0).all() for t in range(2))
    # every slot invalid: -1, past the table, or below the row offset
    bad = np.where(rng.random(size=(nq, k)) < 0.5, -1, 256 + rng.integers(0, 1000, size=(nq, k)))
    bad[1:4, 0] = bad[20, 0] = 0                                            # id 0 is below the row offsets 1 .. 3, and valid at offset 0
    ids, sc, nc = run(bad, [0, 30, 20], [4, 4, 1], 4)
    assert (ids[:2] == -1).all() and nc[:2].tolist() == [0, 0] and np.isneginf(sc[:2]).all()
    assert ids[2].tolist() == [0] + [-1] * 9 and nc[2] == 1                 # (row 20 of the queries is row offset 0 of its task)
    # ids >= n_index are ignored: the tensor has 256 rows, the index 200 -- a kernel without the guard would rank rows 200 .. 255
    mixed = rng.integers(150, 256, size=(nq, k))
    ids, sc, nc = run(mixed, [0, 10, 30], [3, 6, 6], 6, n_index=200)
    assert (ids < 200).all() and (ids >= 0).any()
    wide = M.seq_match(query, table, mixed.astype(np.int32), [0, 10, 30], [3, 6, 6], 6, 10, n_index=256)[0]
    assert (wide >= 200).any()                                            # ... and they would have made the top 10
    # a NaN row, and a +inf / -inf pair in one row: the candidates that touch them are dropped, the others unchanged
    topk = rng.integers(60, 120, size=(nq, k))
    q2 = query.copy()
    q2[:, 3] = q2[:, 70] = 1.0                                             # the pair meets as +inf + -inf = NaN in every row product
    clean = run(topk, [0, 8, 16], [4, 4, 4], 4, n_out=32, qry=q2)
    dirty = table.copy()
    dirty[80, 5] = np.nan
    dirty[100, 3], dirty[100, 70] = np.inf, -np.inf
    ids, sc, nc = run(topk, [0, 8, 16], [4, 4, 4], 4, n_out=32, tab=dirty, qry=q2)
    touched = lambda c: (c <= 80) & (80 < c + 4) | (c <= 100) & (100 < c + 4)
    assert (nc <= clean[2]).all() and (nc < clean[2]).any() and not touched(ids[ids >= 0]).any() and np.isfinite(sc[ids >= 0]).all()
    for t in range(3):
        keep = ~touched(clean[0][t]) & (clean[0][t] >= 0)
        assert np.array_equal(clean[0][t][keep], ids[t][:keep.sum()]) and _same_bits(clean[1][t][keep], sc[t][:keep.sum()])


def test_two_runs_are_byte_identical_and_a_task_does_not_depend_on_its_launch(nafp):
    query, table, topk, q0, ln = _lattice_launch(64, 300, 20, 19, seed=5)
    # unit-norm rows on top of the lattice case: rounding now depends on the summation order, which must not depend on the launch
    table = (table + 0.25) / np.linalg.norm(table + 0.25, axis=1, keepdims=True)
    query = (query + 0.25) / np.linalg.norm(query + 0.25, axis=1, keepdims=True)
    qd, td, kd = _dev(query, np.float32), _dev(table, np.float32), _dev(topk)
    full = _raw_match(nafp, qd, td, 300, kd, _dev(q0), _dev(ln), 19, 10)
    again = _raw_match(nafp, qd, td, 300, kd, _dev(q0), _dev(ln), 19, 10)
    for a, b in zip(full, again):
        assert _same_bits(a, b)
    for a, b in ((0, 1), (100, 131), (250, 257)):
        part = _raw_match(nafp, qd, td, 300, kd, _dev(q0[a:b]), _dev(ln[a:b]), 19, 10)
        for f, p in zip(full, part):
            assert _same_bits(f[a:b], p)
    # a larger max_len than any task needs changes the padding of the launch, not the rows
    roomy = _raw_match(nafp, qd, td, 300, kd, _dev(q0), _dev(np.minimum(ln, 19)), 64, 10)
    for f, p in zip(full, roomy):
        assert _same_bits(f, p)


@pytest.fixture(scope='module')
def eval_case():
    """The data of test_gpu_search.py::test_sequence_evaluation_matches_oracle_and_writes_reference_files, and the oracle's
    evaluation of it (computed once)."""
    rng = np.random.default_rng(5)
    d = 128
    dummy, db = _unit(3000, d, 6), _unit(800, d, 7)
    noise = rng.choice([0.05, 0.8, 1.5], size=(800, 1))
    query = db + noise * rng.normal(size=db.shape) / np.sqrt(d) * 3
    query = (query / np.linalg.norm(query, axis=1, keepdims=True)).astype(np.float32)
    test_ids = np.sort(rng.choice(800 - 19, size=120, replace=False))
    test_ids[-1] = 795                                       # a sequence that is clipped by the end of `query`
    lens = (1, 3, 5, 9, 11, 19)
    return dict(d=d, dummy=dummy, db=db, query=query, test_ids=test_ids, lens=lens,
                want=S.evaluate(query, db, dummy, test_ids, lens, k_probe=20))


@pytest.mark.parametrize('kind', ['flat', 'ivf', 'hnsw'])
def test_search_and_score_device_rank_equals_the_host_ranking_and_the_oracle(nafp, eval_case, kind):
    """All five returns of `search_and_score(device_rank=True)` equal those of the host ranking for each index class, built
    directly.  The oracle's evaluation (exact search in float64) is what the exact index must give, and what IVF-Flat gives when it
    probes all of its lists (the same rows are scanned); an HNSW search is approximate by construction, so it is held to the
    restatement fed with ITS OWN top-k ids instead -- as is every index."""
    from neural_audio_fp_amd.eval import eval_faiss as E
    c = eval_case
    if kind == 'flat':
        idx = E.FlatL2Index(c['d'])
    elif kind == 'ivf':
        from neural_audio_fp_amd.eval.ivf import IVFFlatIndex
        idx = IVFFlatIndex(c['d'], 16)
        idx.nprobe = 16
        idx.train(c['dummy'])
    else:
        from neural_audio_fp_amd.eval.hnsw import HNSWIndex
        idx = HNSWIndex(c['d'], 16)
        idx.efConstruction, idx.efSearch = 80, 64
    idx.add(c['dummy']); idx.add(c['db'])
    host = E.search_and_score(idx, c['query'], c['test_ids'], c['lens'], 20, len(c['dummy']), chunk_tasks=50)
    dev = E.search_and_score(idx, c['query'], c['test_ids'], c['lens'], 20, len(c['dummy']), chunk_tasks=50, device_rank=True)
    assert len(dev) == 5
    for h, g in zip(host, dev):
        assert h.shape == g.shape and h.dtype == g.dtype and np.array_equal(h, g)
    if kind in ('flat', 'ivf'):
        for w, g in zip(c['want'], dev):
            assert np.array_equal(w, g)
    table = np.concatenate([c['dummy'], c['db']])
    own = M.evaluate_with(c['query'], table, lambda q: idx.search(q, 20)[1], c['test_ids'], c['lens'], 20, len(c['dummy']))
    for w, g in zip(own, dev):
        assert np.array_equal(w, g)
    assert 0.05 < dev[0][:, 0].mean() < 0.99                               # the case is not trivial


def _write(out, arrays):
    for name, arr in arrays.items():
        mm = np.memmap(out + name + '.mm', dtype='float32', mode='w+', shape=arr.shape); mm[:] = arr; mm.flush()
        np.save(out + name + '_shape.npy', arr.shape)


def test_run_evaluate_with_and_without_the_switch(nafp, tmp_path):
    """`run.py evaluate` in child processes.  The command line fixes k_probe at 20, so the shape that exceeds the 2048 slots of the
    device ranking is a sequence length of 103 (2060 slots); `1 70` would be 1400 slots and is served by the device."""
    import yaml
    rng = np.random.default_rng(9)
    d = 128
    dummy, db = _unit(2000, d, 10), _unit(300, d, 11)
    noise = rng.choice([0.05, 0.8, 1.5], size=(300, 1))
    query = db + noise * rng.normal(size=db.shape) / np.sqrt(d) * 3
    query = (query / np.linalg.norm(query, axis=1, keepdims=True)).astype(np.float32)
    work = tmp_path / 'work'
    (work / 'config').mkdir(parents=True)
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'config', 'default.yaml')))
    cfg['DIR'].update({'OUTPUT_ROOT_DIR': str(work) + '/logs/emb/', 'LOG_ROOT_DIR': str(work) + '/logs/'})
    yaml.safe_dump(cfg, open(work / 'config' / 'tiny.yaml', 'w'))
    emb = work / 'logs' / 'emb' / 'EXP' / '1'
    emb.mkdir(parents=True)
    _write(str(emb) + '/', {'query': query, 'db': db, 'dummy_db': dummy})
    np.save(work / 'ids.npy', np.concatenate([np.arange(0, 190, 3), [297]]))       # the last one is clipped

    def evaluate(seq_len, switch):
        env = {k: v for k, v in os.environ.items() if k != 'NAFP_SEQ_MATCH'}
        env['PYTHONPATH'] = ROOT
        if switch:
            env['NAFP_SEQ_MATCH'] = '1'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), 'evaluate', 'EXP', '1', '-c', 'tiny', '-i', 'l2', '-t',
                            str(work / 'ids.npy'), '--test_seq_len', seq_len], cwd=work, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return open(emb / 'raw_score.npy', 'rb').read(), open(emb / 'index_used.json').read(), r.stderr

    raw_host, used_host, err_host = evaluate('1 3 5 9 11 19', False)
    raw_dev, used_dev, err_dev = evaluate('1 3 5 9 11 19', True)
    assert raw_host == raw_dev
    assert 'sequence_rank' not in used_host and json.loads(used_dev)['sequence_rank'] == 'device'
    rest = json.loads(used_dev)
    del rest['sequence_rank']
    assert rest == json.loads(used_host)
    assert 'NAFP_SEQ_MATCH' not in err_host and 'NAFP_SEQ_MATCH' not in err_dev
    hits = np.load(emb / 'raw_score.npy')
    assert hits.shape == (65, 24) and 0 < hits[:, 0].mean() < 1
    # 20 x 103 = 2060 slots: the notice, the host path, the same numbers as a run without the switch
    raw_long_host, used_long_host, _ = evaluate('1 103', False)
    raw_long, used_long, err_long = evaluate('1 103', True)
    assert 'NAFP_SEQ_MATCH=1' in err_long and 'host' in err_long
    assert raw_long == raw_long_host and used_long == used_long_host and 'sequence_rank' not in used_long
