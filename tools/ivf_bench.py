"""IVF-Flat / IVF-PQ against the exact search, on the device, nothing on disk (eval/ivf.py, csrc/ivf.hip).

Data: N clustered synthetic fingerprints, d = 128, unit norm: 20 000 random unit centres, each row = normalise(centre +
0.6 * unit Gaussian noise per row) (neighbouring rows of a centre sit at squared distance ~0.5, other centres at ~2, like
fingerprints of one song against the rest); queries = nq random rows with noise (0.3 per row, normalised again) -- the noisy
copies of eval_faiss.  Measures training time (the index's own seeded training subset), `add` rows/s with the rows already
on the device, the lazy list build, search time for nq queries (k = 20, nprobe = 40) for the exact index, IVF-Flat
(nlist 400), IVF-PQ (nlist 256, M 64, nbits 8) and IVFPQ-RR in the same process, and 1-recall@1 / 1-recall@20 of both approximate
indexes against the exact one (the exact nearest neighbour ranked first / within the top 20).  IVF-PQ is searched twice on
the one trained index, with fp32 ADC tables (`ivfpq_*`, the default) and with binary16 ones (`ivfpq_f16_*`, lut = 'f16'): same
queries, same process, the two precisions timed alternately.  IVFPQ-RR (`ivfpq_rr_*`: the same IVF-PQ plus 4 x 4-bit refine codes,
4 k first-stage candidates re-ranked) is trained with the same seed, so its coarse and PQ stages are IVF-PQ's bit for bit; on that
one index the plain k = 20 search (`IVFPQIndex.search_device`: the k <= 32 scan, `ivfpq_rr_plain_*`) and the two-stage search are
timed alternately for both table precisions, and the first stage alone (`nafp_ivf_pq_search_wide` at k1 = 80) once more.

`hnsw` mode: the HNSW graph index (eval/hnsw.py, csrc/hnsw.hip; M 16, efConstruction 80 as get_index sets it) on the same kind of
data: `add` + the round-based build in seconds, search ms per 1,000 queries at efSearch 16 and 64 (k = 20), and recall@1 / @10
against the exact index (the exact nearest neighbour ranked first / within the first 10).

`seqmatch` mode: the sequence ranking of the evaluation after the segment search, on the host (the default) and on the device
(`search_and_score(device_rank=True)`, nafp_search_seq_match).  Data: N unit-norm random rows, d = 128; T + 18 queries that are noisy
copies (0.3 per row, normalised again) of CONSECUTIVE rows, so that sequences exist to be found; test ids 0 .. T - 1, the default
lengths 1 3 5 9 11 19, k = 20, the exact index.  ONE search of all query rows; the index handed to `search_and_score` answers
`search_device` from that result, so what is timed is everything after the search.  The two paths alternate in one process, one
warm-up and `reps` timed calls each, synchronised before every clock read: the whole six-length call (what `evaluate` runs: the host
path builds 19 x 20 slots per task for every length), then each length in a call of its own (the host path then builds only
length x 20 slots).  Printed: the times, the mean n_cand / slots per length (the share of slots left after de-duplication), and
whether the two paths returned the same five arrays.

usage: python tools/ivf_bench.py [N=10000000] [nq=38000] [reps=3]   (one JSON line at the end)
       python tools/ivf_bench.py hnsw [N=200000] [nq=10000] [reps=3]   (N up to 1 M)
       python tools/ivf_bench.py seqmatch [N=1000000] [T=65536] [reps=3]"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neural_audio_fp_amd.eval.eval_faiss import FlatL2Index  # noqa: E402
from neural_audio_fp_amd import _lib  # noqa: E402
from neural_audio_fp_amd.eval.ivf import LUT_CODES, IVFFlatIndex, IVFPQIndex, IVFPQRIndex  # noqa: E402

args = sys.argv[1:]
mode = args[0] if args[:1] in (['hnsw'], ['seqmatch']) else 'ivf'
args = args[1:] if mode != 'ivf' else args
N = int(args[0]) if len(args) > 0 else {'hnsw': 200_000, 'seqmatch': 1_000_000, 'ivf': 10_000_000}[mode]
nq = int(args[1]) if len(args) > 1 else {'hnsw': 10_000, 'seqmatch': 65_536, 'ivf': 38_000}[mode]
reps = int(args[2]) if len(args) > 2 else 3
d, k, nprobe = 128, 20, 40


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def best_search(idx, q):
    idx.search_device(q[:256], k)
    times = []
    for _ in range(reps):
        dt, out = sync_time(lambda: idx.search_device(q, k))
        times.append(dt)
    return min(times), out


def seqmatch():
    import numpy as np
    from neural_audio_fp_amd.eval.eval_faiss import search_and_score
    T, lens, max_sl = nq, (1, 3, 5, 9, 11, 19), 19
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.empty((N, d), device='cuda')
    for a in range(0, N, 1 << 20):
        b = min(N, a + (1 << 20))
        x[a:b] = torch.nn.functional.normalize(torch.randn((b - a, d), generator=g, device='cuda'), dim=1)
    n_query = T + max_sl - 1
    if n_query > N:
        raise SystemExit(f'T + 18 = {n_query} query rows need at least as many table rows (N = {N})')
    start = (N - n_query) // 2
    q = torch.nn.functional.normalize(x[start:start + n_query] + 0.3 * torch.randn((n_query, d), generator=g, device='cuda') / d ** 0.5, dim=1).contiguous()
    ex = FlatL2Index(d, capacity=N)
    ex.add(x)
    ex.search_device(q[:256], k)
    search_s, (Dq, Iq) = sync_time(lambda: ex.search_device(q, k))

    class AfterTheSearch:
        """The exact index with the search already done: test ids 0 .. T - 1 touch the query rows 0 .. T + length - 2, in order."""
        d, device = ex.d, ex.device
        sequence_scores, sequence_match = ex.sequence_scores, ex.sequence_match

        def search_device(self, qq, kk):
            assert kk == k and torch.equal(qq, q[:qq.shape[0]])
            return Dq[:qq.shape[0]], Iq[:qq.shape[0]]

    idx, query, ids = AfterTheSearch(), q.cpu().numpy(), np.arange(T)
    res = {'mode': 'seqmatch', 'N': N, 'T': T, 'k': k, 'd': d, 'lengths': list(lens), 'reps': reps, 'search_s': search_s}

    def alternate(seq_lens):
        times, outs = {False: [], True: []}, {}
        for r in range(reps + 1):                                # r = 0: the warm-up of both
            for dev_rank in (False, True):
                dt, outs[dev_rank] = sync_time(lambda: search_and_score(idx, query, ids, seq_lens, k, start, device_rank=dev_rank))
                if r:
                    times[dev_rank].append(dt)
        same = all(np.array_equal(a, b) for a, b in zip(outs[False], outs[True]))
        return times[False], times[True], same, outs[True]

    host, dev, same, out = alternate(lens)
    res.update(host_s=min(host), device_s=min(dev), host_times_s=host, device_times_s=dev, outputs_equal=same,
               host_over_device=min(host) / min(dev), top1_exact_rate=[float(v) for v in out[0].mean(0)])
    print(f'six lengths, {T} tasks, after the search ({search_s:.3f} s): host ranking {min(host):.3f} s, device ranking {min(dev):.4f} s '
          f'({min(host) / min(dev):.1f} x), outputs equal: {same}', flush=True)
    q0, I32 = torch.arange(T, dtype=torch.int32, device='cuda'), Iq.to(torch.int32).contiguous()
    for sl in lens:
        host, dev, same_l, _ = alternate((sl,))
        n_cand = ex.sequence_match(q[:T + sl - 1], I32[:T + sl - 1], q0, torch.full_like(q0, sl), max_len=sl)[2]
        ratio = float(n_cand.float().mean()) / (sl * k)
        res[f'len{sl}'] = dict(host_s=min(host), device_s=min(dev), host_times_s=host, device_times_s=dev, outputs_equal=same_l,
                               n_cand_over_slots=ratio)
        same = same and same_l
        print(f'length {sl:2d}: host {min(host):.3f} s, device {min(dev):.4f} s, n_cand / slots {ratio:.3f}, outputs equal: {same_l}', flush=True)
    res['all_outputs_equal'] = same
    print(json.dumps(res))
    sys.exit(0 if same else 1)


if mode == 'seqmatch':
    seqmatch()

g = torch.Generator(device='cuda').manual_seed(0)
centres = torch.nn.functional.normalize(torch.randn((20000, d), generator=g, device='cuda'), dim=1)
x = torch.empty((N, d), device='cuda')
step = 1 << 20
for a in range(0, N, step):
    b = min(N, a + step)
    c = centres[torch.randint(0, 20000, (b - a,), generator=g, device='cuda')]
    x[a:b] = torch.nn.functional.normalize(c + 0.6 * torch.randn((b - a, d), generator=g, device='cuda') / d ** 0.5, dim=1)
pick = torch.randint(0, N, (nq,), generator=g, device='cuda')
q = torch.nn.functional.normalize(x[pick] + 0.3 * torch.randn((nq, d), generator=g, device='cuda') / d ** 0.5, dim=1).contiguous()

res = {'N': N, 'nq': nq, 'k': k, 'nprobe': nprobe, 'd': d}
ex = FlatL2Index(d, capacity=N)
ex.add(x)
res['exact_search_s'], (_, Ie) = best_search(ex, q)
print(f'exact: search {res["exact_search_s"]:.3f} s', flush=True)
del ex

if mode == 'hnsw':
    from neural_audio_fp_amd.eval.hnsw import HNSWIndex, round_bounds  # noqa: E402
    idx = HNSWIndex(d)
    idx.efConstruction = 80
    res['hnsw_add_s'], _ = sync_time(lambda: idx.add(x))
    res['hnsw_build_s'], _ = sync_time(idx.build)
    res['hnsw_rounds'] = len(round_bounds(0, N))
    res['hnsw_max_level'] = idx.max_level
    nn = Ie[:, :1]
    for efs in (16, 64):
        idx.efSearch = efs
        dt, (_, Ia) = best_search(idx, q)
        res[f'hnsw_ef{efs}_search_ms_per_1000'] = dt / nq * 1e6
        res[f'hnsw_ef{efs}_search_vs_exact'] = dt / res['exact_search_s']
        res[f'hnsw_ef{efs}_recall_at_1'] = float((Ia[:, :1] == nn).float().mean())
        res[f'hnsw_ef{efs}_recall_at_10'] = float((Ia[:, :10] == nn).any(1).float().mean())
        print(f'hnsw efSearch {efs}: {res[f"hnsw_ef{efs}_search_ms_per_1000"]:.2f} ms per 1,000 queries, recall@1 {res[f"hnsw_ef{efs}_recall_at_1"]:.4f}, '
              f'@10 {res[f"hnsw_ef{efs}_recall_at_10"]:.4f}', flush=True)
    print(f'hnsw: add {res["hnsw_add_s"]:.3f} s, build {res["hnsw_build_s"]:.2f} s ({res["hnsw_rounds"]} rounds, top level {res["hnsw_max_level"]})', flush=True)
    print(json.dumps(res))
    sys.exit(0)


def first_stage_only(idx, q, k1):
    """nafp_ivf_pq_search_wide on its own: the wide scan and its merge without the re-rank."""
    L, lib = idx._prepare(), idx._dev.lib
    D = torch.empty((q.shape[0], k1), dtype=torch.float32, device=q.device)
    I = torch.empty((q.shape[0], k1), dtype=torch.int32, device=q.device)
    need = int(lib.nafp_ivf_pq_wide_workspace_bytes(q.shape[0], idx.nlist, idx.nprobe, k1))
    ws = torch.empty((need,), dtype=torch.uint8, device=q.device)
    _lib.check(lib.nafp_ivf_pq_search_wide(_lib.ptr(q), q.shape[0], _lib.ptr(idx.centroids), idx.nlist, idx.d, idx.nprobe,
                                           _lib.ptr(idx.pq_centroids), idx.M, _lib.ptr(L['codes']), _lib.ptr(L['offsets']), _lib.ptr(L['ids']),
                                           k1, _lib.ptr(D), _lib.ptr(I), LUT_CODES[idx.lut], _lib.ptr(ws), need, _lib.current_stream()),
               'ivf_pq_search_wide')
    return D, I


for name, make in (('ivf', lambda: IVFFlatIndex(d, 400)), ('ivfpq', lambda: IVFPQIndex(d, 256, 64, 8)),
                   ('ivfpq_rr', lambda: IVFPQRIndex(d, 256, 64, 8, 4, 4))):
    idx = make()
    idx.nprobe = nprobe
    res[f'{name}_train_s'], _ = sync_time(lambda: idx.train(x))
    res[f'{name}_add_s'], _ = sync_time(lambda: idx.add(x))
    res[f'{name}_lists_s'], _ = sync_time(idx._prepare)
    res[f'{name}_add_rows_per_s'] = N / res[f'{name}_add_s']
    res[f'{name}_search_s'], (_, Ia) = best_search(idx, q)
    res[f'{name}_search_vs_exact'] = res[f'{name}_search_s'] / res['exact_search_s']
    nn = Ie[:, :1]
    res[f'{name}_recall_at_1'] = float((Ia[:, :1] == nn).float().mean())
    res[f'{name}_recall_at_20'] = float((Ia == nn).any(1).float().mean())
    if name == 'ivfpq':                                        # the two table precisions in turn, reps times: the best of each
        times = {'f32': [res['ivfpq_search_s']], 'f16': []}
        for lut in ['f16', 'f32'] * reps:
            idx.lut = lut
            idx.search_device(q[:256], k)
            dt, (_, Il) = sync_time(lambda: idx.search_device(q, k))
            times[lut].append(dt)
            if lut == 'f16':
                Ih = Il
        res['ivfpq_search_s'] = min(times['f32'])
        res['ivfpq_search_vs_exact'] = res['ivfpq_search_s'] / res['exact_search_s']
        res['ivfpq_f16_search_s'] = min(times['f16'])
        res['ivfpq_f16_search_vs_exact'] = res['ivfpq_f16_search_s'] / res['exact_search_s']
        res['ivfpq_f16_search_vs_f32'] = res['ivfpq_f16_search_s'] / res['ivfpq_search_s']
        res['ivfpq_search_times_s'] = times
        res['ivfpq_f16_recall_at_1'] = float((Ih[:, :1] == nn).float().mean())
        res['ivfpq_f16_recall_at_20'] = float((Ih == nn).any(1).float().mean())
        res['ivfpq_f16_same_top1_as_f32'] = float((Ih[:, 0] == Ia[:, 0]).float().mean())
        print(f'ivfpq, fp16 tables: search {res["ivfpq_f16_search_s"]:.3f} s ({res["ivfpq_f16_search_vs_exact"]:.2f} x exact, '
              f'{res["ivfpq_f16_search_vs_f32"]:.2f} x fp32 tables at {res["ivfpq_search_s"]:.3f} s), 1-recall@1 {res["ivfpq_f16_recall_at_1"]:.4f}, '
              f'@20 {res["ivfpq_f16_recall_at_20"]:.4f}, top-1 equal to fp32 tables for {res["ivfpq_f16_same_top1_as_f32"]:.4f}', flush=True)
    if name == 'ivfpq_rr':                                     # plain k = 20 scan and two-stage search, fp32 / fp16 tables, in turn
        runs = {('plain', 'f32'): [], ('plain', 'f16'): [], ('rr', 'f32'): [res['ivfpq_rr_search_s']], ('rr', 'f16'): []}
        found = {}
        for kind, lut in list(runs) * reps:
            idx.lut = lut
            fn = (lambda: IVFPQIndex.search_device(idx, q, k)) if kind == 'plain' else (lambda: idx.search_device(q, k))
            IVFPQIndex.search_device(idx, q[:256], k) if kind == 'plain' else idx.search_device(q[:256], k)
            dt, (_, Il) = sync_time(fn)
            runs[(kind, lut)].append(dt)
            found[(kind, lut)] = Il
        for (kind, lut), ts in runs.items():
            key = f'ivfpq_rr_{"plain_" if kind == "plain" else ""}{lut}'
            res[f'{key}_search_s'] = min(ts)
            res[f'{key}_search_times_s'] = ts
            res[f'{key}_recall_at_1'] = float((found[(kind, lut)][:, :1] == nn).float().mean())
            res[f'{key}_recall_at_20'] = float((found[(kind, lut)] == nn).any(1).float().mean())
        for lut in ('f32', 'f16'):
            idx.lut = lut
            first_stage_only(idx, q[:256], 4 * k)
            res[f'ivfpq_rr_{lut}_first_stage_s'] = min(sync_time(lambda: first_stage_only(idx, q, 4 * k))[0] for _ in range(reps))
            res[f'ivfpq_rr_{lut}_vs_plain'] = res[f'ivfpq_rr_{lut}_search_s'] / res[f'ivfpq_rr_plain_{lut}_search_s']
            res[f'ivfpq_rr_{lut}_first_stage_vs_plain'] = res[f'ivfpq_rr_{lut}_first_stage_s'] / res[f'ivfpq_rr_plain_{lut}_search_s']
            print(f'ivfpq_rr, {lut} tables: two-stage search {res[f"ivfpq_rr_{lut}_search_s"]:.3f} s = {res[f"ivfpq_rr_{lut}_vs_plain"]:.3f} x the plain '
                  f'k = {k} search of the same index ({res[f"ivfpq_rr_plain_{lut}_search_s"]:.3f} s); first stage alone {res[f"ivfpq_rr_{lut}_first_stage_s"]:.3f} s; '
                  f'1-recall@1 {res[f"ivfpq_rr_{lut}_recall_at_1"]:.4f} (plain {res[f"ivfpq_rr_plain_{lut}_recall_at_1"]:.4f}), '
                  f'@20 {res[f"ivfpq_rr_{lut}_recall_at_20"]:.4f} (plain {res[f"ivfpq_rr_plain_{lut}_recall_at_20"]:.4f})', flush=True)
        idx.lut = 'f32'
    print(f'{name}: train {res[f"{name}_train_s"]:.2f} s, add {res[f"{name}_add_s"]:.3f} s ({res[f"{name}_add_rows_per_s"] / 1e6:.1f} M rows/s) '
          f'+ lists {res[f"{name}_lists_s"]:.3f} s, search {res[f"{name}_search_s"]:.3f} s ({res[f"{name}_search_vs_exact"]:.2f} x exact), '
          f'1-recall@1 {res[f"{name}_recall_at_1"]:.4f}, @20 {res[f"{name}_recall_at_20"]:.4f}', flush=True)
    del idx
    torch.cuda.empty_cache()
print(json.dumps(res))
