"""Time of the masked exact search (nafp_search_topk_l2_excl) as `duplicates` launches it, against nafp_search_topk_l2 on the same
arrays in the same process.

    python tools/search_excl_bench.py [--dim 128] [--rows 262144] [--track 400] [--k 20] [--reps 5]

One MI355X; a synthetic library of `--rows` random unit rows in tracks of `--track` rows, every row a query: the masked search
with each row's own track as its range, and the unmasked search of the same queries.  The two are warmed up, then alternated,
each repetition timed with device events; the medians, their ratio and the rate 2 N^2 d / time are printed.  Not bench.py and
not part of the contract: there is no gate, the ratio of one run is recorded in README.md and DESIGN.md as what it is.
The own track is where a self-join differs from a search of foreign queries: its rows beat the k-th best of their query, so the
blocks that hold them take the insertion branch, masked or not."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--rows', type=int, default=262144)
    ap.add_argument('--track', type=int, default=400)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    from neural_audio_fp_amd.eval.eval_faiss import FlatL2Index
    n, d = a.rows, a.dim
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn((n, d), generator=g, device='cuda', dtype=torch.float32)
    x /= x.norm(dim=1, keepdim=True)
    index = FlatL2Index(d)
    index.add(x)
    first = np.minimum(np.arange(0, n + a.track, a.track), n)
    first = np.unique(first).astype(np.int64)
    tr = np.searchsorted(first, np.arange(n), side='right') - 1
    excl = torch.from_numpy(np.stack([first[tr], first[tr + 1]], 1).astype(np.int32)).cuda()
    q = index._x[:n]                                                 # the resident rows themselves

    masked = lambda: index.search_device_excl(q, a.k, excl)
    plain = lambda: index.search_device(q, a.k)
    for run in (masked, plain):                                      # warm-up: code objects, the half norms, the allocator
        run()
    torch.cuda.synchronize()
    times = {'masked': [], 'plain': []}
    for _ in range(a.reps):
        for name, run in (('masked', masked), ('plain', plain)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = run()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
            if name == 'masked':
                ids = out[1]
    own = ((ids >= excl[:, :1]) & (ids < excl[:, 1:])).any().item()
    assert not own, 'a row of the own track was returned'
    tm, tp = float(np.median(times['masked'])), float(np.median(times['plain']))
    flop = 2.0 * n * n * d
    print(f'{n} rows in tracks of {a.track}, d {d}, k {a.k}, every row a query, median of {a.reps} alternated runs:', flush=True)
    print(f'  nafp_search_topk_l2_excl (own track excluded): {tm:9.2f} ms  {flop / tm / 1e9:7.1f} TFLOP/s', flush=True)
    print(f'  nafp_search_topk_l2      (same arrays)       : {tp:9.2f} ms  {flop / tp / 1e9:7.1f} TFLOP/s', flush=True)
    print(f'  masked / unmasked: {tm / tp:.3f}', flush=True)


if __name__ == '__main__':
    main()
