"""Time of the identification matcher (nafp_search_identify) per 1,000 windows, on synthetic fingerprints held on the device.

    python tools/identify_bench.py [--dim 128] [--tasks 1000] [--reps 5] [--cpu] [--tempos N [N ...]]

Three shapes: the default window (20 segments x k = 20), 8192 slots with k = 32 (256 segments) and 8192 slots with k = 1.
The library is 100,000 random unit rows in tracks of 60; every window holds one planted run (the recording is a noisy copy of
library rows) in a background of random ids, so the candidate lists are as long as a search over unrelated material makes them.
Not bench.py and not part of the contract: there is no earlier path to compare with, the figures are recorded in README.md.
`--cpu` times the numpy restatement of the tests on this host instead (no GPU needed; orientation only: a CPU figure).
`--tempos N ...` times the default window only: nafp_search_identify, then nafp_search_identify_tempo under N hypotheses (the N
nearest 1 of a 0.01 grid, n_short = min(256, 32 N) as `identify --tempos` sets it) on the same windows in the same run."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def make(rng, d, n_index, track_len, n_tasks, k, length):
    x = rng.normal(size=(n_index, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    first = np.arange(0, n_index + 1, track_len, dtype=np.int32)
    n_rows = min(n_tasks * length, 1 << 16)                           # the windows share query rows beyond 65,536
    topk = rng.integers(0, n_index, size=(n_rows, k)).astype(np.int32)
    start = rng.integers(0, n_index - n_rows)
    topk[:, 0] = start + np.arange(n_rows)                            # the planted run: the recording is rows start .. of the library
    q = x[topk[:, 0]] + 0.05 * rng.normal(size=(n_rows, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q0 = (rng.integers(0, max(n_rows - length, 0) + 1, size=n_tasks)).astype(np.int32)
    return x, first, q.astype(np.float32), topk, q0, np.full(n_tasks, length, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--tasks', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu', action='store_true')
    ap.add_argument('--tempos', type=int, nargs='+', default=None)
    a = ap.parse_args()
    from neural_audio_fp_amd.eval.eval_faiss import FlatL2Index
    rng = np.random.default_rng(0)

    def timed(run):
        run()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return np.median(times) * 1000 / a.tasks

    if a.tempos:
        from neural_audio_fp_amd.eval.identify import parse_tempos
        x, first, q, topk, q0, ln = make(rng, a.dim, 100000 // 60 * 60, 60, a.tasks, 20, 20)
        index = FlatL2Index(a.dim)
        index.add(x)
        dev = [torch.from_numpy(v).cuda() for v in (q, topk, q0, ln)]
        kw = dict(n_out=1, min_overlap=4, min_votes=2, max_len=20)
        ms = timed(lambda: index.identify(*dev, first, n_short=32, **kw))
        print(f'20 x 20, nafp_search_identify, d {a.dim}: {ms:9.3f} ms per 1,000 windows (median of {a.reps}, {a.tasks} windows per launch)', flush=True)
        for n in a.tempos:
            rhos = parse_tempos('0.93:1.08:0.01')[:n]
            assert len(rhos) == n, '--tempos: 1 .. 16'
            run = lambda: index.identify_tempo(*dev, first, rhos, n_short=min(256, 32 * n), **kw)
            ms, out = timed(run), run()
            hit = float(((out[1][:, 0].cpu().numpy() == topk[q0, 0]) & (out[6][:, 0].cpu().numpy() == 0)).mean())
            print(f'20 x 20, nafp_search_identify_tempo, {n} hypotheses ({min(rhos) / 65536:.2f} .. {max(rhos) / 65536:.2f}), d {a.dim}: {ms:9.3f} ms '
                  f'per 1,000 windows (median of {a.reps}, {a.tasks} windows per launch; planted alignment found at tempo 1 in {100 * hit:.0f} %)', flush=True)
        return
    for name, k, length in (('20 x 20 (default)', 20, 20), ('8192 slots, k = 32', 32, 256), ('8192 slots, k = 1', 1, 8192)):
        x, first, q, topk, q0, ln = make(rng, a.dim, 100000 // 60 * 60, 60, a.tasks, k, length)
        if a.cpu:
            import _identify_ref as R
            n = min(a.tasks, 20)
            t0 = time.perf_counter()
            R.identify(topk, q0[:n], ln[:n], length, len(q), len(x), first, R.score_f64(q, x), 4, 2, 32, 1)
            print(f'{name:<20s} d {a.dim}: numpy restatement on this host {(time.perf_counter() - t0) / n * 1000:9.1f} s per 1,000 windows '
                  f'(CPU, {n} windows timed)', flush=True)
            continue
        index = FlatL2Index(a.dim)
        index.add(x)
        dev = [torch.from_numpy(v).cuda() for v in (q, topk, q0, ln)]
        run = lambda: index.identify(*dev, first, n_out=1, n_short=32, min_overlap=4, min_votes=2, max_len=length)
        ms, out = timed(run), run()
        hit = float((out[1][:, 0].cpu().numpy() == topk[q0, 0]).mean())
        print(f'{name:<20s} d {a.dim}: {ms:9.3f} ms per 1,000 windows (median of {a.reps}, {a.tasks} windows per launch; '
              f'planted alignment found in {100 * hit:.0f} %)', flush=True)
        del index


if __name__ == '__main__':
    main()
