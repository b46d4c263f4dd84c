"""Throughput of the device-side training loader: batches of 640 anchors + 640 augmented replicas
(bg mix at random SNR + 600-tap IR + normalisation) from a synthetic corpus resident in HBM.
usage: python tools/loader_bench.py [n_clips=300] [--speed LO HI N]

--speed LO HI N: after the figures above, the kernel time per batch of a loader whose replicas are played at a speed drawn from the grid
of N speeds over [LO, HI] (speed_mix_parameter): (a) the batch without speed rows, (b) the speed rows inside the batch kernel
(nafp_augment_rows_speed), (c) the same rows through the two separate kernels -- one nafp_varispeed_i16 launch per step into a scratch
arena, then nafp_augment_rows.  One process, the three alternated, tables uploaded beforehand, medians over the repetitions."""
import os
import sys
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neural_audio_fp_amd.model.utils.dataloader_keras import genUnbalSequence  # noqa: E402

argv, speed = sys.argv[1:], None
if '--speed' in argv:
    k = argv.index('--speed')
    speed = [True, (float(argv[k + 1]), float(argv[k + 2])), int(argv[k + 3])]
    del argv[k:k + 4]
n_clips = int(argv[0]) if argv else 300
d = '/tmp/nafp_loader'
rng = np.random.default_rng(0)


def mk(sub, n, length, scale):
    os.makedirs(f'{d}/{sub}', exist_ok=True)
    out = []
    for k in range(n):
        p = f'{d}/{sub}/{k:05d}.wav'
        if not os.path.exists(p):
            with wave.open(p, 'w') as w:
                w.setnchannels(1); w.setsampwidth(2); w.setframerate(8000)
                w.writeframes((scale * rng.normal(size=length)).astype('<i2').tobytes())
        out.append(p)
    return out


ev, bg, ir = mk('ev', n_clips, 240000, 3000), mk('bg', 40, 80000, 2000), mk('ir', 60, 4000, 500)
t0 = time.perf_counter()
ds = genUnbalSequence(ev, bsz=1280, n_anchor=640, shuffle=True, random_offset_anchor=True,
                      bg_mix_parameter=[True, bg, (0, 10)], ir_mix_parameter=[True, ir], seed=1)
ds._resident(); torch.cuda.synchronize()
print(f'{len(ev) + len(bg) + len(ir)} files, {ds.arena.total * 2 / 1e6:.0f} MB of PCM resident after {time.perf_counter() - t0:.2f} s; '
      f'{len(ds)} batches per epoch')
for rep in range(3):
    t0 = time.perf_counter(); tp = 0.0
    n = min(len(ds), 20)
    for i in range(n):
        a = time.perf_counter(); rows = ds.plan(i); tp += time.perf_counter() - a
        out = ds.run(rows)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); ds.run(rows); e1.record(); torch.cuda.synchronize()
    print(f'batch of 1280 rows: {dt * 1e3:.2f} ms wall ({tp / n * 1e3:.2f} ms host plan, {e0.elapsed_time(e1):.3f} ms kernel+upload) '
          f'= {1280 / dt:.0f} segments/s')


if speed:
    from neural_audio_fp_amd import _lib  # noqa: E402
    from neural_audio_fp_amd.model.utils import varispeed as vs  # noqa: E402
    dss = genUnbalSequence(ev, bsz=1280, n_anchor=640, shuffle=True, random_offset_anchor=True, bg_mix_parameter=[True, bg, (0, 10)],
                           ir_mix_parameter=[True, ir], seed=1, speed_mix_parameter=speed)
    dss._pcm, dss._lib = ds._pcm, ds._lib                     # the same files in the same places: one resident arena
    lib, pcm, T = ds._lib, ds._pcm, ds.seg_len
    print(f'speed grid {[round(x, 4) for x in dss.speed_grid]}: {len(dss.speed_steps)} steps other than unity')
    rows, speeds = dss.plan(0), dss.check_speed(dss.plan(0), dss.plan_speed(0))
    n_speed = int((speeds['slot'] >= 0).sum())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(pcm.device)
    # (c): the arena with a scratch window per row behind it; the speed rows' events rendered there, one piece list per step
    both = torch.cat([pcm, torch.zeros((len(rows) * T,), dtype=torch.int16, device=pcm.device)])
    scratch = both[pcm.numel():]
    rows_c, pieces = rows.copy(), {}
    for i in np.flatnonzero(speeds['slot'] >= 0):
        e = speeds[i]
        step = dss.speed_steps[e['slot']]
        cnt = int(np.clip(vs.n_out(int(e['n_in']), step) - int(e['out0']), 0, T))
        rows_c['ev_off'][i], rows_c['ev_valid'][i] = pcm.numel() + i * T, cnt
        if cnt:
            pieces.setdefault(step, []).append((int(e['file_off']), 0, int(e['n_in']), int(e['n_in']), int(e['out0']), i * T, cnt, 0))
    pieces = {st: vs.check_pieces(st, np.asarray(p, dtype=vs.PIECE_DTYPE), pcm.numel(), scratch.numel()) for st, p in pieces.items()}
    d_pieces = {st: up(p) for st, p in pieces.items()}
    plans = {st: vs.plan_for(st, pcm.device) for st in pieces}
    d_rows, d_rows_c, d_speeds = up(rows), up(rows_c), up(speeds)
    out_a, out_b, out_c = (torch.empty((len(rows), T), dtype=torch.float32, device=pcm.device) for _ in range(3))
    st = _lib.current_stream

    def run_a():
        _lib.check(lib.nafp_augment_rows(_lib.ptr(pcm), _lib.ptr(d_rows), len(rows), T, _lib.ptr(out_a), st()), 'augment_rows')

    def run_b():
        _lib.check(lib.nafp_augment_rows_speed(dss.speedset(), _lib.ptr(pcm), pcm.numel(), _lib.ptr(d_rows), _lib.ptr(d_speeds), len(rows), T,
                                               _lib.ptr(out_b), st()), 'augment_rows_speed')

    def run_c():
        for step, p in pieces.items():
            _lib.check(lib.nafp_varispeed_i16(plans[step].handle, _lib.ptr(pcm), pcm.numel(), _lib.ptr(d_pieces[step]), len(p),
                                              _lib.ptr(scratch), scratch.numel(), st()), 'varispeed_i16')
        _lib.check(lib.nafp_augment_rows(_lib.ptr(both), _lib.ptr(d_rows_c), len(rows), T, _lib.ptr(out_c), st()), 'augment_rows')

    cases = [('a', run_a), ('b', run_b), ('c', run_c)]
    for _, fn in cases:                                       # first launches: table upload, function attributes, clocks
        fn(); fn()
    torch.cuda.synchronize()
    print(f'(b) equals (c) byte for byte: {bool(torch.equal(out_b.view(torch.int32), out_c.view(torch.int32)))}; '
          f'{n_speed} of {len(rows)} rows are speed rows, {len(pieces)} varispeed launches in (c)')
    reps, inner = 9, 10
    ms = {k: [] for k, _ in cases}
    for rep in range(reps):
        for k, fn in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / inner)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for k, what in (('a', 'no speed rows (nafp_augment_rows)'), ('b', 'speed rows in the batch kernel'), ('c', 'varispeed launches + nafp_augment_rows')):
        print(f'({k}) {what}: median {med[k]:.4f} ms per batch of {len(rows)} rows (min {min(ms[k]):.4f}, max {max(ms[k]):.4f}, {reps} x {inner} launches)')
    print(f"b/a {med['b'] / med['a']:.3f}   b/c {med['b'] / med['c']:.3f}")
    # whole batches through the loader (host plan + upload + kernel), with and without the option, alternated
    wall = {'off': [], 'on': []}
    for rep in range(5):
        for k, d_ in (('off', ds), ('on', dss)):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(min(len(ds), 10)):
                d_[i]
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) / min(len(ds), 10) * 1e3)
    print(f"ds[i] wall per batch: {np.median(wall['off']):.2f} ms without, {np.median(wall['on']):.2f} ms with the option")
