"""Generate throughput from 44.1 kHz stereo files (NAFP_RESAMPLE=1) next to the same content as 8 kHz mono files.

    python tools/resample_bench.py [n_files=2000] [work_dir=/tmp/nafp_resample_bench] [--no-profile]

Writes n_files synthetic 30-s clips as 44.1 kHz stereo WAVs and -- converted by the library's own resampler, which the tests
hold equal to the integer contract -- as 8 kHz mono WAVs, then, all from page cache:
  * `python run.py generate NAME --source DIR` on each set (wall time of the whole command, start-up included);
  * write_fingerprints over each set in this process, best of 2 passes (the steady state: segments/s);
  * one `rocprofv3 --kernel-trace --stats` pass of `run.py generate` on the 44.1 kHz set: the resample kernel's share of the
    kernel time, and its achieved filter taps/s.
One JSON line at the end.  The fingerprints of the two sets are compared byte for byte on the way."""
import csv
import json
import os
import shutil
import subprocess
import sys
import time
import wave

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

args = [a for a in sys.argv[1:] if not a.startswith('--')]
n_files = int(args[0]) if args else 2000
work = args[1] if len(args) > 1 else '/tmp/nafp_resample_bench'
FS_IN, SECONDS = 44100, 30


def write_wav(path, pcm, fs, ch):
    with wave.open(path, 'w') as w:
        w.setnchannels(ch); w.setsampwidth(2); w.setframerate(fs)
        w.writeframes(pcm.astype('<i2').tobytes())


def prepare():
    os.environ['NAFP_RESAMPLE'] = '1'
    from neural_audio_fp_amd.model.utils import resample as rs
    from neural_audio_fp_amd.model import generate as g
    for sub in ('src44', 'src8', 'config'):
        os.makedirs(os.path.join(work, sub), exist_ok=True)
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'config', 'default.yaml')))
    cfg['DIR']['LOG_ROOT_DIR'] = work + '/logs/'
    cfg['DIR']['OUTPUT_ROOT_DIR'] = work + '/logs/emb/'
    yaml.safe_dump(cfg, open(os.path.join(work, 'config', 'bench.yaml'), 'w'))
    m_pre, m_fp = g.build_fp(cfg)
    g.save_checkpoint(cfg['DIR']['LOG_ROOT_DIR'] + 'checkpoint/', 'bench', 1, m_fp)
    rng = np.random.default_rng(7)
    n = FS_IN * SECONDS
    t = np.arange(n) / FS_IN
    base = rng.integers(-6000, 6000, size=(n, 2)).astype(np.float64)
    for f in rng.uniform(200, 3900, size=5):
        base += 3500 * np.sin(2 * np.pi * f * t + rng.uniform(0, 6, size=2)[None, :].T).T
    base = np.clip(base, -32768, 32767).astype(np.int16)
    plan = rs.plan_for(FS_IN, 8000)
    n_out = rs.n_out(n, FS_IN, 8000)
    piece = np.array([(0, 0, n, n, 0, 0, n_out, 2)], dtype=rs.PIECE_DTYPE)
    t0 = time.perf_counter()
    for k in range(n_files):
        p44, p8 = os.path.join(work, 'src44', f'{k:05d}.wav'), os.path.join(work, 'src8', f'{k:05d}.wav')
        if os.path.exists(p44) and os.path.exists(p8):
            continue
        x = np.roll(base, 1009 * k, axis=0)                        # distinct files, one synthesis
        x[:, 1] = np.roll(x[:, 1], 37 * k)
        write_wav(p44, x.reshape(-1), FS_IN, 2)
        out = torch.empty((n_out,), dtype=torch.int16, device='cuda')
        plan.run(torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).cuda(), piece, out)
        write_wav(p8, out.cpu().numpy(), 8000, 1)
    print(f'{n_files} clips x 2 ready in {time.perf_counter() - t0:.1f} s', flush=True)
    return cfg, m_pre, m_fp


def steady_state(cfg, m_pre, m_fp, sub, switch):
    from neural_audio_fp_amd.model import generate as g
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    os.environ['NAFP_RESAMPLE'] = '1' if switch else '0'
    d = os.path.join(work, sub)
    paths = sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith('.wav'))[:n_files]
    src = SegmentSource(paths, bsz=cfg['BSZ']['TS_BATCH_SZ'])
    arr = np.zeros((src.n_samples, cfg['MODEL']['EMB_SZ']), np.float32)
    emb = g.StreamedEmbedder(m_pre, m_fp)
    rates = []
    for rep in range(3):                                           # the first pass warms the pinned arenas up
        torch.cuda.synchronize(); t0 = time.perf_counter()
        g.write_fingerprints(src, emb, arr, cfg['BSZ']['TS_BATCH_SZ'])
        rates.append(src.n_samples / (time.perf_counter() - t0))
    return src.n_samples, rates[1:], arr


def run_py(sub, switch, profile_dir=None):
    env = dict(os.environ, NAFP_RESAMPLE='1' if switch else '0')
    cmd = [sys.executable, os.path.join(ROOT, 'run.py'), 'generate', 'bench', '-c', 'bench', '-s', os.path.join(work, sub),
           '-o', os.path.join(work, 'out_' + sub)]
    if profile_dir:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', profile_dir, '-o', 't', '--'] + cmd
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=work, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f'{" ".join(cmd)} failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
    return time.perf_counter() - t0


def kernel_share(profile_dir):
    path = None
    for d, _, files in os.walk(profile_dir):
        for f in files:
            if f.endswith('kernel_stats.csv'):
                path = os.path.join(d, f)
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r['TotalDurationNs']) for r in rows)
    mine = [r for r in rows if 'resample_i16_kernel' in r['Name']]
    ns = sum(float(r['TotalDurationNs']) for r in mine)
    return {'resample_kernel_ms': ns / 1e6, 'all_kernels_ms': total / 1e6, 'share': ns / total,
            'calls': sum(int(r['Calls']) for r in mine)}


if __name__ == '__main__':
    from neural_audio_fp_amd.model.utils import resample as rs
    cfg, m_pre, m_fp = prepare()
    res = {'n_files': n_files, 'seconds_per_file': SECONDS, 'device': torch.cuda.get_device_name(0)}
    n_seg, r8, a8 = steady_state(cfg, m_pre, m_fp, 'src8', False)
    _, r44, a44 = steady_state(cfg, m_pre, m_fp, 'src44', True)
    _, r8b, _ = steady_state(cfg, m_pre, m_fp, 'src8', False)
    res.update(segments=n_seg, segments_per_s_8k_mono=[round(x) for x in r8 + r8b], segments_per_s_44k_stereo=[round(x) for x in r44],
               fingerprints_identical=bool(a8.tobytes() == a44.tobytes()))
    res['run_py_wall_s_8k_mono'] = round(run_py('src8', False), 2)
    res['run_py_wall_s_44k_stereo'] = round(run_py('src44', True), 2)
    if '--no-profile' not in sys.argv:
        prof = os.path.join(work, 'prof')
        shutil.rmtree(prof, ignore_errors=True)
        run_py('src44', True, prof)
        k = kernel_share(prof)
        L, M, half, T = rs.geometry(FS_IN, 8000)
        outputs = n_files * rs.n_out(FS_IN * SECONDS, FS_IN, 8000)       # every output once per file: launches overlap by half a window at most
        k['taps_per_s_lower_bound'] = outputs * T / (k['resample_kernel_ms'] / 1e3)
        res['profile'] = k
    print(json.dumps(res))
