"""Do fingerprints survive a real time-stretch inside a one-second segment?  ONE measurement on the CPU oracle, untrained weights.

    python tools/tempo_stretch_probe.py [--seed 0] [--tempo 1.04] [--hypotheses 1.04 1.03 1]

A score of tone bursts (decaying partials at random pitches, a new note every 0.12 .. 0.45 s) is rendered twice: at tempo 1, 40 s,
the library track; and from its second 5 on at `--tempo`, 12 s, the recording -- the same pitches, every onset and every duration
divided by the tempo.  That is what a time-stretcher aims at (tempo changed, pitch kept) without any stretcher's artefacts.  Both
are cut into 1-s segments every 0.5 s and fingerprinted by the oracle (oracle/melspec.py with each segment normalised by its own
maximum, oracle/nnfp.py in float32, freshly initialised weights).  Segment i of the recording then shows what library row
10 + tempo * i shows, but 4 % compressed inside the segment.  Printed per hypothesis rho: the score of the 20-segment window along
the line a + ((i * rho + 32768) >> 16) (the arithmetic of nafp_search_identify_tempo) at the true a = 10 and at the best a.
No GPU, no library: numpy only.  Nothing is asserted and nothing is claimed about trained weights."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS = 8000


def score_of_notes(rng, seconds):
    """[(onset s, duration s, pitch Hz, level)] at tempo 1."""
    notes, t = [], 0.0
    while t < seconds:
        notes.append((t, float(rng.uniform(0.15, 0.6)), float(rng.uniform(320, 1800)), float(rng.uniform(0.4, 1.0))))
        t += float(rng.uniform(0.12, 0.45))
    return notes


def render(notes, t0, seconds, tempo):
    """`seconds` of audio from score time t0 on, played at `tempo`: onsets and durations divided by it, pitches kept."""
    n = int(seconds * FS)
    x = np.zeros(n)
    for onset, dur, f, level in notes:
        start, dur = (onset - t0) / tempo, dur / tempo
        i0, i1 = int(np.ceil(start * FS)), int((start + 4 * dur) * FS)
        if i1 <= 0 or i0 >= n:
            continue
        i = np.arange(max(i0, 0), min(i1, n))
        u = i / FS - start                                         # seconds since the onset
        env = np.minimum(u / (0.004 / tempo), 1.0) * np.exp(-u / dur)
        x[i] += level * env * (np.sin(2 * np.pi * f * u) + 0.5 * np.sin(2 * np.pi * 2 * f * u) + 0.25 * np.sin(2 * np.pi * 3 * f * u))
    return np.round(8000 * x).clip(-32768, 32767)


def fingerprints(pcm, w):
    from oracle import melspec as o_mel
    from oracle import nnfp as o_nnfp
    segs = np.stack([pcm[s:s + FS] for s in range(0, len(pcm) - FS + 1, FS // 2)]) / 32768.0
    feat = o_mel.melspec_layer(segs[:, None, :], group_size=1, dtype=np.float32)
    return o_nnfp.fingerprinter(feat, w, dtype=np.float32).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--tempo', type=float, default=1.04)
    ap.add_argument('--hypotheses', type=float, nargs='+', default=[1.04, 1.03, 1.0])
    a = ap.parse_args()
    from oracle import nnfp as o_nnfp
    rng = np.random.default_rng(a.seed)
    notes = score_of_notes(rng, 42.0)
    w = o_nnfp.init_weights(seed=a.seed)
    x = fingerprints(render(notes, 0.0, 40.0, 1.0), w)
    q = fingerprints(render(notes, 5.0, 12.0, a.tempo), w)[:20]
    print(f'library {len(x)} rows, recording window {len(q)} segments at tempo {a.tempo}, true alignment 10', flush=True)
    for tempo in a.hypotheses:
        rho = int(round(65536 * tempo))
        off = (np.arange(len(q), dtype=np.int64) * rho + 32768) >> 16
        s = np.array([float(np.mean(np.sum(q * x[al + off], axis=1))) for al in range(len(x) - int(off[-1]))])
        print(f'hypothesis {tempo:.2f} (rho {rho}): score {s[10]:.4f} at the true alignment, best {s.max():.4f} at alignment {int(s.argmax())}; '
              f'the best elsewhere (more than 2 rows away) {np.delete(s, range(8, 13)).max():.4f}', flush=True)


if __name__ == '__main__':
    main()
