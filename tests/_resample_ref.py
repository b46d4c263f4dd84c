"""numpy restatement of the resampler's contract (include/nafp.h): the float64 filter design and
the int64 convolution.  Nothing here calls the library."""
import math

import numpy as np

BETA, ZEROS, CUT = 8.6, 32, 0.95


def geometry(fs_in, fs_out=8000):
    g = math.gcd(fs_in, fs_out)
    L, M = fs_out // g, fs_in // g
    if fs_in == fs_out:
        return 1, 1, 0, 1
    fv = fs_in * L
    half = -(-(ZEROS * 20 * fv) // (19 * fs_out))           # ceil(32 fv / (2 fc)), fc = 0.95 fs_out / 2, in integers
    return L, M, half, -(-(2 * half + 1) // L)


def design(fs_in, fs_out=8000):
    """hq[v + half], v in [-half, half], int64."""
    L, M, half, T = geometry(fs_in, fs_out)
    if half == 0:
        return np.array([1 << 30], np.int64)
    v = np.arange(-half, half + 1, dtype=np.float64)
    r = CUT * fs_out / (float(fs_in) * L)                   # 2 fc / fv
    h = np.sinc(r * v) * np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (v / half) ** 2))) / np.i0(BETA) * r * L
    return np.rint(h * 2.0 ** 30).astype(np.int64)


def table(fs_in, fs_out=8000):
    """[phase p][tap t] = hq[p + t L - half], zero where out of range."""
    L, M, half, T = geometry(fs_in, fs_out)
    flat = np.zeros(L * T, np.int64)
    hq = design(fs_in, fs_out)
    flat[:len(hq)] = hq                                     # index p + t L
    return np.ascontiguousarray(flat.reshape(T, L).T)


def n_out(n_in, fs_in, fs_out=8000):
    L, M, _, _ = geometry(fs_in, fs_out)
    return -(-(n_in * L) // M)


def mono(x):
    x = np.asarray(x, np.int64)
    return x if x.ndim == 1 else x.sum(axis=1)


def finish(acc, channels):
    s = 30 if channels == 1 else 31
    return np.clip((acc + (1 << (s - 1))) >> s, -32768, 32767).astype(np.int16)


def accumulate(x, fs_in, fs_out=8000, tab=None):
    """acc[n] for every output of the file x ((n,) or (n, 2) int16), from the canonical table `tab` (default: this design)."""
    L, M, half, T = geometry(fs_in, fs_out)
    tab = table(fs_in, fs_out) if tab is None else np.asarray(tab, np.int64).reshape(L, T)
    m = mono(x)
    n = np.arange(n_out(len(m), fs_in, fs_out), dtype=np.int64)
    c = n * M + half
    p, jb = c % L, c // L
    mp = np.concatenate([np.zeros(T, np.int64), m, np.zeros(T + 1, np.int64)])      # mp[j + T] = m[j], zero outside the file
    acc = np.zeros(len(n), np.int64)
    for t in range(T):
        acc += tab[p, t] * mp[jb - t + T]
    return acc


def resample(x, fs_in, fs_out=8000, tab=None):
    x = np.asarray(x)
    return finish(accumulate(x, fs_in, fs_out, tab), 1 if x.ndim == 1 else 2)


def accumulate_by_definition(x, fs_in, fs_out=8000):
    """acc[n] = sum_j hq[n M - j L] m[j] over |n M - j L| <= half, 0 <= j < n_in: the definition, output by output."""
    L, M, half, _ = geometry(fs_in, fs_out)
    hq, m = design(fs_in, fs_out), mono(x)
    acc = np.zeros(n_out(len(m), fs_in, fs_out), np.int64)
    for n in range(len(acc)):
        j = np.arange(max(0, -((half - n * M) // L)), min(len(m) - 1, (n * M + half) // L) + 1)
        acc[n] = np.sum(hq[n * M - j * L + half] * m[j])
    return acc


def input_range(n0, n1, n_in, fs_in, fs_out=8000):
    """Brute force: the frames the outputs [n0, n1) read, as (first, last) half-open; None if there are none."""
    L, M, half, _ = geometry(fs_in, fs_out)
    j = np.arange(n_in, dtype=np.int64)
    used = np.zeros(n_in, bool)
    for n in range(n0, n1):
        used |= np.abs(n * M - j * L) <= half
    idx = np.flatnonzero(used)
    return (int(idx[0]), int(idx[-1]) + 1) if len(idx) else None
