"""numpy restatement of the varispeed contract (include/nafp.h): the float64 filter design, the int32
table and the int64 interpolation and convolution.  This file is the definition; nothing here calls the library."""
import math

import numpy as np

BETA, ZEROS, CUT = 8.6, 32, 0.95
ONE = 1 << 24
STEP_MIN, STEP_MAX = 13421773, 20971520
PHASES = 512


def step_for(speed):
    """The step that undoes a recording played `speed` times too fast."""
    return int(round(ONE / float(speed)))


def geometry(step):
    """(W, T)."""
    if not STEP_MIN <= step <= STEP_MAX:
        raise ValueError(step)
    W = -(-(20 * ZEROS * max(step, ONE)) // (19 * ONE))      # ceil(32 / (2 fc)), 2 fc = 0.95 min(1, 2^24 / step), in integers
    return W, 2 * W


def two_fc(step):
    return CUT * float(ONE) / float(step) if step > ONE else CUT


def _i0(x):
    """sum_k ((x/2)^k / k!)^2 term by term, as the library sums it (a term below 1e-18 of the sum no longer changes it)."""
    x = np.asarray(x, np.float64)
    q = 0.25 * x * x
    term, total = np.ones_like(q), np.ones_like(q)
    for k in range(1, 200):
        term = term * (q / (float(k) * float(k)))
        total = total + term
        if np.all(term < 1e-18 * total):
            break
    return total


_sin = np.vectorize(math.sin, otypes=[np.float64])          # the C library's sin, as the host design calls it


def h(u, step):
    """The float64 filter at offsets u (any shape)."""
    W, _ = geometry(step)
    u = np.asarray(u, np.float64)
    f = two_fc(step)
    x = math.pi * (f * u)
    with np.errstate(invalid='ignore', divide='ignore'):
        sinc = np.where(u == 0.0, 1.0, _sin(x) / x)
    r = u / float(W)
    w = _i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - r * r))) * (1.0 / _i0(BETA))
    return np.where(np.abs(u) <= W, sinc * w * f, 0.0)


def table(step):
    """hq[p][t] = round(2^30 h(p / 512 + W - 1 - t)), (513, T) int64."""
    W, T = geometry(step)
    u = np.arange(PHASES + 1, dtype=np.float64)[:, None] / 512.0 + (W - 1 - np.arange(T, dtype=np.float64))[None, :]
    v = h(u, step) * 1073741824.0
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)).astype(np.int64)      # llround: halves away from zero


def n_out(n_in, step):
    return -(-(n_in * ONE) // step)


def phases(n, step):
    """(pos, p, w) of the outputs n."""
    P = np.asarray(n, np.int64) * np.int64(step)
    frac = P & (ONE - 1)
    return P >> 24, frac >> 15, frac & 32767


def coefficients(n, step, tab=None):
    """c[n][t], int64."""
    tab = table(step) if tab is None else np.asarray(tab, np.int64)
    _, p, w = phases(n, step)
    return (tab[p] * (32768 - w)[:, None] + tab[p + 1] * w[:, None] + 16384) >> 15


def accumulate(x, step, tab=None, n=None, frame0=0):
    """acc[n] for every output of the file x (int16), or for the outputs `n`.  frame0: x holds the samples from frame0 on of a
    longer file (all that the outputs `n` read of it, the rest counting as zero)."""
    W, T = geometry(step)
    x = np.asarray(x, np.int64)
    n = np.arange(n_out(len(x), step), dtype=np.int64) if n is None else np.asarray(n, np.int64)
    pos, _, _ = phases(n, step)
    c = coefficients(n, step, tab)
    xp = np.concatenate([x, np.zeros(1, np.int64)])                                     # xp[len(x)]: zero, for every index outside
    acc = np.zeros(len(n), np.int64)
    for t in range(T):
        j = pos - W + 1 + t - frame0
        acc += c[:, t] * xp[np.where((j >= 0) & (j < len(x)), j, len(x))]
    return acc


def finish(acc):
    return np.clip((acc + (1 << 29)) >> 30, -32768, 32767).astype(np.int16)


def unclamped(acc):
    return (acc + (1 << 29)) >> 30


def varispeed(x, step, tab=None):
    return finish(accumulate(x, step, tab))


def evaluate_float(x, step, n=None):
    """sum_j h(P / 2^24 - j) x[j] in float64 over the same window, without table, interpolation or rounding."""
    W, T = geometry(step)
    x = np.asarray(x, np.float64)
    n = np.arange(n_out(len(x), step), dtype=np.int64) if n is None else np.asarray(n, np.int64)
    P = n * np.int64(step)
    pos, frac = P >> 24, (P & (ONE - 1)).astype(np.float64) / float(ONE)
    xp = np.concatenate([np.zeros(W), x, np.zeros(W + 1)])
    t = np.arange(T)
    u = frac[:, None] + (W - 1 - t)[None, :]
    return np.sum(h(u, step) * xp[pos[:, None] + 1 + t[None, :]], axis=1)


def input_range(n0, n1, n_in, step):
    """Brute force: the samples the outputs [n0, n1) read, as (first, last) half-open; None if there are none."""
    W, T = geometry(step)
    used = np.zeros(n_in, bool)
    for n in range(n0, n1):
        pos = (n * step) >> 24
        used[max(0, pos - W + 1):max(0, min(n_in, pos + W + 1))] = True
    idx = np.flatnonzero(used)
    return (int(idx[0]), int(idx[-1]) + 1) if len(idx) else None
