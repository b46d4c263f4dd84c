"""numpy restatement of the general ingest's contract (include/nafp.h `nafp_ingest_*`): decode to the
canonical sample, down-mix, the float64 filter design for either direction, the int64 convolution and the floor-division
finish.  Nothing here calls the library."""
import math

import numpy as np

FORMATS = {'u8': (1, 1), 's16': (2, 2), 's24': (3, 3), 's32': (4, 4), 'f32': (5, 4), 'f64': (6, 8)}     # name -> (code, bytes)
MAX_L, MAX_RATE, LDS_BYTES, BLOCK = 640, 192000, 64 * 1024, 256
Q_MAX, Q_MIN = 2 ** 23 - 1, -2 ** 23


def geometry(fs_in, fs_out):
    """(L, M, half, T), or None for a pair the contract refuses."""
    if fs_in > MAX_RATE or fs_out > MAX_RATE:
        return None
    if fs_in == fs_out:
        return 1, 1, 0, 1
    g = math.gcd(fs_in, fs_out)
    L, M = fs_out // g, fs_in // g
    if L > MAX_L:
        return None
    lo, fv = min(fs_in, fs_out), fs_in * L
    half = -(-(640 * fv) // (19 * lo))
    T = -(-(2 * half + 1) // L)
    if (-(-((BLOCK - 1) * M) // L) + T + 1) * 4 > LDS_BYTES:
        return None
    return L, M, half, T


def design(fs_in, fs_out):
    """hq[v + half], v in [-half, half], int64."""
    L, M, half, T = geometry(fs_in, fs_out)
    if half == 0:
        return np.array([1 << 30], np.int64)
    v = np.arange(-half, half + 1, dtype=np.float64)
    r = 0.95 * min(fs_in, fs_out) / (float(fs_in) * L)        # 2 fc / fv
    h = np.sinc(r * v) * np.i0(8.6 * np.sqrt(np.maximum(0.0, 1.0 - (v / half) ** 2))) / np.i0(8.6) * r * L
    return np.rint(h * 2.0 ** 30).astype(np.int64)


def table(fs_in, fs_out):
    """[phase p][tap t] = hq[p + t L - half], zero where out of range."""
    L, M, half, T = geometry(fs_in, fs_out)
    flat = np.zeros(L * T, np.int64)
    hq = design(fs_in, fs_out)
    flat[:len(hq)] = hq
    return np.ascontiguousarray(flat.reshape(T, L).T)


def n_out(n_in, fs_in, fs_out):
    L, M, _, _ = geometry(fs_in, fs_out)
    return -(-(n_in * L) // M)


def decode(fmt, data):
    """q (int64) of every sample in `data` (bytes of consecutive little-endian samples of format `fmt`)."""
    b = np.frombuffer(bytes(data), np.uint8)
    if fmt == 'u8':
        return (b.astype(np.int64) - 128) << 16
    if fmt == 's16':
        return np.frombuffer(b.tobytes(), '<i2').astype(np.int64) << 8
    if fmt == 's24':
        t = b.reshape(-1, 3).astype(np.int64)
        x = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
        return np.where(x >= 1 << 23, x - (1 << 24), x)
    if fmt == 's32':
        return np.minimum((np.frombuffer(b.tobytes(), '<i4').astype(np.int64) + 128) >> 8, Q_MAX)
    x = np.frombuffer(b.tobytes(), '<f4' if fmt == 'f32' else '<f8')
    with np.errstate(over='ignore', invalid='ignore'):
        y = np.rint(x * x.dtype.type(2.0 ** 23))             # exact (a power of two); to nearest, ties to even
        y = np.where(np.isnan(x), 0.0, np.clip(y.astype(np.float64), float(Q_MIN), float(Q_MAX)))
    return y.astype(np.int64)


def encode(fmt, q):
    """Bytes of format `fmt` that decode to ... something near q (int64 at 2^-23 of full scale): a file body for the tests."""
    q = np.asarray(q, np.int64)
    if fmt == 'u8':
        return (np.clip(q >> 16, -128, 127) + 128).astype(np.uint8).tobytes()
    if fmt == 's16':
        return np.clip(q >> 8, -32768, 32767).astype('<i2').tobytes()
    if fmt == 's24':
        x = np.clip(q, Q_MIN, Q_MAX).astype('<i4')
        return x.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    if fmt == 's32':
        return np.clip(q * 256 + (q & 0x7f), -2 ** 31, 2 ** 31 - 1).astype('<i4').tobytes()
    return (q / 2.0 ** 23).astype('<f4' if fmt == 'f32' else '<f8').tobytes()


def mix(fmt, data, channels):
    """m[j] = sum_c q[j][c] of an interleaved file body."""
    return decode(fmt, data).reshape(-1, channels).sum(axis=1)


def accumulate(m, fs_in, fs_out, tab=None):
    """acc[n] (Python-int exact in int64: |acc| < 2^58) for every output of the down-mixed file m, from the canonical table."""
    L, M, half, T = geometry(fs_in, fs_out)
    tab = table(fs_in, fs_out) if tab is None else np.asarray(tab, np.int64).reshape(L, T)
    m = np.asarray(m, np.int64)
    n = np.arange(n_out(len(m), fs_in, fs_out), dtype=np.int64)
    c = n * M + half
    p, jb = c % L, c // L
    mp = np.concatenate([np.zeros(T, np.int64), m, np.zeros(T + 1 + BLOCK, np.int64)])        # mp[j + T] = m[j], zero outside
    acc = np.zeros(len(n), np.int64)
    for t in range(T):
        acc += tab[p, t] * mp[jb - t + T]
    return acc


def accumulate_by_definition(m, fs_in, fs_out):
    """acc[n] = sum_j hq[n M - j L] m[j] over |n M - j L| <= half, 0 <= j < n_in, output by output."""
    L, M, half, _ = geometry(fs_in, fs_out)
    hq, m = design(fs_in, fs_out), np.asarray(m, np.int64)
    acc = np.zeros(n_out(len(m), fs_in, fs_out), np.int64)
    for n in range(len(acc)):
        j = np.arange(max(0, -((half - n * M) // L)), min(len(m) - 1, (n * M + half) // L) + 1)
        acc[n] = np.sum(hq[n * M - j * L + half] * m[j])
    return acc


def finish(acc, channels):
    D = channels << 38
    return np.clip((np.asarray(acc, np.int64) + D // 2) // D, -32768, 32767).astype(np.int16)       # numpy // floors


def ingest(fmt, data, channels, fs_in, fs_out, tab=None):
    """int16 at fs_out of a file body: the whole contract."""
    return finish(accumulate(mix(fmt, data, channels), fs_in, fs_out, tab), channels)


def input_range(n0, n1, n_in, fs_in, fs_out):
    """Brute force: the frames the outputs [n0, n1) read, as (first, last) half-open; None if there are none."""
    L, M, half, _ = geometry(fs_in, fs_out)
    j = np.arange(n_in, dtype=np.int64)
    used = np.zeros(n_in, bool)
    for n in range(n0, n1):
        used |= np.abs(n * M - j * L) <= half
    idx = np.flatnonzero(used)
    return (int(idx[0]), int(idx[-1]) + 1) if len(idx) else None


GUID_PCM = bytes.fromhex('0100000000001000800000aa00389b71')
GUID_FLOAT = bytes.fromhex('0300000000001000800000aa00389b71')


def wav_bytes(fmt, body, fs, channels, extensible=False, tag=None, bits=None, align=None, guid=None, extra_chunk=None,
              data_size=None):
    """A RIFF/WAVE file around `body`, written with struct (not `wave`); the keyword arguments override single header fields."""
    import struct
    width = FORMATS[fmt][1]
    kind = 3 if fmt in ('f32', 'f64') else 1
    align = channels * width if align is None else align
    bits = 8 * width if bits is None else bits
    if extensible:
        guid = (GUID_FLOAT if kind == 3 else GUID_PCM) if guid is None else guid
        fmt_body = struct.pack('<HHIIHHHHI', 0xFFFE if tag is None else tag, channels, fs, fs * align, align, bits, 22, bits,
                               (1 << channels) - 1) + guid
    else:
        fmt_body = struct.pack('<HHIIHH', kind if tag is None else tag, channels, fs, fs * align, align, bits)
    chunks = b'fmt ' + struct.pack('<I', len(fmt_body)) + fmt_body
    if extra_chunk is not None:                                   # e.g. an odd-sized LIST chunk: padded to even
        chunks += b'LIST' + struct.pack('<I', len(extra_chunk)) + extra_chunk + (b'\0' if len(extra_chunk) & 1 else b'')
    chunks += b'data' + struct.pack('<I', len(body) if data_size is None else data_size) + body
    return b'RIFF' + struct.pack('<I', 4 + len(chunks)) + b'WAVE' + chunks
