"""numpy restatement of the block codecs' contract (include/nafp.h `nafp_codec_*`): G.711 A-law and
mu-law, IMA ADPCM and MS ADPCM at 4 bits -- decode by the text of the contract, vectorised over blocks and serial over the
nibbles of a block; simple encoders that produce file bodies for the tests; a WAV writer with the fmt extension and an optional
`fact` chunk.  Nothing here calls the library."""
import struct

import numpy as np

import _ingest_ref as iref

CODECS = {'alaw': 1, 'ulaw': 2, 'ima4': 3, 'ms4': 4}
TAGS = {'alaw': 6, 'ulaw': 7, 'ima4': 0x11, 'ms4': 2}
MAX_ALIGN = 4096
STEP = np.array([7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118,
                 130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060,
                 1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484,
                 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767],
                np.int64)
IDX = np.array([-1, -1, -1, -1, 2, 4, 6, 8, -1, -1, -1, -1, 2, 4, 6, 8], np.int64)
ADAPT = np.array([230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230], np.int64)
MS_COEFS = [(256, 0), (512, -256), (0, 0), (192, 64), (240, 0), (460, -208), (392, -232)]
C1 = np.array([c[0] for c in MS_COEFS], np.int64)
C2 = np.array([c[1] for c in MS_COEFS], np.int64)


def samples_per_block(codec, channels, align):
    """spb, or -1 for anything outside the contract's lists."""
    if align < 1 or align > MAX_ALIGN or channels < 1:
        return -1
    if codec in ('alaw', 'ulaw'):
        return 1 if channels <= 8 and align == channels else -1
    if channels > 2:
        return -1
    if codec == 'ima4':
        body = align - 4 * channels
        return 8 * (body // (4 * channels)) + 1 if body >= 4 * channels and body % (4 * channels) == 0 else -1
    if codec == 'ms4':
        return 2 + 2 * (align - 7 * channels) // channels if align > 7 * channels else -1
    return -1


def ulaw(byte):
    u = ~np.asarray(byte, np.int64) & 0xff
    t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4)
    return np.where(u & 0x80, 0x84 - t, t - 0x84)


def alaw(byte):
    a = np.asarray(byte, np.int64) ^ 0x55
    t = (a & 15) << 4
    seg = (a & 0x70) >> 4
    t = np.where(seg == 0, t + 8, np.where(seg == 1, t + 0x108, (t + 0x108) << np.maximum(seg - 1, 0)))
    return np.where(a & 0x80, t, -t)


def ima_step(n, pred, idx):
    """One nibble for arrays of states: -> (pred, idx)."""
    s = STEP[idx]
    d = (s >> 3) + np.where(n & 1, s >> 2, 0) + np.where(n & 2, s >> 1, 0) + np.where(n & 4, s, 0)
    pred = np.clip(np.where(n & 8, pred - d, pred + d), -32768, 32767)
    return pred, np.clip(idx + IDX[n], 0, 88)


def ms_step(n, c1, c2, delta, s1, s2):
    """One nibble for arrays of states: -> (x, delta); the caller shifts s2 = s1, s1 = x."""
    s = np.where(n >= 8, n - 16, n)
    a = s1 * c1 + s2 * c2
    pred = np.sign(a) * (np.abs(a) // 256)                    # C division: toward zero
    x = np.clip(pred + s * delta, -32768, 32767)
    return x, np.clip((ADAPT[n] * delta) >> 8, 16, 2796202)


def _i16(lo, hi):
    v = lo.astype(np.int64) | (hi.astype(np.int64) << 8)
    return np.where(v >= 32768, v - 65536, v)


def decode(codec, channels, align, data):
    """int16 [n_blocks * spb * channels] of the whole blocks in `data` (a trailing partial block is ignored)."""
    C, spb = channels, samples_per_block(codec, channels, align)
    assert spb > 0
    b = np.frombuffer(bytes(data), np.uint8)
    B = len(b) // align
    b = b[:B * align].reshape(B, align).astype(np.int64)
    if codec in ('alaw', 'ulaw'):
        return (alaw if codec == 'alaw' else ulaw)(b).reshape(-1).astype(np.int16)
    out = np.zeros((B, spb, C), np.int64)
    for c in range(C):
        if codec == 'ima4':
            pred, idx = _i16(b[:, 4 * c], b[:, 4 * c + 1]), np.minimum(b[:, 4 * c + 2], 88)
            out[:, 0, c] = pred
            G = (align - 4 * C) // (4 * C)
            body = b[:, 4 * C:].reshape(B, G, C, 4)[:, :, c, :]                          # [B][group][byte]
            nib = np.stack([body & 15, body >> 4], axis=-1).reshape(B, 8 * G)           # low nibble first
            for k in range(8 * G):
                pred, idx = ima_step(nib[:, k], pred, idx)
                out[:, 1 + k, c] = pred
        else:
            p = np.minimum(b[:, c], 6)
            c1, c2 = C1[p], C2[p]
            delta = _i16(b[:, C + 2 * c], b[:, C + 2 * c + 1])
            s1 = _i16(b[:, 3 * C + 2 * c], b[:, 3 * C + 2 * c + 1])
            s2 = _i16(b[:, 5 * C + 2 * c], b[:, 5 * C + 2 * c + 1])
            out[:, 0, c], out[:, 1, c] = s2, s1
            body = b[:, 7 * C:]
            nib = np.stack([body >> 4, body & 15], axis=-1).reshape(B, -1)[:, c::C]     # high nibble first, round-robin
            for k in range(nib.shape[1]):
                x, delta = ms_step(nib[:, k], c1, c2, delta, s1, s2)
                s2, s1 = s1, x
                out[:, 2 + k, c] = x
    return out.reshape(-1).astype(np.int16)


def decode_file(codec, channels, align, data, n_frames=None):
    """(n_frames, channels) int16 of a file body: `decode`, cut to the file's frame count."""
    x = decode(codec, channels, align, data).reshape(-1, channels)
    return x if n_frames is None else x[:n_frames]


# ---- simple encoders: file bodies whose decoded signal follows x ----------------------------------------------------------
def _le16(v):
    v = np.asarray(v, np.int64) & 0xffff
    return (v & 0xff).astype(np.uint8), (v >> 8).astype(np.uint8)


def encode(codec, x, channels, align):
    """Bytes of whole blocks that decode to something near x ((n, channels) or flat interleaved int16-range integers); the
    last block is padded by repeating the last frame."""
    C, spb = channels, samples_per_block(codec, channels, align)
    assert spb > 0
    x = np.asarray(x, np.int64).reshape(-1, C)
    if codec in ('alaw', 'ulaw'):
        table = (alaw if codec == 'alaw' else ulaw)(np.arange(256))
        order = np.argsort(table, kind='stable')
        pos = np.clip(np.searchsorted(table[order], x.reshape(-1)), 1, 255)
        lo, hi = order[pos - 1], order[pos]
        pick = np.where(np.abs(table[lo] - x.reshape(-1)) <= np.abs(table[hi] - x.reshape(-1)), lo, hi)
        return pick.astype(np.uint8).tobytes()
    B = -(-len(x) // spb)
    if B * spb > len(x):
        x = np.concatenate([x, np.repeat(x[-1:], B * spb - len(x), axis=0)])
    x = x.reshape(B, spb, C)
    blk = np.zeros((B, align), np.uint8)
    for c in range(C):
        if codec == 'ima4':
            pred = x[:, 0, c].copy()
            idx = np.clip(np.searchsorted(STEP, np.abs(x[:, 1, c] - x[:, 0, c])), 0, 88)
            blk[:, 4 * c], blk[:, 4 * c + 1] = _le16(pred)
            blk[:, 4 * c + 2] = idx
            G = (align - 4 * C) // (4 * C)
            nib = np.zeros((B, 8 * G), np.int64)
            for k in range(8 * G):
                diff = x[:, 1 + k, c] - pred
                n = np.minimum(7, np.abs(diff) * 4 // STEP[idx]) | np.where(diff < 0, 8, 0)
                nib[:, k] = n
                pred, idx = ima_step(n, pred, idx)
            byte = (nib[:, 0::2] | (nib[:, 1::2] << 4)).reshape(B, G, 4)
            for g in range(G):
                blk[:, 4 * C * (g + 1) + 4 * c:4 * C * (g + 1) + 4 * c + 4] = byte[:, g]
        else:
            p = (np.arange(B) + c) % 7                            # every coefficient pair gets used
            c1, c2 = C1[p], C2[p]
            s2, s1 = x[:, 0, c].copy(), x[:, 1, c].copy()
            delta = np.clip(np.abs(s1 - s2) // 4, 16, 32767)
            blk[:, c] = p
            blk[:, C + 2 * c], blk[:, C + 2 * c + 1] = _le16(delta)
            blk[:, 3 * C + 2 * c], blk[:, 3 * C + 2 * c + 1] = _le16(s1)
            blk[:, 5 * C + 2 * c], blk[:, 5 * C + 2 * c + 1] = _le16(s2)
            K = spb - 2
            nib = np.zeros((B, K), np.int64)
            for k in range(K):
                a = s1 * c1 + s2 * c2
                pred = np.sign(a) * (np.abs(a) // 256)
                s = np.clip(np.floor((x[:, 2 + k, c] - pred) / delta + 0.5).astype(np.int64), -8, 7)
                n = s & 15
                nib[:, k] = n
                v, delta = ms_step(n, c1, c2, delta, s1, s2)
                s2, s1 = s1, v
            if C == 1:
                blk[:, 7:] = (nib[:, 0::2] << 4) | nib[:, 1::2]
            elif c == 0:
                blk[:, 14:] |= (nib << 4).astype(np.uint8)
            else:
                blk[:, 14:] |= nib.astype(np.uint8)
    return blk.tobytes()


def fmt_chunk(codec, fs, channels, align, extensible=False, tag=None, bits=None, spb=None, n_coef=None, coefs=None, cb=None,
              guid=None, short=None):
    """The fmt chunk body of a codec file; the keyword arguments override single header fields (`short`: cut to that many bytes)."""
    bits = (8 if codec in ('alaw', 'ulaw') else 4) if bits is None else bits
    if extensible:
        guid = (bytes([TAGS[codec], 0]) + iref.GUID_PCM[2:]) if guid is None else guid
        body = struct.pack('<HHIIHHHHI', 0xFFFE if tag is None else tag, channels, fs, fs * align, align, bits, 22, bits,
                           (1 << channels) - 1) + guid
    else:
        body = struct.pack('<HHIIHH', TAGS[codec] if tag is None else tag, channels, fs, fs * align, align, bits)
        if codec in ('alaw', 'ulaw'):
            body += struct.pack('<H', 0)
        else:
            spb = samples_per_block(codec, channels, align) if spb is None else spb
            if codec == 'ima4':
                body += struct.pack('<HH', 2 if cb is None else cb, spb & 0xffff)
            else:
                coefs = MS_COEFS if coefs is None else coefs
                body += struct.pack('<HHH', 32 if cb is None else cb, spb & 0xffff, 7 if n_coef is None else n_coef)
                body += b''.join(struct.pack('<hh', a, b) for a, b in coefs)
    return body if short is None else body[:short]


def wav_bytes(codec, body, fs, channels, align, fact=None, data_size=None, **fmt_kw):
    """A RIFF/WAVE file around the blocks in `body`; `fact`: the frame count written into a fact chunk (None: no such chunk)."""
    fmt = fmt_chunk(codec, fs, channels, align, **fmt_kw)
    chunks = b'fmt ' + struct.pack('<I', len(fmt)) + fmt + (b'\0' if len(fmt) & 1 else b'')
    if fact is not None:
        chunks += b'fact' + struct.pack('<II', 4, fact)
    chunks += b'data' + struct.pack('<I', len(body) if data_size is None else data_size) + body
    return b'RIFF' + struct.pack('<I', 4 + len(chunks)) + b'WAVE' + chunks


def music(n, fs, channels, seed, amp=0.25):
    """(n, channels) int64 in the int16 range: a few partials below 0.4 * min(fs, 8000) plus a little noise per channel."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = np.stack([sum(amp * np.sin(2 * np.pi * f * t + p) for f, p in zip(rng.uniform(200, 0.4 * min(fs, 8000), 4), rng.uniform(0, 6, 4)))
                  + rng.uniform(-0.05, 0.05, size=n) for _ in range(channels)], axis=1)
    return np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int64)


def pcm16_wav(x, fs, channels):
    """The 16-bit PCM WAV of decoded frames ((n, channels) int16): what a converter would have written."""
    return iref.wav_bytes('s16', np.asarray(x).astype('<i2').tobytes(), fs, channels)
