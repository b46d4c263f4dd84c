"""numpy restatement of what NAFP_INGEST_AIFF=1 adds (include/nafp.h): the signed 8-bit and big-endian
sample formats of `nafp_ingest_*`, Apple's IMA4 packets of `nafp_codec_*` (a decoder by the text of the contract and a simple
encoder), the 80-bit sample rate of an AIFF COMM chunk in both directions, byte-level writers of AIFF, AIFF-C and AU files whose
every header field can be set, a parser of those files that shares nothing with the library's, and `to_wav`: the PCM WAV twin of
any such file.  Nothing here calls the library."""
import struct
from fractions import Fraction

import numpy as np

import _codec_ref as cref
import _ingest_ref as iref

S8, BE = 8, 16
# name -> (NAFP_INGEST_* code, bytes per sample, the little-endian format whose rule applies to the reversed bytes)
FORMATS = {'s8': (S8, 1, None), 's16be': (2 | BE, 2, 's16'), 's24be': (3 | BE, 3, 's24'), 's32be': (4 | BE, 4, 's32'),
           'f32be': (5 | BE, 4, 'f32'), 'f64be': (6 | BE, 8, 'f64')}
WIDTHS = dict({k: v[1] for k, v in iref.FORMATS.items()}, **{k: v[1] for k, v in FORMATS.items()})
QT_CODE, QT_PACKET, QT_SPB = 6, 34, 64


def reverse(data, width):
    """Every sample's bytes in the opposite order."""
    return np.frombuffer(bytes(data), np.uint8).reshape(-1, width)[:, ::-1].tobytes()


def decode(fmt, data):
    """q (int64) of every sample in `data`, for the new formats and the little-endian ones alike."""
    if fmt == 's8':
        return np.frombuffer(bytes(data), np.int8).astype(np.int64) << 16
    if fmt in FORMATS:
        return iref.decode(FORMATS[fmt][2], reverse(data, FORMATS[fmt][1]))
    return iref.decode(fmt, data)


def encode(fmt, q):
    """A file body of format `fmt` near q (int64 at 2^-23 of full scale)."""
    if fmt == 's8':
        return np.clip(np.asarray(q, np.int64) >> 16, -128, 127).astype(np.int8).tobytes()
    if fmt in FORMATS:
        return reverse(iref.encode(FORMATS[fmt][2], q), FORMATS[fmt][1])
    return iref.encode(fmt, q)


# ---- the 80-bit extended sample rate ----------------------------------------------------------------------------------------
def ext80(value):
    """The 10 bytes of `value`: an int, a Fraction whose mantissa fits 64 bits, or a float infinity / NaN."""
    if isinstance(value, float) and value != value:
        return struct.pack('>HQ', 0x7fff, 0xc000000000000000)
    if isinstance(value, float) and value in (float('inf'), float('-inf')):
        return struct.pack('>HQ', 0x7fff | (0x8000 if value < 0 else 0), 0x8000000000000000)
    v = Fraction(value)
    sign, v = (0x8000, -v) if v < 0 else (0, v)
    if v == 0:
        return struct.pack('>HQ', sign, 0)
    k = 0
    while Fraction(2) ** (k + 1) <= v:
        k += 1
    while Fraction(2) ** k > v:
        k -= 1
    mant = v * Fraction(2) ** (63 - k)
    assert mant.denominator == 1 and mant.numerator >> 63 == 1
    return struct.pack('>HQ', sign | (16383 + k), mant.numerator)


def ext80_value(ten):
    """The Fraction an 80-bit field holds, or a float for an infinity / NaN."""
    se, mant = struct.unpack('>HQ', ten)
    if se & 0x7fff == 0x7fff:
        return float('nan') if mant << 1 & 0xffffffffffffffff else float('-inf' if se >> 15 else 'inf')
    v = Fraction(mant) * Fraction(2) ** ((se & 0x7fff) - 16383 - 63)
    return -v if se >> 15 else v


# ---- Apple IMA4 ----------------------------------------------------------------------------------------------------------
def qt_decode(channels, data):
    """int16 [n_blocks * 64 * channels] of the whole blocks in `data`: per channel a 34-byte packet -- a big-endian u16 whose
    upper 9 bits are the predictor and lower 7 the step index (clamped to 88), then 32 bytes of nibbles, low first; the predictor
    after each nibble is a frame.  Nothing is carried from one packet to the next."""
    C, align = channels, QT_PACKET * channels
    b = np.frombuffer(bytes(data), np.uint8)
    B = len(b) // align
    b = b[:B * align].reshape(B, C, QT_PACKET).astype(np.int64)
    out = np.zeros((B, QT_SPB, C), np.int64)
    for c in range(C):
        h = (b[:, c, 0] << 8) | b[:, c, 1]
        pred = h & 0xff80
        pred = np.where(pred >= 32768, pred - 65536, pred)
        idx = np.minimum(h & 0x7f, 88)
        body = b[:, c, 2:]
        nib = np.stack([body & 15, body >> 4], axis=-1).reshape(B, QT_SPB)
        for k in range(QT_SPB):
            pred, idx = cref.ima_step(nib[:, k], pred, idx)
            out[:, k, c] = pred
    return out.reshape(-1).astype(np.int16)


def qt_encode(x, channels):
    """Whole blocks that decode to something near x ((n, channels) int16-range integers): each packet starts from the frame
    before it, with its low 7 bits dropped; the last block is padded by repeating the last frame."""
    C = channels
    x = np.asarray(x, np.int64).reshape(-1, C)
    B = -(-len(x) // QT_SPB)
    if B * QT_SPB > len(x):
        x = np.concatenate([x, np.repeat(x[-1:], B * QT_SPB - len(x), axis=0)])
    x = x.reshape(B, QT_SPB, C)
    blk = np.zeros((B, C, QT_PACKET), np.uint8)
    for c in range(C):
        start = np.concatenate([x[:1, 0, c], x[:-1, -1, c]])
        pred = np.where((start & 0xff80) >= 32768, (start & 0xff80) - 65536, start & 0xff80)
        idx = np.clip(np.searchsorted(cref.STEP, np.abs(x[:, 1, c] - x[:, 0, c])), 0, 88)
        h = (pred & 0xff80) | idx
        blk[:, c, 0], blk[:, c, 1] = h >> 8, h & 0xff
        nib = np.zeros((B, QT_SPB), np.int64)
        for k in range(QT_SPB):
            diff = x[:, k, c] - pred
            n = np.minimum(7, np.abs(diff) * 4 // cref.STEP[idx]) | np.where(diff < 0, 8, 0)
            nib[:, k] = n
            pred, idx = cref.ima_step(n, pred, idx)
        blk[:, c, 2:] = nib[:, 0::2] | (nib[:, 1::2] << 4)
    return blk.tobytes()


# ---- writers -------------------------------------------------------------------------------------------------------------
def _chunk(cid, body, size=None):
    return cid + struct.pack('>I', len(body) if size is None else size) + body + (b'\0' if len(body) & 1 else b'')


def _unit_bytes(ctype, channels, bits):
    """Bytes of one unit numSampleFrames counts: a frame, or for ima4 a block."""
    if ctype == b'ima4':
        return QT_PACKET * channels
    if ctype in (b'alaw', b'ALAW', b'ulaw', b'ULAW'):
        return channels
    if ctype in (b'fl32', b'FL32', b'fl64', b'FL64'):
        return channels * (4 if ctype.lower() == b'fl32' else 8)
    return channels * ((bits + 7) // 8)


def aiff_bytes(body, rate, channels, bits, ctype=None, n_frames=None, ssnd_offset=0, ssnd_first=False, junk=(), truncate=None,
               comm=True, ssnd=True, ssnd_size=None, cname=b'', block_size=0):
    """An AIFF file (ctype None) or an AIFF-C file of compression type `ctype` around `body`, written with struct.  rate: what
    ext80 takes, or 10 bytes as they are.  n_frames: numSampleFrames (default: what the body holds).  ssnd_offset: that many
    filler bytes before the first sample, stated in the SSND chunk's offset field.  ssnd_first: SSND before COMM.  junk:
    (id, body) chunks put between the two (odd-sized ones are padded).  truncate: cut that many bytes off the end of the file
    (the sizes in the headers stay).  comm / ssnd False: leave the chunk out."""
    unit = max(_unit_bytes(ctype or b'NONE', channels, bits), 1)
    n_frames = len(body) // unit if n_frames is None else n_frames
    c = struct.pack('>hIh', channels, n_frames, bits) + (rate if isinstance(rate, bytes) else ext80(rate))
    if ctype is not None:
        c += ctype + bytes([len(cname)]) + cname + (b'' if len(cname) & 1 else b'\0')
    s_body = struct.pack('>II', ssnd_offset, block_size) + b'\xa5' * ssnd_offset + body
    parts = ([_chunk(b'COMM', c)] if comm else []) + [_chunk(i, b) for i, b in junk] + ([_chunk(b'SSND', s_body, ssnd_size)] if ssnd else [])
    if ssnd_first:
        parts = parts[::-1]
    if ctype is not None:
        parts.insert(0, _chunk(b'FVER', struct.pack('>I', 0xa2805140)))
    chunks = b''.join(parts)
    data = b'FORM' + struct.pack('>I', 4 + len(chunks)) + (b'AIFF' if ctype is None else b'AIFC') + chunks
    return data[:len(data) - truncate] if truncate else data


def aifc_bytes(ctype, body, rate, channels, bits, **kw):
    return aiff_bytes(body, rate, channels, bits, ctype=ctype, **kw)


AU_ENCODINGS = {'ulaw': 1, 's8': 2, 's16be': 3, 's24be': 4, 's32be': 5, 'f32be': 6, 'f64be': 7, 'alaw': 27}


def au_bytes(encoding, body, rate, channels, header=24, size=None, magic=b'.snd', truncate=None):
    """An AU file around `body`.  encoding: a name of AU_ENCODINGS or any number.  header: the data offset (the bytes from 24 on are
    an annotation).  size: the stated data size (default: the body's; 0xffffffff: unknown)."""
    enc = AU_ENCODINGS.get(encoding, encoding)
    data = magic + struct.pack('>5I', header, len(body) if size is None else size, enc, rate, channels) + b'\0' * max(header - 24, 0) + body
    return data[:len(data) - truncate] if truncate else data


# ---- a parser of its own, and the WAV twin ---------------------------------------------------------------------------------
_BE = {1: 's8', 2: 's16be', 3: 's24be', 4: 's32be'}
_LE = {1: 's8', 2: 's16', 3: 's24', 4: 's32'}


def parse(data):
    """{'rate', 'channels', 'format', 'width', 'block_align', 'offset', 'n_frames', 'codec', 'samples_per_block'} of the bytes of
    an AIFF, AIFF-C or AU file this module wrote, by the text of the issue; a rate that is no whole number stays a Fraction."""
    if data[:4] == b'.snd':
        off, stated, enc, rate, ch = struct.unpack('>5I', data[4:24])
        fmt = {v: k for k, v in AU_ENCODINGS.items()}[enc]
        present = len(data) - off
        n_bytes, n_units = (present if stated == 0xffffffff else min(stated, present)), None
    else:
        assert data[:4] == b'FORM' and data[8:12] in (b'AIFF', b'AIFC')
        at, comm, ssnd = 12, None, None
        while at + 8 <= len(data):
            cid, size = data[at:at + 4], struct.unpack('>I', data[at + 4:at + 8])[0]
            if cid == b'COMM':
                comm = data[at + 8:at + 8 + size]
            elif cid == b'SSND':
                ssnd = (at + 8, size)
            at += 8 + size + (size & 1)
        ch, n_units, bits = struct.unpack('>hIh', comm[:8])
        rate = ext80_value(comm[8:18])
        rate = int(rate) if isinstance(rate, Fraction) and rate.denominator == 1 else rate
        ctype = comm[18:22] if data[8:12] == b'AIFC' else b'NONE'
        skip, = struct.unpack('>I', data[ssnd[0]:ssnd[0] + 4])
        off = ssnd[0] + 8 + skip
        n_bytes = min(ssnd[1] - 8 - skip, len(data) - off)
        width = (bits + 7) // 8
        fmt = {b'sowt': _LE.get(width), b'raw ': 'u8', b'fl32': 'f32be', b'FL32': 'f32be', b'fl64': 'f64be', b'FL64': 'f64be',
               b'alaw': 'alaw', b'ALAW': 'alaw', b'ulaw': 'ulaw', b'ULAW': 'ulaw', b'ima4': 'qtima4'}.get(ctype, _BE.get(width))
    codec = fmt if fmt in ('alaw', 'ulaw', 'qtima4') else None
    spb = QT_SPB if fmt == 'qtima4' else 1
    width = 0 if codec else WIDTHS[fmt]
    align = QT_PACKET * ch if fmt == 'qtima4' else ch * max(width, 1)
    blocks = max(n_bytes, 0) // align
    return {'rate': rate, 'channels': ch, 'format': fmt, 'width': width, 'block_align': align, 'offset': off,
            'n_frames': (blocks if n_units is None else min(n_units, blocks)) * spb, 'codec': codec, 'samples_per_block': spb}


def to_wav(data):
    """The PCM WAV twin of an AIFF / AIFF-C / AU file: big-endian PCM and float as the little-endian WAV of the same values, signed
    8-bit as a 16-bit file with x << 8, little-endian and unsigned 8-bit bodies as they are, G.711 and Apple IMA4 as the decoded
    16-bit PCM.  Both files give the same canonical samples, so their ingests are equal byte for byte."""
    info = parse(data)
    fmt, ch, rate = info['format'], info['channels'], info['rate']
    n_blocks = info['n_frames'] // info['samples_per_block']
    body = data[info['offset']:info['offset'] + n_blocks * info['block_align']]
    if fmt == 'qtima4':
        return cref.pcm16_wav(qt_decode(ch, body).reshape(-1, ch), rate, ch)
    if fmt in ('alaw', 'ulaw'):
        return cref.pcm16_wav(cref.decode(fmt, ch, ch, body).reshape(-1, ch), rate, ch)
    if fmt == 's8':
        return iref.wav_bytes('s16', (np.frombuffer(body, np.int8).astype('<i2') << 8).tobytes(), rate, ch)
    if fmt in FORMATS:
        return iref.wav_bytes(FORMATS[fmt][2], reverse(body, FORMATS[fmt][1]), rate, ch)
    return iref.wav_bytes(fmt, body, rate, ch)
