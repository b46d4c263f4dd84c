"""CPU: what NAFP_INGEST_AIFF=1 adds.  The header scans of AIFF / AIFF-C / AU files against the restatement's own parser
(tests/_aiff_ref.py) and against files the standard library wrote; the 80-bit sample rate; the library's host decoders -- the
functions the kernels decode with -- for the signed 8-bit and big-endian formats and for Apple's IMA4 packets, against the
restatement and against `audioop`; the refusals by name; the switch."""
import ctypes
import struct
import warnings
from fractions import Fraction

import numpy as np
import pytest

import _aiff_ref as aref
import _codec_ref as cref
import _ingest_ref as iref

SWITCHES = ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS', 'NAFP_INGEST_FLAC', 'NAFP_INGEST_AIFF')
# AIFC compression type -> (bits, format, bytes of one numSampleFrames unit per channel)
AIFC_TYPES = {b'NONE': (16, 's16be'), b'twos': (16, 's16be'), b'in24': (24, 's24be'), b'in32': (32, 's32be'), b'sowt': (16, 's16'),
              b'raw ': (8, 'u8'), b'fl32': (32, 'f32be'), b'FL32': (32, 'f32be'), b'fl64': (64, 'f64be'), b'FL64': (64, 'f64be'),
              b'alaw': (8, 'alaw'), b'ALAW': (16, 'alaw'), b'ulaw': (8, 'ulaw'), b'ULAW': (16, 'ulaw'), b'ima4': (16, 'qtima4')}


def _stdlib(name):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', DeprecationWarning)
        return pytest.importorskip(name)


def _scans():
    from neural_audio_fp_amd.model.utils.audio_utils import aiff_scan, au_scan, aiff_au_scan
    return aiff_scan, au_scan, aiff_au_scan


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def _body(fmt, ch, n, seed=0):
    """n units (frames, or blocks of qtima4) of random bytes."""
    unit = aref.QT_PACKET * ch if fmt == 'qtima4' else ch * (1 if fmt in ('alaw', 'ulaw') else aref.WIDTHS[fmt])
    return np.random.default_rng(seed).integers(0, 256, size=n * unit, dtype=np.uint8).tobytes()


def _ingest_host(nafp, code, data, n):
    buf = np.frombuffer(bytes(data), np.uint8).copy()
    q = np.full(n + 2, 0x5a5a5a5a, np.int32)
    st = nafp._lib.load().nafp_ingest_decode_host(code, buf.ctypes.data_as(ctypes.c_void_p), n, q.ctypes.data_as(ctypes.c_void_p))
    assert np.all(q[n:] == 0x5a5a5a5a)
    return st, q[:n].astype(np.int64)


def _qt_host(nafp, ch, data):
    lib = nafp._lib.load()
    align = aref.QT_PACKET * ch
    assert lib.nafp_codec_samples_per_block(aref.QT_CODE, ch, align) == aref.QT_SPB
    n_blocks = len(data) // align
    buf = np.frombuffer(bytes(data), np.uint8).copy()
    out = np.full(n_blocks * aref.QT_SPB * ch + 4, 0x5555, np.int16)
    st = lib.nafp_codec_decode_host(aref.QT_CODE, ch, align, buf.ctypes.data_as(ctypes.c_void_p), n_blocks, out.ctypes.data_as(ctypes.c_void_p))
    assert st == 0 and np.all(out[-4:] == 0x5555)
    return out[:-4]


# ---- scans -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ch', [1, 2, 8])
def test_aiff_scan_every_format(nafp, tmp_path, ch):
    """AIFF at 1 .. 32 bits and every AIFC type of the list: the dict equals the restatement's parse of the same bytes, and its
    fields are the ones the issue states."""
    aiff_scan, _, dispatch = _scans()
    for bits in (1, 7, 8, 9, 12, 16, 17, 20, 24, 25, 32):
        fmt = {1: 's8', 2: 's16be', 3: 's24be', 4: 's32be'}[(bits + 7) // 8]
        data = aref.aiff_bytes(_body(fmt, ch, 37), 44100, ch, bits)
        got = aiff_scan(_write(tmp_path, f'a{bits}.aif', data))
        assert got == aref.parse(data) and got == dispatch(str(tmp_path / f'a{bits}.aif'))
        assert (got['format'], got['width'], got['block_align'], got['n_frames'], got['codec'], got['samples_per_block'], got['rate'],
                got['channels']) == (fmt, (bits + 7) // 8, ch * ((bits + 7) // 8), 37, None, 1, 44100, ch)
        assert data[got['offset']:got['offset'] + 4] == _body(fmt, ch, 37)[:4]
    for ctype, (bits, fmt) in AIFC_TYPES.items():
        if fmt == 'qtima4' and ch > 2:
            continue
        data = aref.aifc_bytes(ctype, _body(fmt, ch, 21), 22050, ch, bits, cname=b'not compressed')
        got = aiff_scan(_write(tmp_path, 'c.aifc', data))
        assert got == aref.parse(data), ctype
        codec = fmt if fmt in ('alaw', 'ulaw', 'qtima4') else None
        spb = 64 if fmt == 'qtima4' else 1
        align = 34 * ch if fmt == 'qtima4' else ch if codec else ch * aref.WIDTHS[fmt]
        assert (got['format'], got['codec'], got['samples_per_block'], got['block_align'], got['n_frames'], got['width']) == \
               (fmt, codec, spb, align, 21 * spb, 0 if codec else aref.WIDTHS[fmt]), ctype
    for bits, fmt in ((8, 's8'), (24, 's24'), (32, 's32')):         # sowt at the other widths
        data = aref.aifc_bytes(b'sowt', _body(fmt, ch, 5), 8000, ch, bits)
        assert aiff_scan(_write(tmp_path, 's.aifc', data))['format'] == fmt


def test_aiff_scan_chunk_layouts(nafp, tmp_path):
    """SSND before COMM; a junk chunk and an odd-sized chunk in between; a non-zero SSND offset; a truncated SSND (the frames
    present win); numSampleFrames below what is present (the stated count wins); the same for ima4 in packets."""
    aiff_scan = _scans()[0]
    body = _body('s16be', 2, 100)
    junk = ((b'ANNO', b'seven b'), (b'JUNK', bytes(10)))
    for kw, n in (({}, 100), ({'ssnd_first': True}, 100), ({'junk': junk}, 100), ({'junk': junk, 'ssnd_first': True}, 100),
                  ({'ssnd_offset': 6}, 100), ({'ssnd_offset': 5, 'junk': junk, 'block_size': 512}, 100), ({'truncate': 10}, 97),
                  ({'truncate': 11}, 97), ({'truncate': 399}, 0), ({'n_frames': 60}, 60), ({'n_frames': 60, 'truncate': 200}, 50),
                  ({'n_frames': 1000}, 100), ({'ssnd_size': 8 + 200}, 50)):
        data = aref.aiff_bytes(body, 44100, 2, 16, **kw)
        got = aiff_scan(_write(tmp_path, 'x.aiff', data))
        assert got == aref.parse(data), kw
        assert got['n_frames'] == n, kw
        assert data[got['offset']:got['offset'] + 8] == body[:8][:max(0, len(data) - got['offset'])], kw
    body = _body('qtima4', 2, 10)
    for kw, n in (({}, 640), ({'n_frames': 7}, 448), ({'truncate': 1}, 576), ({'truncate': 69}, 512), ({'ssnd_first': True}, 640)):
        data = aref.aifc_bytes(b'ima4', body, 44100, 2, 16, **kw)
        got = aiff_scan(_write(tmp_path, 'x.aifc', data))
        assert got == aref.parse(data) and got['n_frames'] == n, kw


@pytest.mark.parametrize('ch', [1, 2, 8])
def test_au_scan(nafp, tmp_path, ch):
    """Every encoding of the list with a header of 24 and of 40 bytes; size 0xffffffff; a stated size above and below the bytes
    present."""
    _, au_scan, dispatch = _scans()
    for fmt, enc in aref.AU_ENCODINGS.items():
        body = _body(fmt, ch, 33)
        unit = len(body) // 33
        for kw, n in (({}, 33), ({'header': 40}, 33), ({'size': 0xffffffff}, 33), ({'size': 0xffffffff, 'header': 40, 'truncate': unit + 1}, 31),
                      ({'size': 10 * unit}, 10), ({'size': 10 * unit + unit - 1}, 10), ({'size': 50 * unit}, 33),
                      ({'truncate': 1}, 32)):
            data = aref.au_bytes(fmt, body, 8000, ch, **kw)
            name = 'x.snd' if 'header' in kw else 'x.au'
            got = au_scan(_write(tmp_path, name, data))
            assert got == aref.parse(data) and got == dispatch(str(tmp_path / name)), (fmt, kw)
            codec = fmt if fmt in ('alaw', 'ulaw') else None
            assert (got['format'], got['codec'], got['offset'], got['n_frames'], got['block_align'], got['samples_per_block'], got['rate']) == \
                   (fmt, codec, kw.get('header', 24), n, unit, 1, 8000), (fmt, kw)


def test_rates_through_the_80_bit_field(nafp, tmp_path):
    from neural_audio_fp_amd.model.utils.audio_utils import extended_rate
    aiff_scan = _scans()[0]
    for rate in (8000, 11025, 44100, 192000, 1, 48000, 96000):
        ten = aref.ext80(rate)
        assert aref.ext80_value(ten) == rate and extended_rate(ten) == rate
        assert aiff_scan(_write(tmp_path, 'r.aif', aref.aiff_bytes(bytes(8), rate, 1, 16)))['rate'] == rate
    assert aref.ext80(44100) == bytes.fromhex('400eac44000000000000')          # the value every AIFF writer stores
    for value, msg in ((Fraction(88201, 2), r'r\.aif: sample rate 44100\.5 Hz is not a whole number'),
                       (Fraction(1, 4), r'sample rate 0\.25 Hz is not a whole number'),
                       (0, r'sample rate 0 Hz is not positive'), (-44100, r'sample rate -44100\.0 Hz is not positive'),
                       (float('inf'), r'sample rate inf Hz is not a whole number'), (float('-inf'), r'sample rate -inf Hz is not a whole number'),
                       (float('nan'), r'sample rate nan Hz is not a whole number')):
        with pytest.raises(ValueError, match=msg):
            aiff_scan(_write(tmp_path, 'r.aif', aref.aiff_bytes(bytes(8), value, 1, 16)))
    # a denormal and an unnormalised mantissa: still plain integer arithmetic
    with pytest.raises(ValueError, match='is not a whole number'):
        extended_rate(struct.pack('>HQ', 0, 1))
    assert extended_rate(struct.pack('>HQ', 16383 + 63, 44100)) == 44100


# ---- files the standard library wrote ----------------------------------------------------------------------------------------
def test_files_written_by_aifc(nafp, tmp_path):
    """AIFF at 1 .. 4 bytes and AIFC ULAW / ALAW written by `aifc`: the scan, and the host decoders on the body against the samples
    handed to the writer (for G.711 against audioop's expansion of the stored bytes)."""
    aifc, audioop = _stdlib('aifc'), _stdlib('audioop')
    aiff_scan = _scans()[0]
    lib = nafp._lib.load()
    rng = np.random.default_rng(5)
    for width, fmt in ((1, 's8'), (2, 's16be'), (3, 's24be'), (4, 's32be')):
        for ch in (1, 2):
            x = rng.integers(-(1 << (8 * width - 1)), 1 << (8 * width - 1), size=(50, ch))
            be = b''.join(int(v).to_bytes(width, 'big', signed=True) for v in x.reshape(-1))
            path = str(tmp_path / f'w{width}{ch}.aiff')
            with aifc.open(path, 'wb') as w:
                w.setnchannels(ch); w.setsampwidth(width); w.setframerate(44100)
                w.writeframes(be)
            got = aiff_scan(path)
            assert (got['rate'], got['channels'], got['format'], got['width'], got['block_align'], got['n_frames'], got['codec']) == \
                   (44100, ch, fmt, width, ch * width, 50, None)
            body = open(path, 'rb').read()[got['offset']:got['offset'] + 50 * ch * width]
            st, q = _ingest_host(nafp, nafp._lib.INGEST_FORMATS[fmt][0], body, 50 * ch)
            want = {1: x << 16, 2: x << 8, 3: x, 4: np.minimum((x + 128) >> 8, 2 ** 23 - 1)}[width].reshape(-1)
            assert st == 0 and np.array_equal(q, want)
    pcm = rng.integers(-32768, 32768, size=2 * 80).astype('<i2')
    for ctype, name, expand in ((b'ULAW', 'ulaw', audioop.ulaw2lin), (b'ALAW', 'alaw', audioop.alaw2lin)):
        path = str(tmp_path / f'{name}.aifc')
        with aifc.open(path, 'wb') as w:
            w.setnchannels(2); w.setsampwidth(2); w.setframerate(8000); w.setcomptype(ctype, name.encode())
            w.writeframes(pcm.tobytes())
        got = aiff_scan(path)
        assert (got['rate'], got['channels'], got['format'], got['codec'], got['block_align'], got['n_frames'], got['samples_per_block']) == \
               (8000, 2, name, name, 2, 80, 1)
        body = open(path, 'rb').read()[got['offset']:got['offset'] + 160]
        out = np.zeros(160, np.int16)
        buf = np.frombuffer(body, np.uint8).copy()
        assert lib.nafp_codec_decode_host(nafp._lib.CODECS[name], 2, 2, buf.ctypes.data_as(ctypes.c_void_p), 80, out.ctypes.data_as(ctypes.c_void_p)) == 0
        assert np.array_equal(out, np.frombuffer(expand(body, 2), '<i2'))


def test_files_written_by_sunau(nafp, tmp_path):
    sunau, audioop = _stdlib('sunau'), _stdlib('audioop')
    au_scan = _scans()[1]
    rng = np.random.default_rng(6)
    for width, fmt in ((2, 's16be'), (3, 's24be'), (4, 's32be')):
        x = rng.integers(-(1 << (8 * width - 1)), 1 << (8 * width - 1), size=(40, 2))
        path = str(tmp_path / f'w{width}.au')
        with sunau.open(path, 'wb') as w:
            w.setnchannels(2); w.setsampwidth(width); w.setframerate(16000); w.setcomptype('NONE', 'not compressed')
            w.writeframes(b''.join(int(v).to_bytes(width, 'big', signed=True) for v in x.reshape(-1)))
        got = au_scan(path)
        assert (got['rate'], got['channels'], got['format'], got['width'], got['block_align'], got['n_frames']) == (16000, 2, fmt, width, 2 * width, 40)
        body = open(path, 'rb').read()[got['offset']:]
        st, q = _ingest_host(nafp, nafp._lib.INGEST_FORMATS[fmt][0], body, 80)
        assert st == 0 and np.array_equal(q, {2: x << 8, 3: x, 4: np.minimum((x + 128) >> 8, 2 ** 23 - 1)}[width].reshape(-1))
    path = str(tmp_path / 'u.au')
    pcm = rng.integers(-32768, 32768, size=90).astype('<i2')
    with sunau.open(path, 'wb') as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(8000); w.setcomptype('ULAW', 'u')
        w.writeframes(pcm.tobytes())
    got = au_scan(path)
    assert (got['rate'], got['channels'], got['format'], got['codec'], got['n_frames'], got['block_align']) == (8000, 1, 'ulaw', 'ulaw', 90, 1)
    body = open(path, 'rb').read()[got['offset']:]
    out = np.zeros(90, np.int16)
    buf = np.frombuffer(body, np.uint8).copy()
    assert nafp._lib.load().nafp_codec_decode_host(2, 1, 1, buf.ctypes.data_as(ctypes.c_void_p), 90, out.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(out, np.frombuffer(audioop.ulaw2lin(body, 2), '<i2'))


def test_qt_packets_equal_audioop(nafp):
    """20,000 random packets with a step index <= 88: the restatement and the host decoder equal audioop.adpcm2lin, given the header
    state and the nibbles swapped within each byte (audioop takes the high nibble first)."""
    audioop = _stdlib('audioop')
    rng = np.random.default_rng(7)
    pk = rng.integers(0, 256, size=(20000, 34), dtype=np.uint8)
    pk[:, 1] = (pk[:, 1] & 0x80) | rng.integers(0, 89, size=20000).astype(np.uint8)
    ref = aref.qt_decode(1, pk.tobytes()).reshape(20000, 64)
    assert np.array_equal(_qt_host(nafp, 1, pk.tobytes()).reshape(20000, 64), ref)
    swapped = ((pk[:, 2:] << 4) | (pk[:, 2:] >> 4)).astype(np.uint8)
    for i in range(20000):
        h = (int(pk[i, 0]) << 8) | int(pk[i, 1])
        pred = (h & 0xff80) - (65536 if h & 0x8000 else 0)
        want = np.frombuffer(audioop.adpcm2lin(swapped[i].tobytes(), 2, (pred, h & 0x7f))[0], '<i2')
        assert np.array_equal(ref[i], want), i


# ---- the host decoders ----------------------------------------------------------------------------------------------------
def _corners(fmt):
    """Bytes of the corner values of a new format, as the file holds them."""
    if fmt == 's8':
        return bytes(range(256))
    le = aref.FORMATS[fmt][2]
    width = aref.FORMATS[fmt][1]
    if le in ('s16', 's24', 's32'):
        bits = 8 * width
        vals = [0, 1, -1, 2, -2, 127, 128, 129, -127, -128, -129, 255, 256, -256, (1 << (bits - 1)) - 1, -(1 << (bits - 1)),
                (1 << (bits - 1)) - 128, (1 << (bits - 1)) - 129, -(1 << (bits - 1)) + 1, 1 << (bits - 2), 0x1234 if bits == 16 else 0x123456]
        return b''.join(int(v).to_bytes(width, 'big', signed=True) for v in vals)
    dt = '>f4' if le == 'f32' else '>f8'
    tiny = np.finfo(np.dtype(dt).newbyteorder('=')).tiny
    vals = [0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1 - 2.0 ** -23, 2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -25, 5 * 2.0 ** -25, -(2.0 ** -24), 1.5 * 2.0 ** -23,
            2.5 * 2.0 ** -23, np.nan, -np.nan, np.inf, -np.inf, tiny, -tiny, tiny / 4, 1e30, -1e30, 0.999999999, 0.3, -0.7]
    with np.errstate(over='ignore'):
        return np.array(vals, dt).tobytes()


@pytest.mark.parametrize('fmt', list(aref.FORMATS))
def test_ingest_decode_host_new_codes(nafp, fmt):
    """All 256 s8 values, the corner values of each width, NaN / infinities / denormals big-endian, 10,000 random samples per
    code: the host decoder equals the restatement, and equals the little-endian code on the reversed bytes."""
    code, width, le = aref.FORMATS[fmt]
    assert nafp._lib.INGEST_FORMATS[fmt] == (code, width)
    rng = np.random.default_rng(code)
    for data in (_corners(fmt), rng.integers(0, 256, size=10000 * width, dtype=np.uint8).tobytes()):
        n = len(data) // width
        st, q = _ingest_host(nafp, code, data, n)
        assert st == 0 and np.array_equal(q, aref.decode(fmt, data))
        if le is not None:
            st, q_le = _ingest_host(nafp, iref.FORMATS[le][0], aref.reverse(data, width), n)
            assert st == 0 and np.array_equal(q, q_le)
        else:
            st, q_u8 = _ingest_host(nafp, iref.FORMATS['u8'][0], bytes((b + 128) & 255 for b in data), n)
            assert st == 0 and np.array_equal(q, q_u8)
    if fmt == 's8':
        assert np.array_equal(aref.decode('s8', bytes(range(256))), (np.arange(256, dtype=np.int64) + 128) % 256 - 128 << 16)


def test_ingest_codes_outside_the_contract(nafp):
    """0, 7, 9 .. 17 (17 = BE | U8), 23, 24 (BE | S8) and everything above are NAFP_ERR_UNSUPPORTED from every entry point."""
    lib = nafp._lib.load()
    unsupported = 2                                                     # NAFP_ERR_UNSUPPORTED
    buf = np.zeros(64, np.uint8)
    q = np.zeros(8, np.int32)
    valid = {1, 2, 3, 4, 5, 6, 8, 18, 19, 20, 21, 22}
    assert {c for c, _ in nafp._lib.INGEST_FORMATS.values()} == valid
    for code in list(range(-2, 70)) + [2 | 64, 2 | 128, 18 | 256, 1 << 20, -(1 << 31) | 18]:
        st = lib.nafp_ingest_decode_host(code, buf.ctypes.data_as(ctypes.c_void_p), 4, q.ctypes.data_as(ctypes.c_void_p))
        assert st == (0 if code in valid else unsupported), code
        piece = np.array([(0, 0, 4, 4, 0, 0, 4, 1, code, 0)], dtype=nafp._lib.INGEST_PIECE_DTYPE)
        st = lib.nafp_ingest_check_pieces_host(8000, 8000, piece.ctypes.data_as(ctypes.c_void_p), 1, 64, 8)
        assert st == (0 if code in valid else unsupported), code


def test_qt_geometry_and_host_decode(nafp):
    """The geometry grid of code 6 (code 5 stays outside), and random-byte packets -- header indices above 88 and predictors that
    saturate at both rails among them -- through the host decoder against the restatement."""
    lib = nafp._lib.load()
    for ch in (-1, 0, 1, 2, 3):
        for align in (33, 34, 35, 67, 68, 69, 102):
            want = 64 if (ch, align) in ((1, 34), (2, 68)) else -1
            assert lib.nafp_codec_samples_per_block(6, ch, align) == want, (ch, align)
            assert lib.nafp_codec_samples_per_block(5, ch, align) == -1
            assert (lib.nafp_codec_blocks_per_group(6, ch, align) > 0) == (want > 0)
            if want < 0:
                assert lib.nafp_codec_decode_host(6, ch, align, None, 0, None) != 0
    assert nafp._lib.CODECS['qtima4'] == 6
    rng = np.random.default_rng(8)
    for ch in (1, 2):
        pk = rng.integers(0, 256, size=(3000, ch, 34), dtype=np.uint8)
        pk[:500, :, 1] |= 0x7f                                          # index 127 -> 88
        pk[500:700, :, 0], pk[500:700, :, 2:] = 0x7f, 0x77              # climbing from +32640 with the largest steps
        pk[700:900, :, 0], pk[700:900, :, 2:] = 0x80, 0xff              # falling from -32768
        got = _qt_host(nafp, ch, pk.tobytes())
        assert np.array_equal(got, aref.qt_decode(ch, pk.tobytes()))
        g = got.reshape(3000, 64, ch)
        assert g[500:700].max() == 32767 and g[700:900].min() == -32768
    # the encoder of the restatement follows a signal, so that what the GPU tests feed is audio: 4 bits per sample keep the error
    # of such a signal some 20 dB below it; 18 dB (a factor of 8 in amplitude) is asked
    x = cref.music(64 * 40, 22050, 2, 3)
    y = aref.qt_decode(2, aref.qt_encode(x, 2)).reshape(-1, 2).astype(np.int64)
    assert np.sqrt(np.mean((y - x)[64:] ** 2.0)) < np.sqrt(np.mean(x ** 2.0)) / 8


# ---- refusals, the switch, the host readers ---------------------------------------------------------------------------------
def test_refusals_by_name(nafp, tmp_path):
    aiff_scan, au_scan, dispatch = _scans()

    def refused(msg, name, data, scan=dispatch, **kw):
        with pytest.raises(ValueError, match=msg):
            scan(_write(tmp_path, name, data), **kw)

    for ctype in (b'MAC3', b'MAC6', b'GSM ', b'QDMC', b'G722', b'ACE2', b'ACE8', b'Qclp', b'rt24', b'SOWT'):
        refused(rf"x\.aifc: AIFC compression type '{ctype.decode()}' is not taken", 'x.aifc', aref.aifc_bytes(ctype, bytes(64), 8000, 1, 16))
    refused(r'x\.aifc: Apple IMA4 \(ima4\) with 3 channels; 1 or 2 are taken', 'x.aifc', aref.aifc_bytes(b'ima4', bytes(102), 8000, 3, 16))
    refused(r'x\.aif: 9 channels; 1 to 8 are taken', 'x.aif', aref.aiff_bytes(bytes(36), 8000, 9, 16))
    refused(r'x\.aif: 0 channels; 1 to 8 are taken', 'x.aif', aref.aiff_bytes(bytes(36), 8000, 0, 16))
    refused(r'x\.aif: no COMM chunk', 'x.aif', aref.aiff_bytes(bytes(36), 8000, 1, 16, comm=False))
    refused(r'x\.aif: no SSND chunk', 'x.aif', aref.aiff_bytes(bytes(36), 8000, 1, 16, ssnd=False))
    refused(r'x\.aif: sampleSize 0; 1 to 32 bits are taken', 'x.aif', aref.aiff_bytes(bytes(36), 8000, 1, 0))
    refused(r'x\.aif: sampleSize 33', 'x.aif', aref.aiff_bytes(bytes(36), 8000, 1, 33))
    refused(r"16-bit samples of AIFC type 'raw '", 'x.aifc', aref.aifc_bytes(b'raw ', bytes(36), 8000, 1, 16))
    refused(r'x\.au: a little-endian AU header \(magic dns\.\) is not taken', 'x.au', aref.au_bytes('s16be', bytes(36), 8000, 1, magic=b'dns.'))
    refused(r'x\.au: AU encoding 23 \(G\.721 ADPCM\) is not taken', 'x.au', aref.au_bytes(23, bytes(36), 8000, 1))
    for enc in (24, 25, 26):
        refused(rf'x\.snd: AU encoding {enc} \(G\.72[23].*\) is not taken', 'x.snd', aref.au_bytes(enc, bytes(36), 8000, 1))
    refused(r'x\.au: AU encoding 0 is not taken', 'x.au', aref.au_bytes(0, bytes(36), 8000, 1))
    refused(r'x\.au: AU encoding 8 is not taken', 'x.au', aref.au_bytes(8, bytes(36), 8000, 1))
    refused(r'x\.au: 9 channels', 'x.au', aref.au_bytes('ulaw', bytes(36), 8000, 9))
    refused(r'x\.au: AU data offset 20', 'x.au', aref.au_bytes('ulaw', bytes(36), 8000, 1, header=20))
    wav = iref.wav_bytes('s16', bytes(64), 8000, 1)
    refused(r'x\.aif: neither an AIFF / AIFF-C nor an AU file \(it holds RIFF bytes\)', 'x.aif', wav)
    refused(r'x\.aif: not an AIFF / AIFF-C file \(it holds RIFF bytes\)', 'x.aif', wav, scan=aiff_scan)
    refused(r'x\.au: not an AU file', 'x.au', wav, scan=au_scan)
    refused(r'x\.snd: neither an AIFF', 'x.snd', b'fLaC' + bytes(60))
    # with fs, a rate that cannot be brought to it: the reference's wording
    refused(r'Sample rate should be 8000 but got 8001', 'x.aif', aref.aiff_bytes(bytes(36), 8001, 1, 16), fs=8000)
    refused(r'Sample rate should be 8000 but got 300000', 'x.au', aref.au_bytes('s16be', bytes(36), 300000, 1), fs=8000)
    refused(r'Sample rate should be 8000 but got 8001', 'x.aifc', aref.aifc_bytes(b'ima4', bytes(34), 8001, 1, 16), fs=8000)
    assert dispatch(_write(tmp_path, 'ok.aif', aref.aiff_bytes(bytes(36), 44100, 1, 16)), fs=8000)['rate'] == 44100


def test_switch_and_host_readers(nafp, tmp_path, monkeypatch):
    """NAFP_INGEST_AIFF=1 alone turns the whole chain on; without it -- also with NAFP_INGEST_FLAC=1 alone -- an `.aif` name raises
    NotImplementedError as before; what materialises samples on the host raises 'on the device only' for such files, a 16-bit mono
    `sowt` file at the model rate included; the directory glob merges the names in, sorted by path."""
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    from neural_audio_fp_amd.model.utils.dataloader_keras import PcmStore, PcmArena
    from neural_audio_fp_amd.model.utils import ingest as ig, codecs as cd, flac as fl, resample as rs
    from neural_audio_fp_amd.model.dataset import _audio_files
    x = cref.music(9000, 8000, 1, 1)
    files = [_write(tmp_path, 'a.aif', aref.aiff_bytes(x.astype('>i2').tobytes(), 8000, 1, 16)),
             _write(tmp_path, 'b.AIFC', aref.aifc_bytes(b'sowt', x.astype('<i2').tobytes(), 8000, 1, 16)),
             _write(tmp_path, 'c.aifc', aref.aifc_bytes(b'ima4', aref.qt_encode(cref.music(9000, 44100, 2, 2), 2), 44100, 2, 16)),
             _write(tmp_path, 'd.au', aref.au_bytes('ulaw', cref.encode('ulaw', x, 1, 1), 8000, 1)),
             _write(tmp_path, 'e.SND', aref.au_bytes('s16be', x.astype('>i2').tobytes(), 8000, 1, header=40)),
             _write(tmp_path, 'f.aiff', aref.aiff_bytes(bytes(3 * 2 * 500), 44100, 2, 24))]
    _write(tmp_path, 'g.wav', iref.wav_bytes('s16', x.astype('<i2').tobytes(), 8000, 1))
    _write(tmp_path, 'h.txt', b'.snd')
    for envs in ((), ('NAFP_INGEST_FLAC',), ('NAFP_INGEST_CODECS',), ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY')):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k in envs:
            monkeypatch.setenv(k, '1')
        assert not rs.switches().aiff
        for fn in files:
            with pytest.raises(NotImplementedError, match='^' + fn[-3:] + '$'):
                SegmentSource([fn], bsz=4)
            with pytest.raises(NotImplementedError, match='^' + fn[-3:] + '$'):
                PcmStore([fn], 8000)
        assert _audio_files(str(tmp_path) + '/**/') == [str(tmp_path / 'g.wav')]
    for envs in (('NAFP_INGEST_AIFF',), SWITCHES):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k in envs:
            monkeypatch.setenv(k, '1')
        sw = rs.switches()
        assert sw == rs.Switches(True, True, True, True, True, len(envs) > 1)
        assert cd.enabled() and ig.enabled() and fl.enabled()
        assert _audio_files(str(tmp_path) + '/**/') == sorted(files + [str(tmp_path / 'g.wav')])
        src = SegmentSource(files, bsz=4)
        assert src.aiff and src.ingest and src.format == ['s16be', 's16', 'qtima4', 'ulaw', 's16be', 's24be'] and all(src.resampled)
        assert [e.kind for e in src.files] == ['pcm', 'pcm', 'codec', 'codec', 'pcm', 'pcm']
        assert src.spb == [1, 1, 64, 1, 1, 1] and src.block_align == [2, 2, 68, 1, 2, 6]
        assert src.n_frames[:2] == [9000, 9000] and src.n_frames[3:5] == [9000, 9000] and src.n_in[2] == 64 * 141
        assert ig.rates_summary(src)['rates'] == {'8000x1xs16be': 2, '8000x1xs16': 1, '44100x2xqtima4': 1, '8000x1xulaw': 1, '44100x2xs24be': 1}
        for row in (0, int(src.file_first[1]), int(src.file_first[2])):
            with pytest.raises(NotImplementedError, match='on the device only'):
                src.read_rows(row, row + 1)
        store = PcmStore(files, 8000)
        assert list(store.n_frames) == src.n_frames and all(store.resampled)
        with pytest.raises(NotImplementedError, match='on the device only'):
            PcmArena([store]).host()
        with pytest.raises(ValueError, match=r'g\.aif: neither an AIFF'):
            SegmentSource([_write(tmp_path / '..', 'g.aif', iref.wav_bytes('s16', bytes(64), 8000, 1))], bsz=4)
    # the launch plan of such files needs no branch of its own: a codec stage for the packets, direct pieces for the rest
    launch = ig.LaunchPlan(8000)
    for e in src.files:
        launch.add(e, 0, min(e.n_frames, 1500), 0)
    work = launch.work(16)
    assert [s.prepass is not None for s in work.stages] == [False, True]
    assert sorted(int(c) for c in work.stages[1].prepass.pieces['codec']) == [2, 6]
    assert sorted(int(f) for rows in work.stages[0].by_rate.values() for f in rows['format']) == [2, 18, 18, 19]
