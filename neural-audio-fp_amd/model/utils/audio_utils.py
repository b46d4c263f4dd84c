"""Input contract of the hot path: WAV files -> fixed-length int16 segments.

Mirrors what the reference's loader delivers to `m_pre` during `generate`
(model/utils/audio_utils.py:140-218 `get_fns_seg_list` mode 'all', :221-264
`load_audio`; model/utils/dataloader_keras.py:223-228, 303-306 with shuffle=False and
no augmentation): segments of FS*DUR samples every FS*HOP samples, the tail zero-
padded, in file order then segment order.

Differences in mechanism, not in result: each file is opened ONCE and read whole
(the reference re-opens the file for every segment and grows each batch with
np.vstack row by row, dataloader_keras.py:389-397), and segments stay int16 -- the
HIP front end scales by 2^-15 itself, which is exactly `x / 2**15`
(audio_utils.py:245-246) in float32.
"""
import os
import struct
import wave

import numpy as np

from . import codecs as cd
from . import flac as fl
from . import ingest as ig
from . import resample as rs
from . import varispeed as vs


def n_segments(n_frames, fs=8000, duration=1., hop=.5):
    """audio_utils.py:171-177."""
    n_seg_frames, n_hop_frames = fs * duration, fs * hop
    if n_frames > n_seg_frames:
        return int((n_frames - n_seg_frames + n_hop_frames) // n_hop_frames)
    return 1


def _riff_chunks(filename, keep=(b'fmt ',), fmt_min=0):
    """Walk of a RIFF/WAVE file's chunks up to the data chunk, WITHOUT reading the samples: ([(id, declared size, body as stored,
    pad byte included)] of the chunks named in `keep`, in file order; bytes of the data chunk that the file holds; byte offset of
    the first sample).  fmt_min: a fmt chunk shorter than this is refused where it stands."""
    with open(filename, 'rb') as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b'RIFF' or head[8:12] != b'WAVE':
            raise ValueError(f'{filename}: not a RIFF/WAVE file')
        size = os.fstat(f.fileno()).st_size
        chunks, seen_fmt, off = [], False, 12              # off: where the next chunk header stands (no tell() per file)
        while True:
            hdr = f.read(8)
            if len(hdr) < 8:
                raise ValueError(f'{filename}: no data chunk')
            cid, csz = hdr[:4], struct.unpack('<I', hdr[4:])[0]
            if cid == b'data':
                if not seen_fmt:
                    raise ValueError(f'{filename}: data chunk before fmt chunk')
                return chunks, min(csz, size - off - 8), off + 8
            if cid in keep:
                body = f.read(csz + (csz & 1))
                if fmt_min and cid == b'fmt ' and min(csz, len(body)) < fmt_min:
                    raise ValueError(f'{filename}: fmt chunk of {min(csz, len(body))} bytes')
                chunks.append((cid, csz, body))
                seen_fmt = seen_fmt or cid == b'fmt '
            else:
                f.seek(csz + (csz & 1), 1)
            off += 8 + csz + (csz & 1)


def riff_scan(filename):
    """Header scan of a RIFF/WAVE file WITHOUT reading the samples: (fs, channels, sample width in
    bytes, byte offset of the first sample, frame count).  What `wave.open(...).getnframes()` reports
    (audio_utils.py:160-169), plus where the data chunk starts, so that a sample range can be read
    straight into a staging buffer."""
    chunks, size, off = _riff_chunks(filename)
    tag, ch, rate, _, align, bits = struct.unpack('<HHIIHH', chunks[-1][2][:16])          # the last fmt chunk before the data
    return rate, ch, bits // 8, off, size // align


_WAVE_TAGS = {0x0002: 'ADPCM', 0x0006: 'A-law', 0x0007: 'mu-law', 0x0011: 'IMA ADPCM', 0x0031: 'GSM 6.10', 0x0050: 'MPEG',
              0x0055: 'MPEG layer 3'}
_GUID_TAIL = bytes.fromhex('000000001000800000aa00389b71')          # KSDATAFORMAT_SUBTYPE_*: the tag as 2 bytes, then this
_PCM_WIDTHS = {1: 'u8', 2: 's16', 3: 's24', 4: 's32'}
_FLOAT_WIDTHS = {4: 'f32', 8: 'f64'}


_CODEC_TAGS = {0x0006: ('alaw', 'A-law'), 0x0007: ('ulaw', 'mu-law'), 0x0011: ('ima4', 'IMA ADPCM'), 0x0002: ('ms4', 'MS ADPCM')}
_MS_COEFS = (256, 0, 512, -256, 0, 0, 192, 64, 240, 0, 460, -208, 392, -232)


def _codec_header(filename, fmt, tag, ch, align, bits):
    """The checks of a codec file's fmt chunk (riff_scan_ex with codecs=True): (format name, samples per block), or ValueError by
    name.  `tag` is the format tag, or for an extensible header the tag its sub-format GUID carries (6 or 7 only)."""
    name, title = _CODEC_TAGS[tag]
    if name in ('alaw', 'ulaw'):
        if bits != 8:
            raise ValueError(f'{filename}: {bits}-bit {title} samples; G.711 is taken at 8 bits')
        if align != ch:
            raise ValueError(f'{filename}: block_align {align} != {ch} channels of 1-byte {title} samples')
        return name, 1
    if ch > 2:
        raise ValueError(f'{filename}: {title} with {ch} channels; 1 or 2 are taken')
    if bits != 4:
        raise ValueError(f'{filename}: {bits}-bit {title}; 4 bits are taken')
    if align > cd.MAX_BLOCK_ALIGN:
        raise ValueError(f'{filename}: {title} block_align {align}; up to {cd.MAX_BLOCK_ALIGN} is taken')
    spb = cd.samples_per_block(name, ch, align)
    if spb < 0:
        raise ValueError(f'{filename}: block_align {align} is not a block of {ch}-channel {title}')
    if len(fmt) < 20:
        raise ValueError(f'{filename}: {title} fmt chunk of {len(fmt)} bytes holds no wSamplesPerBlock')
    w_spb, = struct.unpack('<H', fmt[18:20])
    if w_spb != spb:
        raise ValueError(f'{filename}: wSamplesPerBlock {w_spb} != {spb}, which {title} blocks of {align} bytes hold')
    if name == 'ms4':
        if len(fmt) < 22:
            raise ValueError(f'{filename}: {title} fmt chunk of {len(fmt)} bytes holds no wNumCoef')
        n_coef, = struct.unpack('<H', fmt[20:22])
        if n_coef != 7:
            raise ValueError(f'{filename}: {title} wNumCoef {n_coef}; the 7 standard coefficient pairs are taken')
        if len(fmt) < 50 or struct.unpack('<14h', fmt[22:50]) != _MS_COEFS:
            raise ValueError(f'{filename}: {title} coefficient table differs from the standard one')
    return name, spb


def riff_scan_ex(filename, fs=None, codecs=False):
    """Header scan of a RIFF/WAVE file for the general ingest (NAFP_INGEST_ANY=1, utils/ingest.py), WITHOUT reading the samples:
    {'rate', 'channels', 'format' ('u8' | 's16' | 's24' | 's32' | 'f32' | 'f64'), 'width' (bytes per sample in the file),
    'block_align', 'offset' (byte offset of the first sample), 'n_frames'}.
    Taken: format tag 1 (PCM) at 8 / 16 / 24 / 32 bits, tag 3 (IEEE float) at 32 / 64 bits, and tag 0xFFFE (extensible) whose
    sub-format GUID is the PCM or the IEEE-float one -- there the container width is block_align / channels (samples are
    MSB-justified in it, so wValidBitsPerSample is not needed); 1 to 8 channels; block_align == channels * width.  Everything
    else raises ValueError by name, and with `fs` given so does a rate that cannot be brought to fs, in the reference's wording
    (audio_utils.py:160-169).
    codecs=True (NAFP_INGEST_CODECS=1, utils/codecs.py): tags 6 (A-law), 7 (mu-law), 0x11 (IMA ADPCM) and 2 (MS ADPCM) are taken
    too, and an extensible header whose sub-format GUID carries 6 or 7 (extensible ADPCM stays refused).  G.711: 8 bits,
    block_align == channels.  ADPCM: 4 bits, 1 or 2 channels, block_align <= 4096 and of the codec's form, wSamplesPerBlock
    equal to what block_align holds; MS: wNumCoef == 7 and the standard pairs.  'format' is then 'alaw' | 'ulaw' | 'ima4' |
    'ms4', 'width' 0, and the dict gains 'codec' (the same name; None for a PCM / float file) and 'samples_per_block' (spb; 1
    for a PCM / float file).  n_frames: whole = (data bytes // block_align) * spb, a trailing partial block ignored; a `fact`
    chunk whose first uint32 n satisfies 0 < n <= whole gives n_frames = n."""
    fact = None
    chunks, csz, off = _riff_chunks(filename, (b'fmt ', b'fact') if codecs else (b'fmt ',), fmt_min=16)
    for cid, size, body in chunks:
        if cid == b'fmt ':
            fmt = body[:size]
        elif size >= 4 and len(body) >= 4:
            fact, = struct.unpack('<I', body[:4])
    tag, ch, rate, _, align, bits = struct.unpack('<HHIIHH', fmt[:16])
    if ch < 1 or ch > 8:
        raise ValueError(f'{filename}: {ch} channels; 1 to 8 are taken')
    codec = None
    if tag == 0xFFFE:
        if len(fmt) < 40:
            raise ValueError(f'{filename}: extensible fmt chunk of {len(fmt)} bytes')
        guid = fmt[24:40]
        if codecs and guid[2:] == _GUID_TAIL and guid[:2] in (b'\x06\x00', b'\x07\x00'):
            codec = _codec_header(filename, fmt, guid[0], ch, align, bits)
        elif guid[2:] != _GUID_TAIL or guid[:2] not in (b'\x01\x00', b'\x03\x00'):
            raise ValueError(f'{filename}: extensible header with unknown sub-format GUID {guid.hex()}; taken: PCM, IEEE float' +
                             (', A-law, mu-law' if codecs else ''))
        kind = guid[0]
        if codec is None:
            if align % ch:
                raise ValueError(f'{filename}: block_align {align} is not a multiple of {ch} channels')
            width = align // ch
    elif tag in (1, 3):
        kind = tag
        if bits % 8:
            raise ValueError(f'{filename}: {bits}-bit samples; taken: PCM at 8 / 16 / 24 / 32 bits, IEEE float at 32 / 64')
        width = bits // 8
    elif codecs and tag in _CODEC_TAGS:
        codec = _codec_header(filename, fmt, tag, ch, align, bits)
    else:
        name = _WAVE_TAGS.get(tag)
        raise ValueError(f'{filename}: WAVE format tag 0x{tag:04x}' + (f' ({name})' if name else '') +
                         ' is not taken; taken: PCM (1), IEEE float (3), extensible (0xfffe) holding either')
    if codec is not None:
        name, spb = codec
        if fs is not None:
            ig.check_rate(rate, fs)
        whole = (csz // align) * spb
        return {'rate': rate, 'channels': ch, 'format': name, 'width': 0, 'block_align': align, 'offset': off,
                'n_frames': fact if fact is not None and 0 < fact <= whole else whole, 'codec': name, 'samples_per_block': spb}
    name = (_PCM_WIDTHS if kind == 1 else _FLOAT_WIDTHS).get(width)
    if name is None:
        raise ValueError(f'{filename}: {8 * width}-bit {"PCM" if kind == 1 else "IEEE float"} samples; taken: PCM at 8 / 16 / 24 / 32 '
                         f'bits, IEEE float at 32 / 64')
    if align != ch * width:
        raise ValueError(f'{filename}: block_align {align} != {ch} channels * {width} bytes per sample')
    if fs is not None:
        ig.check_rate(rate, fs)
    info = {'rate': rate, 'channels': ch, 'format': name, 'width': width, 'block_align': align, 'offset': off,
            'n_frames': csz // align}
    if codecs:
        info['codec'], info['samples_per_block'] = None, 1
    return info


def flac_scan(filename, fs=None):
    """STREAMINFO and frame index of a FLAC file for the general ingest (NAFP_INGEST_FLAC=1, utils/flac.py), one pass over the
    file: what riff_scan_ex returns -- 'format' is 'flacNN' (NN = bits per sample), 'codec' 'flac', 'width' / 'block_align' /
    'offset' 0, 'samples_per_block' 1 -- plus 'bps', 'frames' (per frame the byte offset, first sample as coded, byte length and
    block size: a structured array) and 'index' (flac.Index over them).  n_frames is STREAMINFO's total when that is non-zero and
    not above the indexed sum, otherwise the indexed sum.  Refused by name (ValueError): Ogg FLAC, no `fLaC` marker, a first
    metadata block that is not a 34-byte STREAMINFO, a depth other than 8 / 12 / 16 / 20 / 24 bits, a maximum block size above
    16384, a file without a valid frame, and with `fs` a rate that cannot be brought to fs."""
    with open(filename, 'rb') as f:
        data = f.read()
    info, frames = fl.scan(data)
    refusal = int(info['refusal'])
    if refusal == 4:
        raise ValueError(f"{filename}: {int(info['bps'])}-bit FLAC samples; {fl.REFUSALS[4]}")
    if refusal == 5:
        raise ValueError(f"{filename}: FLAC maximum block size {int(info['max_block'])}; {fl.REFUSALS[5]}")
    if refusal:
        raise ValueError(f'{filename}: {fl.REFUSALS[refusal]}')
    if len(frames) == 0:
        raise ValueError(f'{filename}: no valid FLAC frame found')
    rate, ch, bps = int(info['rate']), int(info['channels']), int(info['bps'])
    if fs is not None:
        ig.check_rate(rate, fs)
    total, indexed = int(info['total_samples']), int(info['indexed_samples'])
    return {'rate': rate, 'channels': ch, 'format': f'flac{bps}', 'width': 0, 'block_align': 0, 'offset': 0,
            'n_frames': total if 0 < total <= indexed else indexed, 'codec': 'flac', 'samples_per_block': 1, 'bps': bps,
            'frames': frames, 'index': fl.Index(frames, ch, bps, rate)}


AIFF_NAMES = ('.aif', '.aiff', '.aifc', '.au', '.snd')              # taken under NAFP_INGEST_AIFF=1, in any letter case
_AIFC_PCM = (b'NONE', b'twos', b'in24', b'in32')
_AIFC_G711 = {b'alaw': 'alaw', b'ALAW': 'alaw', b'ulaw': 'ulaw', b'ULAW': 'ulaw'}
_AIFC_FLOAT = {b'fl32': 'f32be', b'FL32': 'f32be', b'fl64': 'f64be', b'FL64': 'f64be'}
_BE_PCM = {1: 's8', 2: 's16be', 3: 's24be', 4: 's32be'}
_LE_PCM = {1: 's8', 2: 's16', 3: 's24', 4: 's32'}
_AU_ENCODINGS = {1: 'ulaw', 2: 's8', 3: 's16be', 4: 's24be', 5: 's32be', 6: 'f32be', 7: 'f64be', 27: 'alaw'}
_AU_REFUSED = {23: 'G.721 ADPCM', 24: 'G.722', 25: 'G.723 at 3 bits', 26: 'G.723 at 5 bits'}


def is_aiff_name(filename):
    """A name that NAFP_INGEST_AIFF=1 makes eligible: it ends in one of AIFF_NAMES, in any letter case."""
    return filename.lower().endswith(AIFF_NAMES)


def extended_rate(ten):
    """The 80-bit extended value of an AIFF COMM chunk (sign, 15-bit exponent biased by 16383, 64-bit mantissa with its integer bit)
    as a whole number of Hz, in integers.  ValueError -- its text names the value -- for anything that is not a positive whole
    number: a fraction, zero, a negative value, an infinity, a NaN."""
    se, mant = struct.unpack('>HQ', ten)
    neg, e = se >> 15, se & 0x7fff
    if e == 0x7fff:                                                  # an infinity: no mantissa bit below the integer bit
        text = 'nan' if mant & ((1 << 63) - 1) else '-inf' if neg else 'inf'
        raise ValueError(f'sample rate {text} Hz is not a whole number')
    shift = e - 16383 - 63                                          # the value is mant * 2^shift
    if neg or mant == 0:
        raise ValueError('sample rate {} Hz is not positive'.format('-{}'.format(_extended_text(mant, shift)) if neg and mant else '0'))
    if shift >= 0:
        if shift > 64:
            raise ValueError(f'sample rate 2^{e - 16383} Hz is out of range')
        return mant << shift
    if -shift >= 64 or mant & ((1 << -shift) - 1):
        raise ValueError(f'sample rate {_extended_text(mant, shift)} Hz is not a whole number')
    return mant >> -shift


def _extended_text(mant, shift):
    return repr(float(mant << shift)) if shift >= 0 else repr(mant / (1 << -shift))


def _sized_info(filename, fs, rate, ch, fmt, n_stated, n_bytes, off):
    """The scan dict of a header that gave `fmt` (a name of _lib.INGEST_FORMATS or codecs.CODECS) for `n_bytes` sample bytes at
    `off`: n_frames = min(stated units x spb, whole blocks present x spb)."""
    if ch < 1 or ch > 8:
        raise ValueError(f'{filename}: {ch} channels; 1 to 8 are taken')
    if fmt == 'qtima4':
        if ch > 2:
            raise ValueError(f'{filename}: Apple IMA4 (ima4) with {ch} channels; 1 or 2 are taken')
        width, align, spb, codec = 0, 34 * ch, 64, fmt
    elif fmt in cd.CODECS:
        width, align, spb, codec = 0, ch, 1, fmt
    else:
        width = ig.FORMATS[fmt][1]
        align, spb, codec = ch * width, 1, None
    if fs is not None:
        ig.check_rate(rate, fs)
    return {'rate': rate, 'channels': ch, 'format': fmt, 'width': width, 'block_align': align, 'offset': off,
            'n_frames': min(n_stated, max(n_bytes, 0) // align) * spb, 'codec': codec, 'samples_per_block': spb}


def aiff_scan(filename, fs=None):
    """Header scan of an AIFF / AIFF-C file (`FORM` ... `AIFF` | `AIFC`) for the general ingest (NAFP_INGEST_AIFF=1), WITHOUT reading
    the samples: the dict of riff_scan_ex(..., codecs=True).  Sizes are big-endian, chunks padded to even length and taken in any
    order (`SSND` before `COMM` is legal); the first sample stands at the SSND body + 8 + its `offset` field (blockSize is
    ignored); the rate is the COMM chunk's 80-bit value, a positive whole number of Hz (extended_rate).  A sampleSize of 1 .. 32
    bits is stored in ceil(bits / 8) bytes, left-justified, and that container is decoded as it stands.
    'format': AIFF and the AIFC types NONE / twos / in24 / in32 give 's8' | 's16be' | 's24be' | 's32be'; `sowt` the little-endian
    's8' | 's16' | 's24' | 's32'; `raw ` at 8 bits 'u8'; fl32 / FL32 'f32be', fl64 / FL64 'f64be'; alaw / ALAW / ulaw / ULAW the
    codecs 'alaw' / 'ulaw' (block_align = channels); `ima4` the codec 'qtima4' (1 or 2 channels, block_align 34 x channels, 64
    frames per block; numSampleFrames counts packets per channel).  n_frames = min(numSampleFrames x spb, whole blocks the file
    holds x spb).  Refused by name (ValueError): every other compression type, 0 or more than 8 channels, a missing COMM or SSND,
    a rate that is no positive whole number, and with `fs` a rate that cannot be brought to fs, in the reference's wording."""
    comm = ssnd = None
    with open(filename, 'rb') as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b'FORM' or head[8:12] not in (b'AIFF', b'AIFC'):
            raise ValueError(f'{filename}: not an AIFF / AIFF-C file' + (' (it holds RIFF bytes)' if head[:4] == b'RIFF' else ''))
        aifc = head[8:12] == b'AIFC'
        size = os.fstat(f.fileno()).st_size
        off = 12
        while off + 8 <= size:
            f.seek(off)
            hdr = f.read(8)
            if len(hdr) < 8:
                break
            cid, csz = hdr[:4], struct.unpack('>I', hdr[4:])[0]
            if cid == b'COMM' and comm is None:
                comm = f.read(csz)
            elif cid == b'SSND' and ssnd is None:
                first = f.read(8)
                if len(first) == 8:                                  # (first sample's byte, sample bytes the chunk states)
                    skip, = struct.unpack('>I', first[:4])
                    ssnd = (off + 16 + skip, csz - 8 - skip)
            off += 8 + csz + (csz & 1)
    if comm is None:
        raise ValueError(f'{filename}: no COMM chunk')
    if ssnd is None:
        raise ValueError(f'{filename}: no SSND chunk')
    if len(comm) < (22 if aifc else 18):
        raise ValueError(f'{filename}: COMM chunk of {len(comm)} bytes')
    ch, n_stated, bits = struct.unpack('>hIh', comm[:8])
    try:
        rate = extended_rate(comm[8:18])
    except ValueError as e:
        raise ValueError(f'{filename}: {e}') from None
    ctype = comm[18:22] if aifc else b'NONE'
    width = (bits + 7) // 8
    if ctype in _AIFC_PCM or ctype == b'sowt':
        if bits < 1 or bits > 32:
            raise ValueError(f'{filename}: sampleSize {bits}; 1 to 32 bits are taken')
        fmt = (_LE_PCM if ctype == b'sowt' else _BE_PCM)[width]
    elif ctype == b'raw ':
        if bits != 8:
            raise ValueError(f"{filename}: {bits}-bit samples of AIFC type 'raw '; 8 bits are taken")
        fmt = 'u8'
    elif ctype in _AIFC_FLOAT:
        fmt = _AIFC_FLOAT[ctype]
    elif ctype in _AIFC_G711:
        fmt = _AIFC_G711[ctype]
    elif ctype == b'ima4':
        fmt = 'qtima4'
    else:
        raise ValueError(f"{filename}: AIFC compression type '{ctype.decode('latin-1')}' is not taken; taken: NONE, twos, in24, in32, "
                         "sowt, raw, fl32, fl64, alaw, ulaw, ima4")
    data, stated = ssnd
    return _sized_info(filename, fs, rate, ch, fmt, n_stated, min(stated, size - data), data)


def au_scan(filename, fs=None):
    """Header scan of an AU / `.snd` file for the general ingest (NAFP_INGEST_AIFF=1), WITHOUT reading the samples: the dict of
    riff_scan_ex(..., codecs=True).  The header is big-endian: magic `.snd`, data offset (>= 24), data size (0xffffffff: to the end
    of the file), encoding, rate, channels.  Encodings 1 -> 'ulaw', 2 -> 's8', 3 -> 's16be', 4 -> 's24be', 5 -> 's32be',
    6 -> 'f32be', 7 -> 'f64be', 27 -> 'alaw'; n_frames = min(stated size, bytes present) // block_align.  Refused by name
    (ValueError): the G.721 / G.722 / G.723 encodings 23 .. 26, every other number, the byte-swapped magic `dns.` (a little-endian
    header), 0 or more than 8 channels, and with `fs` a rate that cannot be brought to fs, in the reference's wording."""
    with open(filename, 'rb') as f:
        head = f.read(24)
        size = os.fstat(f.fileno()).st_size
    if head[:4] == b'dns.':
        raise ValueError(f'{filename}: a little-endian AU header (magic dns.) is not taken')
    if len(head) < 24 or head[:4] != b'.snd':
        raise ValueError(f'{filename}: not an AU file' + (' (it holds RIFF bytes)' if head[:4] == b'RIFF' else ''))
    off, stated, enc, rate, ch = struct.unpack('>5I', head[4:24])
    if off < 24:
        raise ValueError(f'{filename}: AU data offset {off}; at least 24')
    if enc not in _AU_ENCODINGS:
        raise ValueError(f'{filename}: AU encoding {enc}' + (f' ({_AU_REFUSED[enc]})' if enc in _AU_REFUSED else '') +
                         ' is not taken; taken: 1 (mu-law), 2 .. 5 (PCM at 8 / 16 / 24 / 32 bits), 6, 7 (IEEE float), 27 (A-law)')
    if rate < 1:
        raise ValueError(f'{filename}: sample rate {rate} Hz is not positive')
    present = size - off
    return _sized_info(filename, fs, rate, ch, _AU_ENCODINGS[enc], 1 << 62, present if stated == 0xffffffff else min(stated, present), off)


def aiff_au_scan(filename, fs=None):
    """An AIFF_NAMES file: the name made it eligible, its first four bytes choose the parser; any other content is refused by name."""
    with open(filename, 'rb') as f:
        magic = f.read(4)
    if magic == b'FORM':
        return aiff_scan(filename, fs)
    if magic in (b'.snd', b'dns.'):
        return au_scan(filename, fs)
    raise ValueError(f'{filename}: neither an AIFF / AIFF-C nor an AU file' + (' (it holds RIFF bytes)' if magic == b'RIFF' else ''))


def wav_info(filename, fs):
    """Frame count of a 16-bit mono WAV; ValueError on a wrong sample rate
    (audio_utils.py:160-169)."""
    if filename[-3:] != 'wav':
        raise NotImplementedError(filename[-3:])
    with wave.open(filename, 'r') as w:
        if w.getframerate() != fs:
            raise ValueError('Sample rate should be {} but got {}'.format(str(fs), str(w.getframerate())))
        return w.getnframes()


def get_fns_seg_list(fns_list, fs=8000, duration=1., hop=None):
    """[[filename, seg_idx], ...] in file order then segment order (mode 'all')."""
    if hop is None:
        hop = duration
    out = []
    for fn in fns_list:
        for s in range(n_segments(wav_info(fn, fs), fs, duration, hop)):
            out.append([fn, s])
    return out


def read_wav_int16(filename):
    with wave.open(filename, 'r') as w:
        if w.getsampwidth() != 2 or w.getnchannels() != 1:
            raise ValueError(f'{filename}: expected 16-bit mono PCM')
        return np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16)


def file_segments(pcm, fs=8000, duration=1., hop=.5):
    """All segments of one file as an (n_segs, seg_len) int16 array, tail zero-padded
    (load_audio's `audio_arr[:len(x)] = x`, audio_utils.py:261-263)."""
    seg_len, hop_len = int(fs * duration), int(np.floor(hop * fs))
    n = n_segments(len(pcm), fs, duration, hop)
    need = (n - 1) * hop_len + seg_len
    if len(pcm) < need:
        pcm = np.concatenate([pcm, np.zeros(need - len(pcm), np.int16)])
    idx = np.arange(seg_len)[None, :] + hop_len * np.arange(n)[:, None]
    return pcm[idx]


class FileCatalog:
    """The files of a loader, each header scanned ONCE (the reference re-opens per segment) under the opt-in layers the environment
    sets (utils/resample.switches: the flags `resample`, `ingest`, `codecs`, `flac`, `aiff`).  With `aiff` a name ending in one of
    AIFF_NAMES is an AIFF / AIFF-C or AU file (aiff_au_scan): kind 'pcm' or 'codec' like a WAV file's, never read on the host, not
    even 16-bit mono at `fs`.  `files[f]` is the whole entry
    (ingest.FileEntry); the same as columns, one value per file: `n_frames` (the length at the model rate `fs`), `data_offset`,
    and what describes the file itself, `rate`, `channels`, `n_in` (its frame count), `resampled` (the device converts it: not
    16-bit mono at `fs`); with `ingest` also `format`, `block_align` and `spb` (frames per block_align bytes: 1 unless a codec).
    `flac_index[f]` is the frame index of a FLAC file, built here by one pass over it, and `flac_failed` (flac.FailedFrames, None
    without a FLAC file) collects on the device which of those frames failed their checks when decoded."""

    def __init__(self, fns, fs):
        self.fns, self.fs = list(fns), fs
        self.resample, self.ingest, self.codecs, self.flac, self.aiff, _ = rs.switches()
        rows, n_flac_frames = [], 0
        for fn in self.fns:
            aiff = self.aiff and is_aiff_name(fn)
            if fn[-3:] != 'wav' and not aiff and not (self.flac and fn[-5:].lower() == '.flac'):     # `.flac` in any letter case
                raise NotImplementedError(fn[-3:])
            if self.ingest:
                info = aiff_au_scan(fn, fs) if aiff else flac_scan(fn, fs) if fn[-3:] != 'wav' else riff_scan_ex(fn, fs, codecs=self.codecs)
                index = info.get('index')
                kind = 'flac' if index is not None else 'codec' if info['format'] in cd.CODECS else 'pcm'
                rate, ch, off, nfr = info['rate'], info['channels'], info['offset'], info['n_frames']
                native = not aiff and ig.is_native(info, fs)       # an AIFF / AU file is read on the device whatever it holds
                n_model = nfr if native else ig.n_out(nfr, rate, fs)
                fmt, align, spb = info['format'], info['block_align'], info.get('samples_per_block', 1)
            else:
                rate, ch, width, off, nfr = riff_scan(fn)
                kind, index, fmt, align, spb = 'pcm16', None, 's16', 2 * ch, 1
                if self.resample:
                    rs.check_file(fn, rate, ch, width, fs)
                    native = rate == fs and ch == 1
                    n_model = nfr if native else rs.n_out(nfr, rate, fs)
                else:
                    if rate != fs:
                        raise ValueError('Sample rate should be {} but got {}'.format(str(fs), str(rate)))
                    if width != 2 or ch != 1:
                        raise ValueError(f'{fn}: expected 16-bit mono PCM')
                    native, n_model = True, nfr
            rows.append((fn, kind, rate, ch, nfr, n_model, not native, off, fmt, align, spb, index, n_flac_frames))
            if index is not None:
                n_flac_frames += len(index)
        self.files = list(map(ig.FileEntry._make, rows))
        cols = dict(zip(ig.FileEntry._fields, map(list, zip(*self.files)))) if self.files else {k: [] for k in ig.FileEntry._fields}
        for col in ('n_frames', 'data_offset', 'rate', 'channels', 'n_in', 'resampled'):
            setattr(self, col, cols[col])
        for col in ('format', 'block_align', 'spb'):
            setattr(self, col, cols[col] if self.ingest else [])
        self.flac_index = {f: index for f, index in enumerate(cols['flac']) if index is not None} if self.flac else {}
        self.flac_failed = fl.FailedFrames([0 if index is None else len(index) for index in cols['flac']]) if self.flac_index else None


class SegmentSource(FileCatalog):
    """Ordered segments of a list of WAV files, served in consecutive batches.

    Counterpart of `genUnbalSequence(fns, bsz, n_anchor=bsz, shuffle=False,
    drop_the_last_non_full_batch=False)` as the generate path uses it
    (model/dataset.py:204-215): `.n_samples` segments, `len()` batches of `bsz`
    (the last one ragged), item i = segments [i*bsz, (i+1)*bsz) as int16 (n,1,T).

    step (utils/varispeed, None: off): every file is taken as played step / 2^24 times as fast.  The column `n_frames` is then
    the STRETCHED length n_out(model-rate length, step), from which the segment counts and `file_first` follow; `n_model` keeps
    the model-rate lengths (as `files[f].n_frames` does).  The stretch exists on the device only (iter_windows).
    """

    def __init__(self, fns_list, bsz, duration=1., hop=.5, fs=8000, step=None):
        super().__init__(fns_list, fs)
        self.bsz, self.duration, self.hop = int(bsz), duration, hop
        self.seg_len = int(fs * duration)
        self.hop_len = int(np.floor(hop * fs))
        self.step = None if step is None else int(step)
        if self.step is not None:
            vs.geometry(self.step)                                   # ValueError by name for a step outside the range
            self.n_model = self.n_frames
            self.n_frames = [vs.n_out(n, self.step) for n in self.n_model]
        counts = [n_segments(nfr, fs, duration, hop) for nfr in self.n_frames]
        self.file_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.n_samples = int(self.file_first[-1])

    def __len__(self):
        return (self.n_samples + self.bsz - 1) // self.bsz

    def _host_pcm(self, f):
        if self.step is not None:
            raise NotImplementedError(f'{self.fns[f]}: a speed change (step {self.step}) is undone on the device only (iter_windows + '
                                      'StreamedEmbedder.embed_windows); there is no CPU path')
        if self.resampled[f] and self.ingest:
            raise NotImplementedError(f'{self.fns[f]}: {self.rate[f]} Hz x {self.channels[f]} x {self.format[f]} is decoded and '
                                      'resampled on the device only (iter_windows + StreamedEmbedder.embed_windows); there is no '
                                      'CPU path')
        if self.resampled[f]:
            raise NotImplementedError(f'{self.fns[f]}: {self.rate[f]} Hz x {self.channels[f]} is resampled on the device only '
                                      '(iter_windows + StreamedEmbedder.embed_windows); there is no CPU resampler')
        return read_wav_int16(self.fns[f])

    def read_rows(self, row0, row1):
        """int16 (row1-row0, 1, seg_len) for global segment rows [row0, row1)."""
        out = np.zeros((row1 - row0, 1, self.seg_len), np.int16)
        f = int(np.searchsorted(self.file_first, row0, side='right') - 1)
        r = row0
        while r < row1:
            first, nxt = int(self.file_first[f]), int(self.file_first[f + 1])
            segs = file_segments(self._host_pcm(f), self.fs, self.duration, self.hop)
            a, b = r - first, min(row1, nxt) - first
            out[r - row0:r - row0 + (b - a), 0] = segs[a:b]
            r += b - a
            f += 1
        return out

    def __getitem__(self, i):
        if i < 0 or i >= len(self):
            raise IndexError(i)
        return self.read_rows(i * self.bsz, min((i + 1) * self.bsz, self.n_samples)), None

    def iter_rows(self, row0, row1, rows_per_chunk):
        """Yield (start_row, int16 chunk) over [row0, row1), each file read once."""
        cache_f, cache = -1, None
        r = row0
        while r < row1:
            end = min(r + rows_per_chunk, row1)
            out = np.zeros((end - r, 1, self.seg_len), np.int16)
            q = r
            while q < end:
                f = int(np.searchsorted(self.file_first, q, side='right') - 1)
                if f != cache_f:
                    cache = file_segments(self._host_pcm(f), self.fs, self.duration, self.hop)
                    cache_f = f
                first, nxt = int(self.file_first[f]), int(self.file_first[f + 1])
                a, b = q - first, min(end, nxt) - first
                out[q - r:q - r + (b - a), 0] = cache[a:b]
                q += b - a
            yield r, out
            r = end

    def iter_windows(self, row0, row1, rows_per_chunk, alloc=None):
        """Yield (start_row, n_rows, arena, used, seg_offset, seg_valid) -- with NAFP_RESAMPLE=1 (or a layer above it) a seventh
        item, the launch's device work (utils/ingest.ChunkPieces, the arena then holding the files' bytes as they are) or None
        for a launch of model-rate 16-bit mono files -- over rows [row0, row1):
        the PCM every row needs is read ONCE from each file (contiguous sample range, straight into
        `arena` = alloc(n_samples), e.g. pinned memory) and row i is the window
        arena[seg_offset[i] : seg_offset[i] + seg_len] with samples >= seg_valid[i] meaning zero --
        the same segments `iter_rows` materialises, without the 2x duplication of HOP = DUR/2.
        Under a step the launch is planned in the stretched domain and the seventh item is always there (varispeed.Stage): per
        piece the model-rate samples its stretched outputs read are planned exactly as the outputs of a launch without a step are,
        and the stage turns them into the stretched arena that seg_offset / seg_valid index, last on the launch's stream."""
        seg_len, hop_len = self.seg_len, self.hop_len
        r = row0
        while r < row1:
            end = min(r + rows_per_chunk, row1)
            n = end - r
            pieces, total, q = [], 0, r
            while q < end:
                f = int(np.searchsorted(self.file_first, q, side='right') - 1)
                first, nxt = int(self.file_first[f]), int(self.file_first[f + 1])
                a, b = q - first, min(end, nxt) - first
                s0 = a * hop_len
                s1 = max(s0, min((b - 1) * hop_len + seg_len, self.n_frames[f]))
                pieces.append((f, a, b, s0, s1, total, q - r))
                total += (s1 - s0 + 7) // 8 * 8                      # 16-B aligned piece starts
                q += b - a
            stretched, out_total = None, total
            if self.step is not None:
                # the pieces so far are stretched outputs; from here on `pieces` / `total` are the model-rate samples they read
                stretched, pieces, total = pieces, [], 0
                for f, a, b, s0, s1, base, o in stretched:
                    m0, m1 = vs.input_range(s0, s1, self.n_model[f], self.step) if s1 > s0 else (0, 0)
                    pieces.append((f, a, b, m0, m1, total, o))
                    total += (m1 - m0 + 7) // 8 * 8
                vs_rows = [(mp[5], mp[3], mp[4] - mp[3], self.n_model[sp[0]], sp[3], sp[5], sp[4] - sp[3], 0)
                           for sp, mp in zip(stretched, pieces)]
            if self.resample and any(self.resampled[p[0]] for p in pieces):
                # a launch that holds a file to convert: the arena holds the files' BYTES as they are (ingest.plan_span per piece),
                # seg_offset / seg_valid index the model-rate arena of `total` samples that the work fills on the device; files
                # the loaders would read straight go the same way in such a launch (the identity plan copies them)
                launch = ig.LaunchPlan(self.fs, self.flac_failed)
                for f, a, b, s0, s1, base, o in pieces:
                    launch.add(self.files[f], s0, s1, base)
                reads, used, work = launch.reads, launch.raw_bytes // 2, (launch.work(total),)
            else:
                reads = [(self.fns[f], self.data_offset[f] + 2 * s0, 2 * (s1 - s0), 2 * base) for f, a, b, s0, s1, base, o in pieces]
                used, work = total, ((None,) if self.resample else ())
            if stretched is not None:
                work = (vs.Stage(self.step, np.array(vs_rows, dtype=vs.PIECE_DTYPE), out_total, work[0] if work else None),)
                pieces = stretched
            arena = alloc(used) if alloc is not None else np.empty(max(used, 1), np.int16)
            raw = arena.view(np.uint8)
            for fn, file_off, n_bytes, at in reads:
                if n_bytes:
                    with open(fn, 'rb', buffering=0) as fh:
                        fh.seek(file_off)
                        if fh.readinto(memoryview(raw[at:at + n_bytes])) != n_bytes:
                            raise IOError(f'{fn}: short read')
            seg_offset = np.empty(n, np.int64)
            seg_valid = np.empty(n, np.int32)
            for f, a, b, s0, s1, base, o in pieces:
                k = np.arange(a, b, dtype=np.int64)
                seg_offset[o:o + (b - a)] = base + (k - a) * hop_len
                seg_valid[o:o + (b - a)] = np.clip(self.n_frames[f] - k * hop_len, 0, seg_len)
            yield (r, n, arena, used, seg_offset, seg_valid) + work
            r = end
