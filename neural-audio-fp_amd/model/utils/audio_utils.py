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


def n_segments(n_frames, fs=8000, duration=1., hop=.5):
    """audio_utils.py:171-177."""
    n_seg_frames, n_hop_frames = fs * duration, fs * hop
    if n_frames > n_seg_frames:
        return int((n_frames - n_seg_frames + n_hop_frames) // n_hop_frames)
    return 1


def riff_scan(filename):
    """Header scan of a RIFF/WAVE file WITHOUT reading the samples: (fs, channels, sample width in
    bytes, byte offset of the first sample, frame count).  What `wave.open(...).getnframes()` reports
    (audio_utils.py:160-169), plus where the data chunk starts, so that a sample range can be read
    straight into a staging buffer."""
    size = os.path.getsize(filename)
    with open(filename, 'rb') as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b'RIFF' or head[8:12] != b'WAVE':
            raise ValueError(f'{filename}: not a RIFF/WAVE file')
        fmt = None
        while True:
            hdr = f.read(8)
            if len(hdr) < 8:
                raise ValueError(f'{filename}: no data chunk')
            cid, csz = hdr[:4], struct.unpack('<I', hdr[4:])[0]
            if cid == b'fmt ':
                body = f.read(csz + (csz & 1))
                tag, ch, rate, _, align, bits = struct.unpack('<HHIIHH', body[:16])
                fmt = (tag, ch, rate, align, bits)
            elif cid == b'data':
                if fmt is None:
                    raise ValueError(f'{filename}: data chunk before fmt chunk')
                off = f.tell()
                csz = min(csz, size - off)
                return fmt[2], fmt[1], fmt[4] // 8, off, csz // fmt[3]
            else:
                f.seek(csz + (csz & 1), 1)


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
    from . import codecs as cd
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
    size = os.path.getsize(filename)
    fact = None
    with open(filename, 'rb') as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b'RIFF' or head[8:12] != b'WAVE':
            raise ValueError(f'{filename}: not a RIFF/WAVE file')
        fmt = None
        while True:
            hdr = f.read(8)
            if len(hdr) < 8:
                raise ValueError(f'{filename}: no data chunk')
            cid, csz = hdr[:4], struct.unpack('<I', hdr[4:])[0]
            if cid == b'fmt ':
                fmt = f.read(csz + (csz & 1))[:csz]
                if len(fmt) < 16:
                    raise ValueError(f'{filename}: fmt chunk of {len(fmt)} bytes')
            elif cid == b'fact' and codecs:
                body = f.read(csz + (csz & 1))[:csz]
                if len(body) >= 4:
                    fact, = struct.unpack('<I', body[:4])
            elif cid == b'data':
                if fmt is None:
                    raise ValueError(f'{filename}: data chunk before fmt chunk')
                off = f.tell()
                csz = min(csz, size - off)
                break
            else:
                f.seek(csz + (csz & 1), 1)
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
            from . import ingest as ig
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
        from . import ingest as ig
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
    from . import flac as fl
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
        from . import ingest as ig
        ig.check_rate(rate, fs)
    total, indexed = int(info['total_samples']), int(info['indexed_samples'])
    return {'rate': rate, 'channels': ch, 'format': f'flac{bps}', 'width': 0, 'block_align': 0, 'offset': 0,
            'n_frames': total if 0 < total <= indexed else indexed, 'codec': 'flac', 'samples_per_block': 1, 'bps': bps,
            'frames': frames, 'index': fl.Index(frames, ch, bps, rate)}


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


def _resample_on():
    return os.environ.get('NAFP_RESAMPLE', '') == '1'


def _flac_on():
    return os.environ.get('NAFP_INGEST_FLAC', '') == '1'


def _codecs_on():
    return os.environ.get('NAFP_INGEST_CODECS', '') == '1' or _flac_on()           # NAFP_INGEST_FLAC=1 includes it


def _taken_name(fn, flac):
    """The loaders' name check: `wav`, and under NAFP_INGEST_FLAC=1 `.flac` in any letter case."""
    return fn[-3:] == 'wav' or (flac and fn[-5:].lower() == '.flac')


def _ingest_on():
    return os.environ.get('NAFP_INGEST_ANY', '') == '1' or _codecs_on()          # NAFP_INGEST_CODECS=1 includes it


class SegmentSource:
    """Ordered segments of a list of WAV files, served in consecutive batches.

    Counterpart of `genUnbalSequence(fns, bsz, n_anchor=bsz, shuffle=False,
    drop_the_last_non_full_batch=False)` as the generate path uses it
    (model/dataset.py:204-215): `.n_samples` segments, `len()` batches of `bsz`
    (the last one ragged), item i = segments [i*bsz, (i+1)*bsz) as int16 (n,1,T).
    """

    def __init__(self, fns_list, bsz, duration=1., hop=.5, fs=8000):
        self.fns, self.bsz, self.duration, self.hop, self.fs = list(fns_list), int(bsz), duration, hop, fs
        self.seg_len = int(fs * duration)
        self.hop_len = int(np.floor(hop * fs))
        self.n_frames, self.data_offset = [], []
        # NAFP_RESAMPLE=1: files at other rates / in stereo are taken too and resampled on the device (utils/resample.py);
        # n_frames is then the length at the model rate, n_in / rate / channels describe the file itself
        # NAFP_INGEST_ANY=1 (includes the above): any PCM / float format, 1 to 8 channels, rates in either direction
        # (utils/ingest.py); `format` / `block_align` then describe the file's samples, and the raw arena of a launch holds BYTES
        # NAFP_INGEST_CODECS=1 (includes both): A-law, mu-law, IMA and MS ADPCM too (utils/codecs.py); `spb` is then the frames per
        # block_align bytes (1 for PCM / float), n_in the file's frame count, and a launch decodes whole blocks in a pre-pass
        # NAFP_INGEST_FLAC=1 (includes all three): `.flac` names too (utils/flac.py); `flac_index[f]` is then the file's frame index,
        # built here by one pass over the file, and a launch decodes the whole frames that cover its samples in a pre-pass
        self.flac = _flac_on()
        self.flac_index = {}
        self.codecs = _codecs_on()
        self.ingest = _ingest_on()
        self.resample = _resample_on() or self.ingest
        self.rate, self.channels, self.n_in, self.resampled = [], [], [], []
        self.format, self.block_align, self.spb = [], [], []
        for fn in self.fns:                      # ONE header scan per file (the reference re-opens per segment)
            if not _taken_name(fn, self.flac):
                raise NotImplementedError(fn[-3:])
            if self.ingest:
                from . import ingest as ig
                if fn[-3:] != 'wav':
                    info = flac_scan(fn, fs)
                    self.flac_index[len(self.n_frames)] = info['index']
                else:
                    info = riff_scan_ex(fn, fs, codecs=True) if self.codecs else riff_scan_ex(fn, fs)
                rate, ch, off, nfr = info['rate'], info['channels'], info['offset'], info['n_frames']
                native = ig.is_native(info, fs)
                n_model = nfr if native else ig.n_out(nfr, rate, fs)
                self.format.append(info['format']); self.block_align.append(info['block_align'])
                self.spb.append(info.get('samples_per_block', 1))
                self.n_frames.append(n_model); self.data_offset.append(off)
                self.rate.append(rate); self.channels.append(ch); self.n_in.append(nfr); self.resampled.append(not native)
                continue
            rate, ch, width, off, nfr = riff_scan(fn)
            if self.resample:
                from . import resample as rs
                rs.check_file(fn, rate, ch, width, fs)
                native = rate == fs and ch == 1
                n_model = nfr if native else rs.n_out(nfr, rate, fs)
            else:
                if rate != fs:
                    raise ValueError('Sample rate should be {} but got {}'.format(str(fs), str(rate)))
                if width != 2 or ch != 1:
                    raise ValueError(f'{fn}: expected 16-bit mono PCM')
                native, n_model = True, nfr
            self.n_frames.append(n_model); self.data_offset.append(off)
            self.rate.append(rate); self.channels.append(ch); self.n_in.append(nfr); self.resampled.append(not native)
        self.flac_failed = None
        if self.flac_index:                      # which frames failed their checks: one byte per frame, on the device
            from . import flac as fl
            self.flac_failed = fl.FailedFrames([len(self.flac_index[f]) if f in self.flac_index else 0 for f in range(len(self.fns))])
        counts = [n_segments(nfr, fs, duration, hop) for nfr in self.n_frames]
        self.file_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.n_samples = int(self.file_first[-1])

    def __len__(self):
        return (self.n_samples + self.bsz - 1) // self.bsz

    def _host_pcm(self, f):
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
        """Yield (start_row, n_rows, arena, used, seg_offset, seg_valid) -- with NAFP_RESAMPLE=1 a seventh item, the launch's
        resampling work (utils/resample.ChunkPieces; with NAFP_INGEST_ANY=1 utils/ingest.ChunkPieces, the arena then holding the
        files' bytes) or None for a launch of model-rate mono files -- over rows [row0, row1):
        the PCM every row needs is read ONCE from each file (contiguous sample range, straight into
        `arena` = alloc(n_samples), e.g. pinned memory) and row i is the window
        arena[seg_offset[i] : seg_offset[i] + seg_len] with samples >= seg_valid[i] meaning zero --
        the same segments `iter_rows` materialises, without the 2x duplication of HOP = DUR/2."""
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
            if self.resample and any(self.resampled[p[0]] for p in pieces):
                chunk = self._ingest_chunk if self.ingest else self._resample_chunk
                yield (r, n) + chunk(pieces, n, total, alloc)
                r = end
                continue
            arena = alloc(total) if alloc is not None else np.empty(max(total, 1), np.int16)
            seg_offset = np.empty(n, np.int64)
            seg_valid = np.empty(n, np.int32)
            for f, a, b, s0, s1, base, o in pieces:
                if s1 > s0:
                    with open(self.fns[f], 'rb', buffering=0) as fh:
                        fh.seek(self.data_offset[f] + 2 * s0)
                        dst = memoryview(arena[base:base + (s1 - s0)]).cast('B')
                        got = fh.readinto(dst)
                        if got != 2 * (s1 - s0):
                            raise IOError(f'{self.fns[f]}: short read')
                k = np.arange(a, b, dtype=np.int64)
                seg_offset[o:o + (b - a)] = base + (k - a) * hop_len
                seg_valid[o:o + (b - a)] = np.clip(self.n_frames[f] - k * hop_len, 0, seg_len)
            if self.resample:
                yield r, n, arena, total, seg_offset, seg_valid, None
            else:
                yield r, n, arena, total, seg_offset, seg_valid
            r = end

    def _resample_chunk(self, pieces, n, total, alloc):
        """A launch that holds a file to resample: (raw arena, used, seg_offset, seg_valid, ChunkPieces).  `arena` then holds the
        RAW frames every piece's outputs read (nafp_resample_input_range; interleaved for stereo; 16-B aligned piece starts) and
        seg_offset / seg_valid index the model-rate arena of `total` samples that ChunkPieces.run fills on the device.  Files
        at the model rate in mono go the same way in such a launch (the identity plan copies them)."""
        from . import resample as rs
        seg_len, hop_len = self.seg_len, self.hop_len
        raw_total, spans = 0, []
        for f, a, b, s0, s1, base, o in pieces:
            first, last = rs.input_range(s0, s1, self.n_in[f], self.rate[f], self.fs) if s1 > s0 else (0, 0)
            spans.append((first, last, raw_total))
            raw_total += ((last - first) * self.channels[f] + 7) // 8 * 8
        arena = alloc(raw_total) if alloc is not None else np.empty(max(raw_total, 1), np.int16)
        seg_offset = np.empty(n, np.int64)
        seg_valid = np.empty(n, np.int32)
        by_rate = {}
        for (f, a, b, s0, s1, base, o), (first, last, raw_base) in zip(pieces, spans):
            ch = self.channels[f]
            if last > first:
                with open(self.fns[f], 'rb', buffering=0) as fh:
                    fh.seek(self.data_offset[f] + 2 * ch * first)
                    dst = memoryview(arena[raw_base:raw_base + (last - first) * ch]).cast('B')
                    if fh.readinto(dst) != 2 * ch * (last - first):
                        raise IOError(f'{self.fns[f]}: short read')
            by_rate.setdefault(self.rate[f], []).append((raw_base, first, last - first, self.n_in[f], s0, base, s1 - s0, ch))
            k = np.arange(a, b, dtype=np.int64)
            seg_offset[o:o + (b - a)] = base + (k - a) * hop_len
            seg_valid[o:o + (b - a)] = np.clip(self.n_frames[f] - k * hop_len, 0, seg_len)
        by_rate = {rate: np.array(rows, dtype=rs.PIECE_DTYPE) for rate, rows in by_rate.items()}
        return arena, raw_total, seg_offset, seg_valid, rs.ChunkPieces(self.fs, by_rate, total)

    def _ingest_chunk(self, pieces, n, total, alloc):
        """`_resample_chunk` for NAFP_INGEST_ANY=1: (raw arena, used, seg_offset, seg_valid, ingest.ChunkPieces).  `arena` (int16
        units, as `alloc` hands it out; `used` counts them) holds the files' BYTES: for every piece the byte range
        nafp_ingest_input_range x block_align, read as the file has it, piece starts 16-B aligned.  seg_offset / seg_valid index
        the model-rate arena of `total` samples, unchanged.  Native files go the same way in such a launch (identity plan).
        A codec file (NAFP_INGEST_CODECS=1) uploads the WHOLE BLOCKS that cover its frame range; the launch's pre-pass
        (codecs.PrePass) decodes them into an int16 scratch tensor and the file's ingest piece indexes that tensor as 16-bit PCM.
        A FLAC file (NAFP_INGEST_FLAC=1) uploads the WHOLE FRAMES that cover its sample range, one contiguous byte range of the
        file; flac.PrePass decodes them into a byte scratch tensor of its own, indexed as 16- or 24-bit PCM."""
        from . import ingest as ig
        from . import codecs as cd
        from . import flac as fl
        seg_len, hop_len = self.seg_len, self.hop_len
        raw_bytes, spans = 0, []
        for f, a, b, s0, s1, base, o in pieces:
            first, last = ig.input_range(s0, s1, self.n_in[f], self.rate[f], self.fs) if s1 > s0 else (0, 0)
            if f in self.flac_index:                 # samples -> the frames that hold them; their bytes
                first, last = fl.frame_range(self.flac_index[f], first, last)
                spans.append((first, last, raw_bytes))
                raw_bytes += (fl.records(self.flac_index[f], first, last, 0, 0)[1] + 15) // 16 * 16
                continue
            if self.format[f] in cd.CODECS:          # frames -> the blocks that hold them
                first, last = cd.block_range(first, last, self.spb[f])
            spans.append((first, last, raw_bytes))
            raw_bytes += ((last - first) * self.block_align[f] + 15) // 16 * 16
        used = raw_bytes // 2
        arena = alloc(used) if alloc is not None else np.empty(max(used, 1), np.int16)
        raw = arena.view(np.uint8)
        seg_offset = np.empty(n, np.int64)
        seg_valid = np.empty(n, np.int32)
        by_rate, by_rate_decoded, codec_rows, scratch = {}, {}, [], 0
        by_rate_flac, flac_rows, flac_ids, flac_scratch = {}, [], [], 0
        for (f, a, b, s0, s1, base, o), (first, last, raw_base) in zip(pieces, spans):
            align = self.block_align[f]
            if f in self.flac_index:
                idx = self.flac_index[f]
                rows, n_raw, n_pcm = fl.records(idx, first, last, raw_base, flac_scratch)
                if n_raw:
                    with open(self.fns[f], 'rb', buffering=0) as fh:
                        fh.seek(int(idx.offset[first]))
                        if fh.readinto(memoryview(raw[raw_base:raw_base + n_raw])) != n_raw:
                            raise IOError(f'{self.fns[f]}: short read')
                    flac_rows.append(rows)
                    flac_ids.append(self.flac_failed.base[f] + np.arange(first, last, dtype=np.int64))
                frame0 = int(idx.start[first]) if last > first else 0
                covered = int(idx.start[last] - idx.start[first]) if last > first else 0
                by_rate_flac.setdefault(self.rate[f], []).append(
                    (flac_scratch, frame0, max(0, min(covered, self.n_in[f] - frame0)), self.n_in[f], s0, base, s1 - s0, self.channels[f],
                     ig.FORMATS['s16' if idx.bps <= 16 else 's24'][0], 0))
                flac_scratch += (n_pcm + 15) // 16 * 16
            elif last > first:
                with open(self.fns[f], 'rb', buffering=0) as fh:
                    fh.seek(self.data_offset[f] + align * first)
                    if fh.readinto(memoryview(raw[raw_base:raw_base + (last - first) * align])) != align * (last - first):
                        raise IOError(f'{self.fns[f]}: short read')
            if f in self.flac_index:
                pass
            elif self.format[f] in cd.CODECS:
                spb, ch = self.spb[f], self.channels[f]
                codec_rows.append((raw_base, last - first, scratch, cd.CODECS[self.format[f]], ch, align, spb))
                by_rate_decoded.setdefault(self.rate[f], []).append(
                    (2 * scratch, first * spb, min((last - first) * spb, self.n_in[f] - first * spb), self.n_in[f], s0, base, s1 - s0,
                     ch, ig.FORMATS['s16'][0], 0))
                scratch += ((last - first) * spb * ch + 7) // 8 * 8
            else:
                by_rate.setdefault(self.rate[f], []).append((raw_base, first, last - first, self.n_in[f], s0, base, s1 - s0,
                                                             self.channels[f], ig.FORMATS[self.format[f]][0], 0))
            k = np.arange(a, b, dtype=np.int64)
            seg_offset[o:o + (b - a)] = base + (k - a) * hop_len
            seg_valid[o:o + (b - a)] = np.clip(self.n_frames[f] - k * hop_len, 0, seg_len)
        by_rate = {rate: np.array(rows, dtype=ig.PIECE_DTYPE) for rate, rows in by_rate.items()}
        flac = None
        if by_rate_flac:
            by_rate_flac = {rate: np.array(rows, dtype=ig.PIECE_DTYPE) for rate, rows in by_rate_flac.items()}
            frames = np.concatenate(flac_rows) if flac_rows else np.zeros(0, fl.FRAME_DTYPE)
            ids = np.concatenate(flac_ids) if flac_ids else np.zeros(0, np.int64)
            flac = (fl.PrePass(frames, flac_scratch, self.flac_failed, ids), by_rate_flac)
        if not codec_rows:
            return arena, used, seg_offset, seg_valid, ig.ChunkPieces(self.fs, by_rate, total, flac=flac)
        by_rate_decoded = {rate: np.array(rows, dtype=ig.PIECE_DTYPE) for rate, rows in by_rate_decoded.items()}
        prepass = cd.PrePass(np.array(codec_rows, dtype=cd.PIECE_DTYPE), scratch)
        return arena, used, seg_offset, seg_valid, ig.ChunkPieces(self.fs, by_rate, total, prepass, by_rate_decoded, flac=flac)
