"""Ingest of WAV files of any PCM / IEEE-float format, 1 to 8 channels, at any supported rate in either direction: host side
of `nafp_ingest_*` (include/nafp.h).

Opt-in: NAFP_INGEST_ANY=1 (the layers: utils/resample.switches).  Without any of them every loader raises on anything but FS-rate
16-bit mono, as the reference does (model/utils/audio_utils.py:160-169).  Decoding, down-mix and rate conversion exist on the
device only (csrc/ingest.hip, exact integer arithmetic): there is no CPU path, so whatever materialises samples on the host raises
for such a file.

This module also holds the one rule both loaders share for every layer (`plan_span`): which bytes of a file cover a range of its
frames, what pre-pass records decode them and which piece reads the result -- and on top of it the plan of a launch of many
files (`LaunchPlan`, for SegmentSource) and of one file in runs through a staging buffer (`file_runs`, for PcmArena).
"""
import collections
import ctypes
import functools
import sys
import types

import numpy as np

from ... import _lib
from . import codecs as cd
from . import flac as fl
from . import resample as rs

PIECE_DTYPE = np.dtype(_lib.INGEST_PIECE_DTYPE)
FORMATS = _lib.INGEST_FORMATS                      # name -> (NAFP_INGEST_* code, bytes per sample)


def enabled():
    return rs.switches().ingest


def geometry(fs_in, fs_out):
    """(L, M, half, T); ValueError for a pair of rates the ingest does not take."""
    v = [ctypes.c_int() for _ in range(4)]
    st = _lib.load().nafp_ingest_geometry(int(fs_in), int(fs_out), *[ctypes.byref(x) for x in v])
    if st != 0:
        raise ValueError(f'cannot convert {fs_in} Hz to {fs_out} Hz (supported: both rates up to 192000 Hz and a reduced ratio '
                         f'fs_out / fs_in whose numerator is <= 640, e.g. 4000 ... 192000 -> 8000, 8000 / 11025 -> 16000)')
    return tuple(x.value for x in v)


def n_out(n_in, fs_in, fs_out):
    n = int(_lib.load().nafp_ingest_n_out(int(n_in), int(fs_in), int(fs_out)))
    if n < 0:
        raise ValueError(f'cannot convert {fs_in} Hz to {fs_out} Hz')
    return n


def input_range(n0, n1, n_in, fs_in, fs_out):
    """Frames [first, last) of the file that the outputs [n0, n1) read."""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.load().nafp_ingest_input_range(int(n0), int(n1), int(n_in), int(fs_in), int(fs_out), ctypes.byref(a),
                                                   ctypes.byref(b)), 'ingest_input_range')
    return a.value, b.value


def check_rate(rate, fs):
    """The reference's wording for a rate that cannot be brought to the model rate."""
    if rate != fs:
        try:
            geometry(rate, fs)
        except ValueError:
            raise ValueError('Sample rate should be {} but got {}'.format(str(fs), str(rate)))


def is_native(info, fs):
    """A file the loaders read straight into the int16 arena: 16-bit PCM mono at the model rate (never a codec file)."""
    return info['rate'] == fs and info['channels'] == 1 and info['format'] == 's16' and not info.get('codec')


def check_pieces(fs_in, fs_out, pieces, raw_size, out_samples):
    """The kernel's own per-piece checks on the host-built list, before anything is uploaded."""
    pieces = np.ascontiguousarray(pieces, dtype=PIECE_DTYPE)
    _lib.check(_lib.load().nafp_ingest_check_pieces_host(int(fs_in), int(fs_out), pieces.ctypes.data_as(ctypes.c_void_p),
                                                         len(pieces), int(raw_size), int(out_samples)), 'ingest pieces')
    return pieces


class Plan:
    """nafp_ingest plan of one (fs_in, fs_out): owns the device table."""

    def __init__(self, fs_in, fs_out):
        self.fs_in, self.fs_out = int(fs_in), int(fs_out)
        self.L, self.M, self.half, self.T = geometry(fs_in, fs_out)
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(self._lib.nafp_ingest_create(ctypes.byref(h), self.fs_in, self.fs_out), 'ingest_create')
        self.handle = h

    def __del__(self):
        if getattr(self, 'handle', None):
            self._lib.nafp_ingest_destroy(self.handle)
            self.handle = None

    def run(self, raw, pieces, out, pieces_dev=None):
        """raw: uint8 CUDA tensor (the files' bytes); out: int16 CUDA tensor; pieces: host array of PIECE_DTYPE (checked here,
        uploaded unless `pieces_dev`, a CUDA uint8 tensor holding the same bytes, is given).  Enqueued on the current stream."""
        import torch
        _lib.require_cuda(raw, 'raw'); _lib.require_cuda(out, 'out')
        if raw.dtype != torch.uint8 or out.dtype != torch.int16:
            raise TypeError('ingest: a uint8 raw arena and an int16 output arena expected')
        pieces = check_pieces(self.fs_in, self.fs_out, pieces, raw.numel(), out.numel())
        if len(pieces) == 0:
            return out
        if pieces_dev is None:
            pieces_dev = torch.from_numpy(pieces.view(np.uint8).reshape(-1)).to(raw.device)
        with torch.cuda.device(raw.device):
            _lib.check(self._lib.nafp_ingest_i16(self.handle, _lib.ptr(raw), raw.numel(), _lib.ptr(pieces_dev), len(pieces),
                                                 _lib.ptr(out), out.numel(), _lib.current_stream()), 'ingest_i16')
        return out


_PLANS = {}


def plan_for(fs_in, fs_out, device=None):
    """Small cache of plans per (rate, model rate, device)."""
    import torch
    dev = torch.cuda.current_device() if device is None else torch.device(device).index or 0
    key = (int(fs_in), int(fs_out), dev)
    if key not in _PLANS:
        with torch.cuda.device(dev):
            _PLANS[key] = Plan(fs_in, fs_out)
    return _PLANS[key]


def as_raw(t):
    """The uploaded arena as this kernel takes it: uint8, or the bytes of an int16 tensor (the loaders' pinned buffers are int16)."""
    import torch
    return t if t.dtype == torch.uint8 else t.view(torch.uint8)


rates_summary = functools.partial(rs.rates_summary, formats=True)


# ---- what a file's frames need: the rule shared by every layer and both loaders --------------------------------------------
FileEntry = collections.namedtuple('FileEntry', 'fn kind rate channels n_in n_frames resampled data_offset format block_align spb '
                                                'flac frame_base')
FileEntry.__doc__ = """One file of a loader's catalog (audio_utils.FileCatalog).  kind: 'pcm16' (the 16-bit layer of NAFP_RESAMPLE=1 and
the switch-less loaders: nafp_resample_* pieces), 'pcm' (any PCM / float format), 'codec' (block codec) or 'flac'.  rate / channels /
n_in describe the file, n_frames is its length at the model rate, `resampled` whether the device converts it.  data_offset: the
first sample's byte; format / block_align: the file's samples; spb: frames per block_align bytes (1 unless a codec); flac: the
file's frame index (flac.Index) or None; frame_base: its first frame's place in the source's flac.FailedFrames."""

STAGE_OF = {'pcm16': 0, 'pcm': 0, 'codec': 1, 'flac': 2}       # the order a launch's stages run in: direct, codec blocks, FLAC frames
Stage = collections.namedtuple('Stage', 'prepass by_rate')
Span = collections.namedtuple('Span', 'units file_off n_bytes records scratch ids raw_off frame0 n_frames format')


def family(e):
    """The module whose kernel converts the file: geometry, input_range, plan_for, PIECE_DTYPE and as_raw of its pieces."""
    return rs if e.kind == 'pcm16' else sys.modules[__name__]


def plan_span(e, first, last, raw_base=0, scratch_base=0):
    """What the input frames [first, last) of file `e` need, when their bytes go to `raw_base` (bytes) of a raw arena and what a
    pre-pass decodes of them to `scratch_base` (bytes) of its scratch tensor:
      units             the frames (PCM / float), whole blocks (codec) or whole FLAC frames covered, half-open
      file_off, n_bytes the one byte range of the file to read
      records, scratch  the pre-pass records (codecs.PIECE_DTYPE / flac.FRAME_DTYPE; None: read directly) and the bytes they produce
      ids               a FLAC file: its frames' places in the source's FailedFrames
      raw_off, frame0, n_frames, format   of the piece that reads the result: where (the raw arena, in the kernel's units, or the
                        scratch tensor, in bytes), the first frame held there, how many, and as which sample format."""
    if e.kind == 'flac':                             # samples -> the frames that hold them; s16 containers up to 16 bits, s24 above
        k0, k1 = fl.frame_range(e.flac, first, last)
        rows, n_raw, n_pcm = fl.records(e.flac, k0, k1, raw_base, scratch_base)
        frame0 = int(e.flac.start[k0]) if k1 > k0 else 0
        covered = int(e.flac.start[k1] - e.flac.start[k0]) if k1 > k0 else 0
        return Span((k0, k1), int(e.flac.offset[k0]) if n_raw else 0, n_raw, rows, n_pcm, e.frame_base + np.arange(k0, k1, dtype=np.int64),
                    scratch_base, frame0, max(0, min(covered, e.n_in - frame0)), FORMATS['s16' if e.flac.bps <= 16 else 's24'][0])
    if e.kind == 'codec':                            # frames -> the blocks that hold them, decoded to interleaved 16-bit PCM
        b0, b1 = cd.block_range(first, last, e.spb)
        rows = np.array([(raw_base, b1 - b0, scratch_base // 2, cd.CODECS[e.format], e.channels, e.block_align, e.spb)], dtype=cd.PIECE_DTYPE)
        return Span((b0, b1), e.data_offset + e.block_align * b0, (b1 - b0) * e.block_align, rows, 2 * (b1 - b0) * e.spb * e.channels, None,
                    scratch_base, b0 * e.spb, min((b1 - b0) * e.spb, e.n_in - b0 * e.spb), FORMATS['s16'][0])
    unit = 2 if e.kind == 'pcm16' else 1             # the 16-bit layer's pieces count the raw arena in int16
    return Span((first, last), e.data_offset + e.block_align * first, (last - first) * e.block_align, None, 0, None,
                raw_base // unit, first, last - first, FORMATS[e.format][0])


def piece_row(e, span, out0, out_off, n_out):
    """The piece that turns `span` into the outputs [out0, out0 + n_out) of the file, written at out_off of the model-rate arena."""
    row = (span.raw_off, span.frame0, span.n_frames, e.n_in, out0, out_off, n_out, e.channels)
    return row if e.kind == 'pcm16' else row + (span.format, 0)


class LaunchPlan:
    """The device work of one launch, built file piece by file piece (`add`): the layout of the raw arena (`reads`: file, byte
    offset, byte count, place in the arena; piece starts 16-byte aligned; `raw_bytes` in all), and per stage the pre-pass records,
    the layout of its scratch tensor (16-byte aligned too) and the pieces by rate.  `work` wraps it up as ChunkPieces."""

    def __init__(self, fs_out, failed=None):
        self.fs_out, self.failed, self.family = fs_out, failed, None
        self.raw_bytes, self.reads = 0, []
        self._stages = {0: types.SimpleNamespace(scratch=0, records=[], ids=[], by_rate={})}

    def add(self, e, out0, out1, out_off):
        """Outputs [out0, out1) of file `e`, to out_off of the model-rate arena."""
        self.family = family(e)
        first, last = self.family.input_range(out0, out1, e.n_in, e.rate, self.fs_out) if out1 > out0 else (0, 0)
        st = self._stages.setdefault(STAGE_OF[e.kind], types.SimpleNamespace(scratch=0, records=[], ids=[], by_rate={}))
        span = plan_span(e, first, last, self.raw_bytes, st.scratch)
        self.reads.append((e.fn, span.file_off, span.n_bytes, self.raw_bytes))
        self.raw_bytes += (span.n_bytes + 15) // 16 * 16
        st.scratch += (span.scratch + 15) // 16 * 16
        if span.records is not None:
            st.records.append(span.records)
        if span.ids is not None:
            st.ids.append(span.ids)
        st.by_rate.setdefault(e.rate, []).append(piece_row(e, span, out0, out_off, out1 - out0))
        return span

    def work(self, out_total):
        stages = []
        for k, st in sorted(self._stages.items()):
            prepass = None
            if k == 1:
                prepass = cd.PrePass(np.concatenate(st.records), st.scratch // 2)
            elif k == 2:
                prepass = fl.PrePass(np.concatenate(st.records), st.scratch, self.failed, np.concatenate(st.ids))
            stages.append(Stage(prepass, {rate: np.array(rows, dtype=self.family.PIECE_DTYPE) for rate, rows in st.by_rate.items()}))
        return ChunkPieces(self.fs_out, stages, out_total, self.family)


def _room(e, stage_bytes):
    """Input frames whose bytes fit a staging buffer of stage_bytes.  A codec file's span is rounded out to whole blocks: two more;
    a FLAC file's to whole frames, taken at the file's mean bytes per sample with the largest frame counted twice."""
    if e.kind == 'flac':
        per_sample = max(1., float(e.flac.n_bytes.sum()) / max(int(e.flac.start[-1]), 1))
        return int((stage_bytes - 2 * int(e.flac.n_bytes.max())) / (2 * per_sample)) - 2 * int(e.flac.block.max())
    return (stage_bytes // e.block_align - (2 if e.kind == 'codec' else 0)) * e.spb


def file_runs(e, fs_out, out_off, stage_bytes, failed=None):
    """File `e` -> [out_off, out_off + n_frames) of the model-rate arena through a staging buffer of stage_bytes, in runs of
    outputs: yields (n0, n1, LaunchPlan of that one piece) per run, whose bytes fit the buffer.  Host only."""
    L, M, half, _ = family(e).geometry(e.rate, fs_out)
    # outputs per run: their input span (n M / L frames + the filter's two half-widths) fits the staging buffer
    room = _room(e, stage_bytes) - 2 * (half // L + 2)
    if room * L < M:
        what = {'pcm16': 'resample', 'flac': 'convert FLAC'}.get(e.kind, 'convert')
        raise NotImplementedError(f'{e.fn}: staging buffer too small to {what} from {e.rate} Hz')
    step = max(1, min(room * L // M, (1 << 31) - 1))
    n0 = 0
    while n0 < e.n_frames:
        n1 = min(e.n_frames, n0 + step)
        run = LaunchPlan(fs_out, failed)
        run.add(e, n0, n1, out_off + n0)
        if run.reads[0][2] > stage_bytes:                # FLAC frames denser than the file's mean (nothing else can): halve the run
            if n1 - n0 <= 1:
                raise NotImplementedError(f'{e.fn}: staging buffer too small for its FLAC frames')
            step = max(1, (n1 - n0) // 2)
            continue
        yield n0, n1, run
        n0 = n1


class ChunkPieces:
    """The device work of one launch: raw arena (the files' bytes) -> `out_total` int16 at the model rate.  `stages`, in run order:
    Stage(prepass, by_rate) -- an optional pre-pass (codecs.PrePass, flac.PrePass) that decodes part of the raw arena into a
    scratch tensor of its own, on the same stream, and per fs_in the host piece array that reads the raw arena (no pre-pass) or that
    tensor.  Stage 0 is the direct one (`by_rate`; native files ride along there through the identity plan).  `family`: this
    module, or utils/resample for a launch of the 16-bit layer."""

    def __init__(self, fs_out, stages, out_total, family=None):
        self.fs_out, self.stages, self.out_total = fs_out, list(stages), int(out_total)
        self.family = family or sys.modules[__name__]

    @property
    def by_rate(self):
        return self.stages[0].by_rate

    def run(self, raw_dev, out=None):
        """raw_dev: the uploaded arena (uint8 or int16 over the same bytes).  out: the int16 arena to fill (default: a new one)."""
        import torch
        raw = self.family.as_raw(raw_dev)
        if out is None:
            out = torch.empty((max(self.out_total, 1),), dtype=torch.int16, device=raw.device)
        for prepass, by_rate in self.stages:
            src = raw if prepass is None else self.family.as_raw(prepass.run(raw))
            for fs_in, pieces in by_rate.items():
                self.family.plan_for(fs_in, self.fs_out, raw.device).run(src, pieces, out)
        return out
