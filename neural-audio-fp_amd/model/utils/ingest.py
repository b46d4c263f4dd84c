"""Ingest of WAV files of any PCM / IEEE-float format, 1 to 8 channels, at any supported rate in either direction: host side
of `nafp_ingest_*` (include/nafp.h).

Opt-in: NAFP_INGEST_ANY=1.  It includes everything NAFP_RESAMPLE=1 does (utils/resample.py); setting both is the same as
setting it alone.  Without either every loader raises on anything but FS-rate 16-bit mono, as the reference does
(model/utils/audio_utils.py:160-169).  Decoding, down-mix and rate conversion exist on the device only (csrc/ingest.hip, exact
integer arithmetic): there is no CPU path, so whatever materialises samples on the host raises for such a file.
"""
import ctypes
import os

import numpy as np

from ... import _lib

PIECE_DTYPE = np.dtype(_lib.INGEST_PIECE_DTYPE)
FORMATS = _lib.INGEST_FORMATS                      # name -> (NAFP_INGEST_* code, bytes per sample)


def enabled():
    # NAFP_INGEST_CODECS=1 (utils/codecs.py) and NAFP_INGEST_FLAC=1 (utils/flac.py) include this switch
    return any(os.environ.get(k, '') == '1' for k in ('NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS', 'NAFP_INGEST_FLAC'))


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


class ChunkPieces:
    """The ingest work of one launch: raw arena (the files' bytes) -> `out_total` int16 at the model rate; `by_rate` maps fs_in
    to the host piece array of that rate (native files ride along through the identity plan).  With NAFP_INGEST_CODECS=1 a
    launch may hold codec files: `prepass` (utils/codecs.PrePass) then decodes their blocks from the raw arena into an int16
    scratch tensor first, on the same stream, and `by_rate_decoded` holds the pieces (format s16) that index that tensor's
    bytes.  With NAFP_INGEST_FLAC=1 it may hold FLAC files: `flac` = (utils/flac.PrePass, pieces by rate) is the same arrangement
    with a byte scratch tensor of its own, its pieces of format s16 or s24."""

    def __init__(self, fs_out, by_rate, out_total, prepass=None, by_rate_decoded=None, flac=None):
        self.fs_out, self.by_rate, self.out_total = fs_out, by_rate, int(out_total)
        self.prepass, self.by_rate_decoded = prepass, by_rate_decoded or {}
        self.flac = flac

    def run(self, raw_dev):
        """raw_dev: the uploaded arena, uint8 or an int16 tensor over the same bytes (the loaders' pinned buffers are int16)."""
        import torch
        raw = raw_dev if raw_dev.dtype == torch.uint8 else raw_dev.view(torch.uint8)
        out = torch.empty((max(self.out_total, 1),), dtype=torch.int16, device=raw.device)
        for fs_in, pieces in self.by_rate.items():
            plan_for(fs_in, self.fs_out, raw.device).run(raw, pieces, out)
        if self.prepass is not None:
            pcm = self.prepass.run(raw).view(torch.uint8)
            for fs_in, pieces in self.by_rate_decoded.items():
                plan_for(fs_in, self.fs_out, raw.device).run(pcm, pieces, out)
        if self.flac is not None:
            pcm = self.flac[0].run(raw)
            for fs_in, pieces in self.flac[1].items():
                plan_for(fs_in, self.fs_out, raw.device).run(pcm, pieces, out)
        return out


def rates_summary(source):
    """{'files': n, 'resampled': k, 'rates': {'48000x2xs24': count, ...}} of a SegmentSource / PcmStore: rate x channels x
    sample format per file class; 'resampled' counts the files that went through the device ingest."""
    rates = {}
    for r, c, f in zip(source.rate, source.channels, source.format):
        key = f'{r}x{c}x{f}'
        rates[key] = rates.get(key, 0) + 1
    return {'files': len(source.rate), 'resampled': int(sum(bool(x) for x in source.resampled)), 'rates': rates}
