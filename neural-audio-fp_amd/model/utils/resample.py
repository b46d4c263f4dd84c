"""Ingest of WAV files at other sample rates / in stereo: host side of `nafp_resample_*` (include/nafp.h).

Opt-in: NAFP_RESAMPLE=1.  Without it every loader raises on anything but FS-rate mono, as the reference does
(model/utils/audio_utils.py:160-169).  The conversion itself exists on the device only (csrc/resample.hip, exact integer
arithmetic): there is no CPU resampler here, so whatever materialises samples on the host raises for such a file.
"""
import collections
import ctypes
import os

import numpy as np

from ... import _lib

PIECE_DTYPE = np.dtype(_lib.RESAMPLE_PIECE_DTYPE)

Switches = collections.namedtuple('Switches', 'resample ingest codecs flac aiff resample_itself')


def switches():
    """The opt-in layers of audio ingest as the environment sets them, the one place that reads it.  Each layer includes the
    ones before it, so setting one together with an earlier one is the same as setting it alone:
      resample  NAFP_RESAMPLE=1       16-bit PCM in mono or stereo at a higher rate; its own kernel (nafp_resample_*, this module)
      ingest    NAFP_INGEST_ANY=1     any PCM / float format, 1 to 8 channels, rates in either direction (utils/ingest.py)
      codecs    NAFP_INGEST_CODECS=1  A-law, mu-law, IMA and MS ADPCM too, decoded by a pre-pass of whole blocks (utils/codecs.py)
      flac      NAFP_INGEST_FLAC=1    `.flac` names too, decoded by a pre-pass of whole frames (utils/flac.py)
      aiff      NAFP_INGEST_AIFF=1    `.aif` / `.aiff` / `.aifc` / `.au` / `.snd` names too: big-endian and signed 8-bit samples read
                                      by the ingest itself, Apple IMA4 packets by the codec pre-pass (audio_utils.aiff_scan, au_scan)
    `resample_itself`: NAFP_RESAMPLE=1 is set, whatever else is."""
    on = [os.environ.get(k, '') == '1' for k in ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS', 'NAFP_INGEST_FLAC',
                                                 'NAFP_INGEST_AIFF')]
    return Switches(any(on), any(on[1:]), any(on[2:]), any(on[3:]), on[4], on[0])


def enabled():
    return switches().resample_itself


def geometry(fs_in, fs_out):
    """(L, M, half, T); ValueError for a ratio the resampler does not take."""
    v = [ctypes.c_int() for _ in range(4)]
    st = _lib.load().nafp_resample_geometry(int(fs_in), int(fs_out), *[ctypes.byref(x) for x in v])
    if st != 0:
        raise ValueError(f'cannot resample {fs_in} Hz to {fs_out} Hz (supported: a higher rate up to 192000 Hz whose reduced '
                         f'ratio has a numerator <= 320, e.g. 11025 ... 192000 -> 8000)')
    return tuple(x.value for x in v)


def n_out(n_in, fs_in, fs_out):
    n = int(_lib.load().nafp_resample_n_out(int(n_in), int(fs_in), int(fs_out)))
    if n < 0:
        raise ValueError(f'cannot resample {fs_in} Hz to {fs_out} Hz')
    return n


def input_range(n0, n1, n_in, fs_in, fs_out):
    """Frames [first, last) of the file that the outputs [n0, n1) read."""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.load().nafp_resample_input_range(int(n0), int(n1), int(n_in), int(fs_in), int(fs_out), ctypes.byref(a),
                                                     ctypes.byref(b)), 'resample_input_range')
    return a.value, b.value


def check_file(fn, rate, channels, width, fs):
    """What a loader accepts with the switch on; raises as without it for everything else."""
    if width != 2 or channels not in (1, 2):
        raise ValueError(f'{fn}: expected 16-bit PCM with 1 or 2 channels')
    if rate != fs:
        try:
            geometry(rate, fs)
        except ValueError:
            raise ValueError('Sample rate should be {} but got {}'.format(str(fs), str(rate)))


def check_pieces(fs_in, fs_out, pieces, raw_samples, out_samples):
    """The kernel's own per-piece checks on the host-built list, before anything is uploaded."""
    pieces = np.ascontiguousarray(pieces, dtype=PIECE_DTYPE)
    _lib.check(_lib.load().nafp_resample_check_pieces_host(int(fs_in), int(fs_out), pieces.ctypes.data_as(ctypes.c_void_p),
                                                           len(pieces), int(raw_samples), int(out_samples)), 'resample pieces')
    return pieces


class Plan:
    """nafp_resample plan of one (fs_in, fs_out): owns the device table."""

    def __init__(self, fs_in, fs_out):
        self.fs_in, self.fs_out = int(fs_in), int(fs_out)
        self.L, self.M, self.half, self.T = geometry(fs_in, fs_out)
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(self._lib.nafp_resample_create(ctypes.byref(h), self.fs_in, self.fs_out), 'resample_create')
        self.handle = h

    def __del__(self):
        if getattr(self, 'handle', None):
            self._lib.nafp_resample_destroy(self.handle)
            self.handle = None

    def run(self, raw, pieces, out, pieces_dev=None):
        """raw / out: int16 CUDA tensors; pieces: host array of PIECE_DTYPE (checked here, uploaded unless `pieces_dev`, a CUDA
        uint8 tensor holding the same bytes, is given).  Enqueued on the current stream."""
        import torch
        _lib.require_cuda(raw, 'raw'); _lib.require_cuda(out, 'out')
        if raw.dtype != torch.int16 or out.dtype != torch.int16:
            raise TypeError('resample: int16 arenas expected')
        pieces = check_pieces(self.fs_in, self.fs_out, pieces, raw.numel(), out.numel())
        if len(pieces) == 0:
            return out
        if pieces_dev is None:
            pieces_dev = torch.from_numpy(pieces.view(np.uint8).reshape(-1)).to(raw.device)
        with torch.cuda.device(raw.device):
            _lib.check(self._lib.nafp_resample_i16(self.handle, _lib.ptr(raw), raw.numel(), _lib.ptr(pieces_dev), len(pieces),
                                                   _lib.ptr(out), out.numel(), _lib.current_stream()), 'resample_i16')
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
    """The uploaded arena as this kernel takes it: int16, as the loaders' buffers are."""
    return t


def rates_summary(source, formats=False):
    """{'files': n, 'resampled': k, 'rates': {'44100x2': count, ...}} of a SegmentSource / PcmStore; 'resampled' counts the files
    that are converted on the device.  formats=True (utils/ingest.rates_summary): rate x channels x sample format per file class,
    e.g. '48000x2xs24'."""
    rates = {}
    for row in zip(source.rate, source.channels, *([source.format] if formats else [])):
        key = 'x'.join(str(v) for v in row)
        rates[key] = rates.get(key, 0) + 1
    return {'files': len(source.rate), 'resampled': int(sum(bool(x) for x in source.resampled)), 'rates': rates}
