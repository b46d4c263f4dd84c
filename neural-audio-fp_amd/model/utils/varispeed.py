"""Undoing a speed change (tempo and pitch together) of model-rate PCM: host side of `nafp_varispeed_*` (include/nafp.h, DESIGN.md
section 4.10.4).

A step is an unsigned Q24 count of input samples per output sample; a recording played `s` times too fast is undone by
`step_for(s)`.  The conversion exists on the device only (csrc/varispeed.hip, exact integer arithmetic): there is no CPU path, so
whatever materialises samples on the host raises under a step.
"""
import ctypes

import numpy as np

from ... import _lib

PIECE_DTYPE = np.dtype(_lib.VARISPEED_PIECE_DTYPE)
ONE = 1 << 24
STEP_MIN, STEP_MAX = _lib.VARISPEED_STEP_MIN, _lib.VARISPEED_STEP_MAX
SPEED_MIN, SPEED_MAX = 0.8, 1.25


def step_for(speed):
    """The step that undoes a recording played `speed` times too fast; ValueError outside 0.8 .. 1.25."""
    speed = float(speed)
    if not SPEED_MIN <= speed <= SPEED_MAX:            # (a NaN fails the comparison too)
        raise ValueError(f'speed {speed!r} is outside the supported range {SPEED_MIN} .. {SPEED_MAX}')
    return int(round(ONE / speed))


def speed_of(step):
    """The speed reported back for a step."""
    return ONE / int(step)


def geometry(step):
    """(W, T); ValueError for a step outside the range."""
    W, T = ctypes.c_int(), ctypes.c_int()
    if _lib.load().nafp_varispeed_geometry(int(step), ctypes.byref(W), ctypes.byref(T)) != 0:
        raise ValueError(f'varispeed step {step} is outside {STEP_MIN} .. {STEP_MAX} (speeds {SPEED_MIN} .. {SPEED_MAX})')
    return W.value, T.value


def n_out(n_in, step):
    n = int(_lib.load().nafp_varispeed_n_out(int(n_in), int(step)))
    if n < 0:
        raise ValueError(f'varispeed: step {step} is outside {STEP_MIN} .. {STEP_MAX}, or {n_in} samples are not in [0, 2^31)')
    return n


def input_range(n0, n1, n_in, step):
    """Model-rate samples [first, last) of the file that the stretched outputs [n0, n1) read."""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.load().nafp_varispeed_input_range(int(n0), int(n1), int(n_in), int(step), ctypes.byref(a), ctypes.byref(b)),
               'varispeed_input_range')
    return a.value, b.value


def check_pieces(step, pieces, src_samples, out_samples):
    """The kernel's own per-piece checks on the host-built list, before anything is uploaded."""
    pieces = np.ascontiguousarray(pieces, dtype=PIECE_DTYPE)
    _lib.check(_lib.load().nafp_varispeed_check_pieces_host(int(step), pieces.ctypes.data_as(ctypes.c_void_p), len(pieces),
                                                            int(src_samples), int(out_samples)), 'varispeed pieces')
    return pieces


class Plan:
    """nafp_varispeed plan of one step: owns the device table."""

    def __init__(self, step):
        self.step = int(step)
        self.W, self.T = geometry(step)
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(self._lib.nafp_varispeed_create(ctypes.byref(h), self.step), 'varispeed_create')
        self.handle = h

    def __del__(self):
        if getattr(self, 'handle', None):
            self._lib.nafp_varispeed_destroy(self.handle)
            self.handle = None

    def run(self, src, pieces, out, pieces_dev=None):
        """src / out: int16 CUDA tensors; pieces: host array of PIECE_DTYPE (checked here, uploaded unless `pieces_dev`, a CUDA
        uint8 tensor holding the same bytes, is given).  Enqueued on the current stream."""
        import torch
        _lib.require_cuda(src, 'src'); _lib.require_cuda(out, 'out')
        if src.dtype != torch.int16 or out.dtype != torch.int16:
            raise TypeError('varispeed: int16 arenas expected')
        pieces = check_pieces(self.step, pieces, src.numel(), out.numel())
        if len(pieces) == 0:
            return out
        if pieces_dev is None:
            pieces_dev = torch.from_numpy(pieces.view(np.uint8).reshape(-1)).to(src.device)
        with torch.cuda.device(src.device):
            _lib.check(self._lib.nafp_varispeed_i16(self.handle, _lib.ptr(src), src.numel(), _lib.ptr(pieces_dev), len(pieces),
                                                    _lib.ptr(out), out.numel(), _lib.current_stream()), 'varispeed_i16')
        return out


_PLANS = {}


def plan_for(step, device=None):
    """Small cache of plans per (step, device)."""
    import torch
    dev = torch.cuda.current_device() if device is None else torch.device(device).index or 0
    key = (int(step), dev)
    if key not in _PLANS:
        with torch.cuda.device(dev):
            _PLANS[key] = Plan(step)
    return _PLANS[key]


class Stage:
    """The last stage of a launch under a step: the model-rate arena the launch's ingest filled (or the uploaded arena itself, for
    a launch of native files) -> `out_total` stretched int16, which the launch's windows index.  `inner`: the ingest work of the
    launch (ingest.ChunkPieces) or None."""

    def __init__(self, step, pieces, out_total, inner=None):
        self.step, self.pieces, self.out_total, self.inner = int(step), np.asarray(pieces, dtype=PIECE_DTYPE), int(out_total), inner

    def run(self, raw_dev, out=None):
        import torch
        src = raw_dev if self.inner is None else self.inner.run(raw_dev)
        if src.dtype != torch.int16:
            src = src.view(torch.int16)
        if out is None:
            out = torch.empty((max(self.out_total, 1),), dtype=torch.int16, device=src.device)
        return plan_for(self.step, src.device).run(src, self.pieces, out)
