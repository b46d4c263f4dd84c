"""FLAC files: host side of `nafp_flac_*` (include/nafp.h).

Opt-in: NAFP_INGEST_FLAC=1 (the layers: utils/resample.switches).  Without it every loader refuses a `.flac` name as before.  A FLAC file is decoded on the device only (csrc/flac.hip, exact integer arithmetic): a pre-pass turns the WHOLE
FRAMES that cover a sample range into interleaved PCM of the file's own channel count and rate in a byte scratch tensor -- s16
containers for up to 16 bits, s24 above, MSB-justified -- and the general ingest then reads that tensor as 16- or 24-bit PCM.  There
is no CPU path, so whatever materialises samples on the host raises for such a file.

The frame index of a file (byte offset, byte length, first sample, block size per frame) is built once, at construction, by one pass
over the file on the host (`scan`, nafp_flac_index_host).
"""
import ctypes

import numpy as np

from ... import _lib
from .resample import switches

INFO_DTYPE = np.dtype(_lib.FLAC_INFO_DTYPE)
INDEX_DTYPE = np.dtype(_lib.FLAC_INDEX_DTYPE)
FRAME_DTYPE = np.dtype(_lib.FLAC_FRAME_DTYPE)
MAX_BLOCK = 16384
REFUSALS = {1: 'Ogg-encapsulated FLAC is not taken (native FLAC streams are)',
            2: 'no fLaC marker: not a native FLAC stream',
            3: 'the first metadata block is not a 34-byte STREAMINFO',
            4: 'taken: 8, 12, 16, 20 or 24 bits',
            5: f'up to {MAX_BLOCK} is taken'}


def enabled():
    return switches().flac


def container(bps):
    """Bytes per sample of the pre-pass output."""
    return 2 if bps <= 16 else 3


def scan(data):
    """STREAMINFO and frame index of the stream in `data` (bytes): (info record of INFO_DTYPE, index array of INDEX_DTYPE).  A
    stream that is not taken has info['refusal'] != 0 and an empty index."""
    lib = _lib.load()
    buf = np.frombuffer(data, np.uint8)
    info = np.zeros(1, INFO_DTYPE)
    cap = len(buf) // 64 + 1024
    while True:
        index = np.zeros(cap, INDEX_DTYPE)
        _lib.check(lib.nafp_flac_index_host(buf.ctypes.data_as(ctypes.c_void_p), len(buf), info.ctypes.data_as(ctypes.c_void_p),
                                            index.ctypes.data_as(ctypes.c_void_p), cap), 'flac_index_host')
        n = int(info[0]['n_indexed'])
        if n <= cap:
            return info[0], index[:n]
        cap = n


class Index:
    """The frames of one file: offset / n_bytes / block (arrays) and start = the position of each frame's first sample in the file's
    PCM (the coded first sample relative to the first indexed frame's), n + 1 entries."""

    def __init__(self, index, channels, bps, rate):
        self.offset = index['offset'].astype(np.int64)
        self.block = index['block_size'].astype(np.int64)
        # up to the next indexed frame (the last one: the end of the file); a frame reads what it needs of that and no more
        self.n_bytes = np.minimum(index['n_bytes'].astype(np.int64), (1 << 31) - 1)
        self.start = np.concatenate([[0], np.cumsum(self.block)]).astype(np.int64)
        self.channels, self.bps, self.rate = int(channels), int(bps), int(rate)

    def __len__(self):
        return len(self.block)


def frame_range(index, first, last):
    """The whole frames [k0, k1) that cover the samples [first, last) (k0 == k1: none)."""
    if last <= first or len(index) == 0:
        return 0, 0
    k0 = int(np.searchsorted(index.start, first, side='right') - 1)
    k1 = int(np.searchsorted(index.start, last, side='left'))
    return max(k0, 0), min(max(k1, k0), len(index))


def records(index, k0, k1, raw_base, scratch_base):
    """FRAME_DTYPE rows of the frames [k0, k1) whose bytes offset[k0] .. offset[k1-1] + n_bytes[k1-1] sit at raw_base of the raw arena
    and whose PCM goes to scratch_base (bytes) of the scratch arena, in order.  -> (rows, raw bytes to upload, scratch bytes)."""
    rows = np.zeros(k1 - k0, FRAME_DTYPE)
    if k1 <= k0:
        return rows, 0, 0
    per = index.channels * container(index.bps)
    rows['raw_off'] = raw_base + index.offset[k0:k1] - index.offset[k0]
    rows['scratch_off'] = scratch_base + (index.start[k0:k1] - index.start[k0]) * per
    rows['n_bytes'] = index.n_bytes[k0:k1]
    rows['block_size'] = index.block[k0:k1]
    rows['channels'], rows['bps'], rows['rate'] = index.channels, index.bps, index.rate
    raw_bytes = int(index.offset[k1 - 1] + index.n_bytes[k1 - 1] - index.offset[k0])
    return rows, raw_bytes, int(index.start[k1] - index.start[k0]) * per


def check_frames(frames, raw_size, scratch_size):
    """The kernels' own per-record checks on the host-built list, before anything is uploaded."""
    frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    _lib.check(_lib.load().nafp_flac_check_frames_host(frames.ctypes.data_as(ctypes.c_void_p), len(frames), int(raw_size),
                                                       int(scratch_size)), 'flac frames')
    return frames


def decode(raw, frames, scratch, status=None):
    """raw: uint8 CUDA tensor (the files' frames); scratch: uint8 CUDA tensor; frames: host array of FRAME_DTYPE (checked here, then
    uploaded); status: optional int32 CUDA tensor, one per frame.  Enqueued on the current stream."""
    import torch
    _lib.require_cuda(raw, 'raw'); _lib.require_cuda(scratch, 'scratch')
    if raw.dtype != torch.uint8 or scratch.dtype != torch.uint8:
        raise TypeError('flac decode: uint8 raw and scratch arenas expected')
    if status is not None and (status.dtype != torch.int32 or status.numel() < len(frames) or not status.is_cuda):
        raise TypeError('flac decode: status is an int32 CUDA tensor with one element per frame')
    frames = check_frames(frames, raw.numel(), scratch.numel())
    if len(frames) == 0:
        return scratch
    frames_dev = torch.from_numpy(frames.view(np.uint8).reshape(-1)).to(raw.device)
    with torch.cuda.device(raw.device):
        _lib.check(_lib.load().nafp_flac_decode(_lib.ptr(raw), raw.numel(), _lib.ptr(frames_dev), len(frames), _lib.ptr(scratch),
                                                scratch.numel(), _lib.ptr(status), _lib.current_stream()), 'flac_decode')
    return scratch


class FailedFrames:
    """Which frames of a source's FLAC files failed their checks, kept ON THE DEVICE: one byte per frame of every file (frame k of
    file f at base[f] + k), set by the launches that decode it -- a frame two launches share is still one frame.  `count()` reads
    the sum once."""

    def __init__(self, frames_per_file):
        self.base = np.concatenate([[0], np.cumsum(frames_per_file)]).astype(np.int64)
        self.flags = None

    def mark(self, ids_dev, status):
        import torch
        if self.flags is None or self.flags.device != status.device:
            self.flags = torch.zeros((max(int(self.base[-1]), 1),), dtype=torch.uint8, device=status.device)
            torch.cuda.synchronize(status.device)       # once: launches on other streams find it zeroed
        self.flags.index_put_((ids_dev,), (status != 0).to(torch.uint8), accumulate=False)

    def count(self, dist=None):
        """Failed frames so far.  dist (torch.distributed, initialised): over all ranks, a frame two ranks decoded counted once."""
        import torch
        if dist is not None:
            if self.flags is None:
                self.flags = torch.zeros((max(int(self.base[-1]), 1),), dtype=torch.uint8, device=torch.device('cuda', torch.cuda.current_device()))
            torch.cuda.synchronize(self.flags.device)
            dist.all_reduce(self.flags, op=dist.ReduceOp.MAX)
        return 0 if self.flags is None else int(self.flags.sum(dtype=torch.int64).item())


def failed_count(source, dist=None):
    """Frames of a SegmentSource's / PcmStore's FLAC files that failed their checks in the launches so far: one read."""
    ff = getattr(source, 'flac_failed', None)
    return 0 if ff is None else ff.count(dist)


class PrePass:
    """The FLAC work of one launch: `frames` (host array of FRAME_DTYPE) decode frames of the uploaded raw arena into a uint8 scratch
    tensor of `scratch_bytes`; the launch's ingest pieces of FLAC files then index that tensor as 16- or 24-bit PCM.  `failed`
    (FailedFrames) with `ids` (the frames' places in it) collects the statuses on the device."""

    def __init__(self, frames, scratch_bytes, failed=None, ids=None):
        self.frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
        self.scratch_bytes = int(scratch_bytes)
        self.failed, self.ids = failed, ids

    def run(self, raw):
        import torch
        scratch = torch.empty((max(self.scratch_bytes, 1),), dtype=torch.uint8, device=raw.device)
        status = None
        if self.failed is not None and len(self.frames):
            status = torch.empty((len(self.frames),), dtype=torch.int32, device=raw.device)
        decode(raw, self.frames, scratch, status)
        if status is not None:
            self.failed.mark(torch.from_numpy(np.ascontiguousarray(self.ids, np.int64)).to(raw.device), status)
        return scratch
