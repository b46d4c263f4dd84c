"""Block codecs in WAV files -- G.711 A-law / mu-law, IMA ADPCM and MS ADPCM at 4 bits -- and, under NAFP_INGEST_AIFF=1, the G.711
and Apple IMA4 ('qtima4') bodies of AIFF-C and AU files: host side of `nafp_codec_*` (include/nafp.h, DESIGN.md sections 4.10.2, 4.10.5).

Opt-in: NAFP_INGEST_CODECS=1 (the layers: utils/resample.switches).  Without it every loader refuses these files by name, as before.
A codec file is decoded on the device only (csrc/codec.hip, exact integer arithmetic): a pre-pass turns the WHOLE BLOCKS that
cover a frame range into interleaved 16-bit PCM in a scratch tensor, and the general ingest then reads that tensor as 16-bit
PCM.  There is no CPU path, so whatever materialises samples on the host raises for such a file.
"""
import ctypes

import numpy as np

from ... import _lib
from .resample import switches

PIECE_DTYPE = np.dtype(_lib.CODEC_PIECE_DTYPE)
CODECS = _lib.CODECS                               # format name -> NAFP_CODEC_* code
MAX_BLOCK_ALIGN = 4096


def enabled():
    return switches().codecs


def samples_per_block(codec, channels, block_align):
    """Frames per block, or -1 for a (codec, channels, block_align) the decoder does not take.  `codec`: name or code."""
    code = CODECS.get(codec, codec)
    return int(_lib.load().nafp_codec_samples_per_block(int(code), int(channels), int(block_align)))


def block_range(first, last, spb):
    """The whole blocks [b0, b1) that cover the frames [first, last) (b0 == b1: none)."""
    if last <= first:
        return 0, 0
    return first // spb, -(-last // spb)


def check_pieces(pieces, raw_size, out_samples):
    """The kernel's own per-piece checks on the host-built list, before anything is uploaded."""
    pieces = np.ascontiguousarray(pieces, dtype=PIECE_DTYPE)
    _lib.check(_lib.load().nafp_codec_check_pieces_host(pieces.ctypes.data_as(ctypes.c_void_p), len(pieces), int(raw_size),
                                                        int(out_samples)), 'codec pieces')
    return pieces


def decode(raw, pieces, out):
    """raw: uint8 CUDA tensor (the files' blocks); out: int16 CUDA tensor; pieces: host array of PIECE_DTYPE (checked here, then
    uploaded).  Enqueued on the current stream."""
    import torch
    _lib.require_cuda(raw, 'raw'); _lib.require_cuda(out, 'out')
    if raw.dtype != torch.uint8 or out.dtype != torch.int16:
        raise TypeError('codec decode: a uint8 raw arena and an int16 output arena expected')
    pieces = check_pieces(pieces, raw.numel(), out.numel())
    if len(pieces) == 0:
        return out
    pieces_dev = torch.from_numpy(pieces.view(np.uint8).reshape(-1)).to(raw.device)
    with torch.cuda.device(raw.device):
        _lib.check(_lib.load().nafp_codec_decode_i16(_lib.ptr(raw), raw.numel(), _lib.ptr(pieces_dev), len(pieces), _lib.ptr(out),
                                                     out.numel(), _lib.current_stream()), 'codec_decode_i16')
    return out


class PrePass:
    """The codec work of one launch: `pieces` (host array of PIECE_DTYPE) decode blocks of the uploaded raw arena into an int16
    scratch tensor of `scratch_samples`; the launch's ingest pieces of codec files then index the scratch's BYTES as 16-bit PCM."""

    def __init__(self, pieces, scratch_samples):
        self.pieces = np.ascontiguousarray(pieces, dtype=PIECE_DTYPE)
        self.scratch_samples = int(scratch_samples)

    def run(self, raw):
        import torch
        scratch = torch.empty((max(self.scratch_samples, 1),), dtype=torch.int16, device=raw.device)
        return decode(raw, self.pieces, scratch)
