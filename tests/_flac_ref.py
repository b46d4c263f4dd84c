"""FLAC in plain numpy / Python, for the tests of nafp_flac_* (include/nafp.h, csrc/flac_decode.h): a WRITER that builds a valid
stream from given samples and an explicit recipe per frame and subframe, and a READER, a bit-level restatement of the decode and of
the frame index.  The two share no code beyond the two CRC tables.  The ground truth of every test is the samples handed to the
writer, not either decoder's output.

No FLAC file written by another implementation and no other decoder exist where these tests were written: parity with
libFLAC-written files rests on test_flac_host.py::test_md5_of_real_files, once NAFP_FLAC_SAMPLES points it at some.

Writer recipes
    frame:    {'block': n, 'assign': 0..10 (default channels - 1: independent), 'subframes': one recipe or a list per channel,
               'bs_form': 'auto' | 'code' | '8bit' | '16bit', 'rate_form': 'streaminfo' | 'code' | 'khz' | 'hz' | 'tenhz',
               'bps_form': 'streaminfo' | 'code', 'number': coded number (default: continuing)}
    subframe: {'type': 'constant' | 'verbatim' | 'fixed' | 'lpc', 'order', 'coefs', 'precision', 'shift', 'wasted': 0,
               'method': 0 | 1, 'porder': 0, 'params': None (best Rice parameter per partition) | [k | ('esc', n_bits), ...]}
"""
import hashlib
import struct

import numpy as np


def _table(poly, width):
    top, mask = 1 << (width - 1), (1 << width) - 1
    out = []
    for i in range(256):
        c = i << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        out.append(c)
    return out


CRC8_TABLE = _table(0x07, 8)
CRC16_TABLE = _table(0x8005, 16)


def crc8(data):
    c = 0
    for b in data:
        c = CRC8_TABLE[c ^ b]
    return c


def crc16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xffff) ^ CRC16_TABLE[(c >> 8) ^ b]
    return c


BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
BPS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}
FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


# =================================================================================================================================
# writer
# =================================================================================================================================
class _Bits:
    """Fields (value, width) packed MSB first; a unary run of q zeros and a one is the field (1, q + 1)."""

    def __init__(self):
        self.v, self.n = [], []

    def put(self, v, n):
        self.v.append(np.array([v], np.uint64))
        self.n.append(np.array([n], np.int64))

    def put_many(self, v, n):
        v = np.asarray(v).astype(np.int64).astype(np.uint64)
        self.v.append(v)
        self.n.append(np.broadcast_to(np.asarray(n, np.int64), v.shape).copy())

    def tobytes(self):
        v, n = np.concatenate(self.v), np.concatenate(self.n)
        end = np.cumsum(n)
        total = int(end[-1])
        bits = np.zeros(total + (-total % 8), np.uint8)
        for j in range(int(min(n.max(), 40))):
            m = n > j
            bits[end[m] - 1 - j] = ((v[m] >> np.uint64(j)) & np.uint64(1)).astype(np.uint8)
        return np.packbits(bits).tobytes()


def _wrap32(x):
    return ((np.asarray(x, np.int64) + (1 << 31)) & 0xffffffff) - (1 << 31)


def _utf8(v):
    if v < 0x80:
        return bytes([v])
    for extra in range(1, 7):
        if v < 1 << (5 * extra + 6) or extra == 6:
            lead = (0xff << (7 - extra)) & 0xff
            return bytes([lead | (v >> (6 * extra))] + [0x80 | ((v >> (6 * k)) & 0x3f) for k in range(extra - 1, -1, -1)])


def _residual(bits, res, block, order, method, porder, params):
    bits.put(method, 2)
    bits.put(porder, 4)
    per = block >> porder
    assert block % (1 << porder) == 0 and per >= order, 'partition order'
    pb, esc = (5, 31) if method else (4, 15)
    i = 0
    for p in range(1 << porder):
        cnt = per - (order if p == 0 else 0)
        seg = res[i:i + cnt]
        i += cnt
        u = np.where(seg >= 0, 2 * seg, -2 * seg - 1).astype(np.int64)
        prm = params[p] if params is not None else None
        if prm is None:
            costs = [int((u >> k).sum()) + cnt * (k + 1) for k in range(esc)]
            prm = int(np.argmin(costs))
        if isinstance(prm, tuple):
            nb = prm[1]
            bits.put(esc, pb)
            bits.put(nb, 5)
            if nb == 0:
                assert not seg.any()
            else:
                assert cnt == 0 or (seg.min() >= -(1 << (nb - 1)) and seg.max() < (1 << (nb - 1))), 'escape width'
                bits.put_many(seg & ((1 << nb) - 1), nb)
        else:
            assert 0 <= prm < esc
            bits.put(prm, pb)
            v, n = np.empty(2 * cnt, np.int64), np.empty(2 * cnt, np.int64)
            v[0::2], n[0::2] = 1, (u >> prm) + 1
            v[1::2], n[1::2] = u & ((1 << prm) - 1), prm
            bits.put_many(v, n)


def _subframe(bits, x, w, r):
    x = np.asarray(x, np.int64)
    block, wasted, kind = len(x), r.get('wasted', 0), r['type']
    order = r.get('order', 0) if kind in ('fixed', 'lpc') else 0
    code = {'constant': 0, 'verbatim': 1, 'fixed': 8 + order, 'lpc': 31 + order}[kind]
    if 'type_code' in r:                    # for corrupt streams: any 6-bit code
        code = r['type_code']
    bits.put(0, 1)
    bits.put(code, 6)
    if wasted:
        assert not (x & ((1 << wasted) - 1)).any(), 'wasted bits are not zero'
        bits.put(1, 1)
        bits.put(1, wasted)
    else:
        bits.put(0, 1)
    s = x >> wasted
    w -= wasted
    assert w >= 1 and s.min() >= -(1 << (w - 1)) and s.max() < (1 << (w - 1)), 'sample width'
    mask = (1 << w) - 1
    if kind == 'constant':
        assert (s == s[0]).all()
        bits.put(int(s[0]) & mask, w)
        return
    if kind == 'verbatim':
        bits.put_many(s & mask, w)
        return
    if order:
        bits.put_many(s[:order] & mask, w)
    if kind == 'lpc':
        coefs, precision, shift = [int(c) for c in r['coefs']], r['precision'], r['shift']
        assert len(coefs) == order and 1 <= precision <= 15 and 0 <= shift <= 15
        assert all(-(1 << (precision - 1)) <= c < (1 << (precision - 1)) for c in coefs)
        bits.put(precision - 1, 4)
        bits.put(shift, 5)
        bits.put_many(np.array(coefs, np.int64) & ((1 << precision) - 1), precision)
    else:
        coefs, shift = FIXED[order], 0
    total = np.zeros(block - order, np.int64)
    for j, c in enumerate(coefs):
        total += c * s[order - 1 - j:block - 1 - j]
    res = _wrap32(s[order:] - _wrap32(total >> shift))
    _residual(bits, res, block, order, r.get('method', 0), r.get('porder', 0), r.get('params'))


def _channels(block, assign):
    """The channel signals of one frame from its (n, ch) samples, and their widths beyond bps."""
    x = np.asarray(block, np.int64)
    if assign < 8:
        return [x[:, c] for c in range(x.shape[1])], [0] * x.shape[1]
    left, right = x[:, 0], x[:, 1]
    if assign == 8:
        return [left, left - right], [0, 1]
    if assign == 9:
        return [left - right, right], [1, 0]
    return [(left + right) >> 1, left - right], [0, 1]


class Stream:
    """data: the file's bytes; frames: [(offset, n_bytes, first sample as coded, block size)]; audio_off; header_len per frame."""

    def __init__(self, data, frames, audio_off, header_lens):
        self.data, self.frames, self.audio_off, self.header_lens = data, frames, audio_off, header_lens


def md5_of(samples, bps):
    x = np.asarray(samples, np.int64)
    width = (bps + 7) // 8
    raw = (x.reshape(-1) & ((1 << (8 * width)) - 1)).astype('<u8').view(np.uint8).reshape(-1, 8)[:, :width]
    return hashlib.md5(raw.tobytes()).digest()


def frame_bytes(samples, bps, rate, recipe, number, variable=False):
    """One frame: (bytes, header length)."""
    x = np.asarray(samples, np.int64)
    if x.ndim == 1:
        x = x[:, None]
    block, ch = x.shape
    assign = recipe.get('assign', ch - 1)
    form = recipe.get('bs_form', 'auto')
    if form == 'auto':
        form = 'code' if block in BS_CODES else ('8bit' if block <= 256 else '16bit')
    bs_code = BS_CODES[block] if form == 'code' else (6 if form == '8bit' else 7)
    rform = recipe.get('rate_form', 'streaminfo')
    rate_code = {'streaminfo': 0, 'khz': 12, 'hz': 13, 'tenhz': 14}.get(rform)
    if rate_code is None:
        rate_code = RATE_CODES[rate]
    size_code = BPS_CODES[bps] if recipe.get('bps_form', 'streaminfo') == 'code' else 0
    head = bytes([0xff, 0xf8 | (1 if variable else 0), (bs_code << 4) | rate_code, (assign << 4) | (size_code << 1)]) + _utf8(number)
    if bs_code == 6:
        head += bytes([block - 1])
    elif bs_code == 7:
        head += struct.pack('>H', block - 1)
    if rate_code == 12:
        head += bytes([rate // 1000])
    elif rate_code == 13:
        head += struct.pack('>H', rate)
    elif rate_code == 14:
        head += struct.pack('>H', rate // 10)
    head += bytes([crc8(head)])
    bits = _Bits()
    subs = recipe.get('subframes', {'type': 'fixed', 'order': 2})
    signals, extra = _channels(x, assign)
    for c, (sig, e) in enumerate(zip(signals, extra)):
        _subframe(bits, sig, bps + e, subs[c] if isinstance(subs, (list, tuple)) else subs)
    body = head + bits.tobytes()
    return body + struct.pack('>H', crc16(body)), len(head)


def write_stream(samples, bps, rate, frames=None, block=4096, variable=False, first_number=0, total=None, id3=0, sub=None,
                 max_block=None):
    """samples: (n, ch) integers of `bps` bits.  frames: recipes covering the n samples in order; None: blocks of `block` with the
    subframe recipe `sub` (default: fixed order 2).  first_number: the first frame's number (fixed) or sample number (variable).
    total: STREAMINFO's total samples (None: n).  id3: bytes of an ID3v2 tag in front."""
    x = np.asarray(samples, np.int64)
    if x.ndim == 1:
        x = x[:, None]
    n, ch = x.shape
    if frames is None:
        sub = sub or {'type': 'fixed', 'order': 2}
        frames = [{'block': min(block, n - a), 'subframes': sub} for a in range(0, n, block)]
        last, po = frames[-1]['block'], sub.get('porder', 0)
        while po and (last % (1 << po) or (last >> po) < sub.get('order', 0)):       # a shorter last frame: the largest order it allows
            po -= 1
        frames[-1]['subframes'] = dict(sub, porder=po, order=min(sub.get('order', 0), last)) if sub['type'] == 'fixed' else dict(sub, porder=po)
    assert sum(f['block'] for f in frames) == n
    blocks = [f['block'] for f in frames]
    big = max_block or max(blocks)
    out, index, header_lens, pos = [], [], [], 0
    number = first_number
    for f in frames:
        coded = f.get('number', number)
        data, hl = frame_bytes(x[pos:pos + f['block']], bps, rate, f, coded, variable)
        index.append((data, coded if variable else coded * big, f['block']))
        header_lens.append(hl)
        out.append(data)
        pos += f['block']
        number = coded + (f['block'] if variable else 1)
    sizes = [len(d) for d in out]
    small = min(blocks[:-1]) if len(blocks) > 1 else blocks[0]
    info = struct.pack('>HH', small, big) + struct.pack('>I', min(sizes))[1:] + struct.pack('>I', max(sizes))[1:]
    t = n if total is None else total
    info += struct.pack('>Q', (rate << 44) | ((ch - 1) << 41) | ((bps - 1) << 36) | t) + md5_of(x, bps)
    head = b''
    if id3:
        size = id3 - 10
        head = b'ID3\x04\x00\x00' + bytes([(size >> 21) & 0x7f, (size >> 14) & 0x7f, (size >> 7) & 0x7f, size & 0x7f]) + bytes(size)
    head += b'fLaC' + bytes([0x00, 0, 0, 34]) + info + bytes([0x81, 0, 0, 6]) + bytes(6)          # STREAMINFO, then a padding block
    offs = np.cumsum([len(head)] + sizes)
    return Stream(head + b''.join(out), [(int(o), len(d), fs, b) for o, (d, fs, b) in zip(offs, index)], len(head), header_lens)


def justified(samples, bps):
    """The bytes the pre-pass writes for these samples: little-endian s16 containers holding v << (16 - bps), or 3-byte s24
    containers holding v << (24 - bps), interleaved."""
    x = np.asarray(samples, np.int64).reshape(-1)
    if bps <= 16:
        return ((x << (16 - bps)) & 0xffff).astype('<u2').view(np.uint8)
    return ((x << (24 - bps)) & 0xffffff).astype('<u4').view(np.uint8).reshape(-1, 4)[:, :3].reshape(-1).copy()


def pcm_wav(samples, bps, rate):
    """The MSB-justified PCM WAV (16- or 24-bit) of the same samples."""
    x = np.asarray(samples, np.int64)
    if x.ndim == 1:
        x = x[:, None]
    ch, width = x.shape[1], 2 if bps <= 16 else 3
    body = justified(x, bps).tobytes()
    fmt = struct.pack('<HHIIHH', 1, ch, rate, rate * ch * width, ch * width, 8 * width)
    return b'RIFF' + struct.pack('<I', 36 + len(body)) + b'WAVE' + b'fmt ' + struct.pack('<I', 16) + fmt + b'data' + \
        struct.pack('<I', len(body)) + body


def music(n, rate, ch, bps, seed, scale=0.5):
    """Music-like test signal: a few decaying partials and noise, per channel, `bps` bits."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    out = np.zeros((n, ch))
    for c in range(ch):
        for k in range(5):
            f0 = rng.uniform(80, min(3000, rate / 4))
            out[:, c] += rng.uniform(.2, 1) * np.sin(2 * np.pi * f0 * t + rng.uniform(0, 6)) * np.exp(-((t * rng.uniform(.2, 2)) % 1.))
        out[:, c] += 0.02 * rng.standard_normal(n)
    if ch > 1:
        out[:, 1:] = 0.7 * out[:, :1] + 0.3 * out[:, 1:]
    out *= scale * (1 << (bps - 1)) / max(np.abs(out).max(), 1e-9)
    return np.round(out).astype(np.int64)


def lpc_recipe(x, order, precision=12, porder=0, method=0):
    """A reasonable LPC recipe for the 1-D signal x (least squares, quantised), for the measurement rows."""
    x = np.asarray(x, np.float64)
    rows = np.stack([x[order - 1 - j:len(x) - 1 - j] for j in range(order)], 1)
    a = np.linalg.lstsq(rows, x[order:], rcond=None)[0]
    shift = int(max(0, min(15, precision - 2 - int(np.ceil(np.log2(max(np.abs(a).max(), 1e-9)))))))
    q = np.clip(np.round(a * (1 << shift)), -(1 << (precision - 1)), (1 << (precision - 1)) - 1).astype(np.int64)
    return {'type': 'lpc', 'order': order, 'coefs': [int(c) for c in q], 'precision': precision, 'shift': shift, 'porder': porder,
            'method': method}


_GRID = []


def variant_grid():
    """[(name, Stream, samples (n, ch), bps)]: every depth x channel count, the stereo modes at full scale, every subframe, residual
    and block-size variant the decoder takes.  Built once; small streams."""
    if _GRID:
        return _GRID

    def add(name, x, bps, rate=44100, **kw):
        _GRID.append((name, write_stream(x, bps, rate, **kw), np.asarray(x, np.int64).reshape(len(x), -1), bps))

    def full(n, ch, bps, seed):              # full-scale samples of both signs among music
        x = music(n, 44100, ch, bps, seed, .95)
        x[1::7] = (1 << (bps - 1)) - 1
        x[4::7] = -(1 << (bps - 1))
        if ch > 1:
            x[1::14, 1::2] = -(1 << (bps - 1))
            x[4::14, 1::2] = (1 << (bps - 1)) - 1
        return x

    for bps in (8, 12, 16, 20, 24):
        for ch in range(1, 9):
            add(f'depth{bps}x{ch}', full(96, ch, bps, 10 * bps + ch), bps, block=64, sub={'type': 'fixed', 'order': 2, 'method': 1})
    for bps in (16, 24):
        for assign in (8, 9, 10):
            x = full(160, 2, bps, 100 + assign)
            add(f'stereo{assign}x{bps}', x, bps, frames=[{'block': 80, 'assign': assign, 'subframes': {'type': 'fixed', 'order': 0, 'method': 1}},
                                                         {'block': 80, 'assign': assign, 'subframes': {'type': 'verbatim'}}])
    x = music(256, 44100, 1, 16, 7, .9)
    add('constant', np.full((64, 2), -1234), 16, sub={'type': 'constant'})
    add('verbatim', x, 16, block=128, sub={'type': 'verbatim'})
    for order in range(5):
        add(f'fixed{order}', x, 16, block=128, sub={'type': 'fixed', 'order': order, 'porder': 1})
    for order in (1, 2, 12, 32):
        add(f'lpc{order}', x, 16, block=128, sub=lpc_recipe(x[:, 0], order, 13, porder=1))
    add('precision1', x, 16, block=128, sub={'type': 'lpc', 'order': 2, 'coefs': [-1, 0], 'precision': 1, 'shift': 0, 'method': 1})
    add('precision15_shift14', x, 16, block=128, sub={'type': 'lpc', 'order': 2, 'coefs': [16000, -8100], 'precision': 15, 'shift': 14})
    add('shift0', x, 16, block=128, sub={'type': 'lpc', 'order': 3, 'coefs': [2, -2, 1], 'precision': 3, 'shift': 0, 'method': 1})
    big = np.full((128, 1), (1 << 23) - 5) - np.arange(128)[:, None] % 3
    add('sum_above_32_bits', big, 24, block=128, sub={'type': 'lpc', 'order': 32, 'coefs': [16383] * 32, 'precision': 15, 'shift': 14, 'method': 1})
    flat = np.full((128, 1), 300) + (np.arange(128)[:, None] // 50)
    add('rice0', flat, 16, block=128, sub={'type': 'fixed', 'order': 1, 'params': [0]})
    noise = np.random.default_rng(3).integers(-30000, 30000, size=(128, 1))
    add('rice14', noise, 16, block=128, sub={'type': 'fixed', 'order': 0, 'params': [14]})
    add('rice30', full(128, 1, 24, 5), 24, block=128, sub={'type': 'fixed', 'order': 4, 'method': 1, 'params': [30]})
    add('escape0', np.full((128, 1), 77), 16, block=128, sub={'type': 'fixed', 'order': 1, 'params': [('esc', 0)]})
    steps = -np.cumsum(np.random.default_rng(4).integers(0, 2, size=(128, 1)), 0)
    add('escape1', steps, 16, block=128, sub={'type': 'fixed', 'order': 1, 'porder': 1, 'params': [('esc', 1), None]})
    add('escape25', full(128, 2, 24, 6), 24, frames=[{'block': 128, 'assign': 8, 'subframes': {'type': 'fixed', 'order': 0, 'method': 1,
                                                                                                 'params': [('esc', 25)]}}])
    add('porder_largest', x, 16, block=64, sub={'type': 'fixed', 'order': 1, 'porder': 6})
    add('wasted1', x & ~1, 16, block=128, sub={'type': 'fixed', 'order': 2, 'wasted': 1})
    add('wasted7', full(128, 2, 24, 8) & ~127, 24, frames=[{'block': 128, 'assign': 8, 'subframes': {'type': 'fixed', 'order': 2, 'wasted': 7,
                                                                                                        'method': 1}}])
    long = music(16384, 44100, 1, 8, 9, .9)
    for block in (192, 576, 1152, 2304, 4608, 256, 512, 1024, 2048, 4096, 8192, 16384):
        add(f'block_code{block}', long[:block], 8, block=block, sub={'type': 'fixed', 'order': 1})
    for block, form in ((16, '8bit'), (256, '8bit'), (257, '16bit'), (4096, '16bit'), (16384, '16bit')):
        add(f'block_{form}{block}', long[:block], 8, frames=[{'block': block, 'bs_form': form, 'subframes': {'type': 'fixed', 'order': 1}}])
    add('short_last', long[:4096 * 2 + 1000], 8, block=4096, sub={'type': 'fixed', 'order': 2})
    for form, rate in (('code', 48000), ('khz', 32000), ('hz', 11025), ('tenhz', 352800)):
        add(f'rate_{form}', x, 16, rate=rate, frames=[{'block': 256, 'rate_form': form, 'bps_form': 'code'}])
    return _GRID


def golden_streams():
    """The seed streams of tools/flac_host_check.cpp, kept as tests/golden/flac_streams_v1.bin (b'NAFPFLAC', uint32 count, then
    uint32 length + bytes per stream; `python tests/_flac_ref.py` rewrites it).  Stream 0 is the one named_mutations() works on."""
    out = []
    x = music(16 * 6, 8000, 2, 16, 1, .9)
    lpc2 = {'type': 'lpc', 'order': 2, 'coefs': [1900, -900], 'precision': 12, 'shift': 10}
    out.append(write_stream(x, 16, 8000, frames=[{'block': 16, 'assign': a, 'subframes': sf} for a, sf in
                                                   ((1, lpc2), (10, {'type': 'fixed', 'order': 2}), (8, lpc2), (9, {'type': 'verbatim'}),
                                                    (1, {'type': 'fixed', 'order': 4, 'porder': 2}), (10, lpc2))]))
    x = music(1024, 44100, 2, 16, 2, .8)
    out.append(write_stream(x, 16, 44100, block=256, sub=lpc_recipe(x[:, 0], 8, 12, porder=2)))
    x = music(600, 48000, 2, 24, 3, 1.)
    out.append(write_stream(x, 24, 48000, variable=True, frames=[
        {'block': 192, 'assign': 8, 'subframes': {'type': 'fixed', 'order': 4, 'method': 1, 'porder': 1, 'params': [('esc', 27), None]}},
        {'block': 192, 'assign': 10, 'subframes': lpc_recipe(x[:, 0], 12, 15, method=1), 'rate_form': 'code', 'bps_form': 'code'},
        {'block': 216, 'assign': 9, 'subframes': {'type': 'fixed', 'order': 1}, 'rate_form': 'khz'}]))
    x = music(300, 22050, 1, 8, 4, .9) & ~3
    out.append(write_stream(x, 8, 22050, frames=[{'block': 100, 'subframes': {'type': 'verbatim', 'wasted': 2}},
                                                 {'block': 100, 'subframes': {'type': 'fixed', 'order': 3, 'wasted': 1}, 'bs_form': '16bit'},
                                                 {'block': 100, 'subframes': {'type': 'fixed', 'order': 0, 'params': [0]}, 'rate_form': 'hz'}]))
    x = music(192, 32000, 3, 20, 5, .7)
    out.append(write_stream(x, 20, 32000, block=64, sub=lpc_recipe(x[:, 1], 32, 14)))
    x = music(500, 96000, 8, 12, 6, .9)
    x[100:200, 3] = 77
    out.append(write_stream(x, 12, 96000, variable=True, first_number=4000, frames=[
        {'block': 100, 'subframes': {'type': 'fixed', 'order': 2}}, {'block': 100, 'subframes': [{'type': 'fixed', 'order': 1}] * 3 +
         [{'type': 'constant'}] + [{'type': 'verbatim'}] * 4}, {'block': 300, 'subframes': {'type': 'fixed', 'order': 2, 'porder': 2}, 'rate_form': 'tenhz'}]))
    return out


def named_mutations(stream):
    """The six corrupt-input cases that test_gpu_flac.py launches on the device, all on frame 1 of golden stream 0, with the same
    definitions as tools/flac_host_check.cpp, which runs them (and thousands more) under the sanitizers first: name ->
    (bytes of the whole stream, {field: value} to overwrite in frame 1's record)."""
    off, nb, _, block = stream.frames[1]
    hl, d = stream.header_lens[1], stream.data

    def patched(changes):
        b = bytearray(d)
        for k, v in changes.items():
            b[k] = v(b[k]) if callable(v) else v
        return bytes(b)

    return {'bit_flip': (patched({off + nb // 2: lambda v: v ^ 0x10}), {}),
            'truncation': (d, {'n_bytes': nb - 3}),
            'unary_run': (patched({k: 0 for k in range(off + hl + 2, off + nb - 1)}), {}),
            'lpc_order_above_block': (patched({off + hl: 0x7e}), {}),
            'reserved_subframe_type': (patched({off + hl: 0x04}), {}),
            'inconsistent_record': (d, {'raw_off': len(d) - nb + 1})}


# =================================================================================================================================
# reader: a bit-level restatement
# =================================================================================================================================
class Refused(ValueError):
    pass


class _Fail(Exception):
    pass


class _Reader:
    def __init__(self, data):
        self.d, self.pos, self.end = data, 0, 8 * len(data)

    def u(self, n):
        if n == 0:
            return 0
        if self.pos + n > self.end:
            raise _Fail('truncated')
        a, b = self.pos >> 3, (self.pos + n + 7) >> 3
        v = int.from_bytes(self.d[a:b], 'big') >> (8 * b - self.pos - n)
        self.pos += n
        return v & ((1 << n) - 1)

    def s(self, n):
        v = self.u(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self):
        q = 0
        while True:
            if self.pos >= self.end:
                raise _Fail('truncated')
            byte = self.d[self.pos >> 3]
            for k in range(self.pos & 7, 8):
                self.pos += 1
                if (byte >> (7 - k)) & 1:
                    return q
                q += 1


def read_streaminfo(data):
    """{'rate', 'channels', 'bps', 'min_block', 'max_block', 'total', 'md5', 'audio_off'}; Refused by name."""
    pos = 0
    if data[:3] == b'ID3' and len(data) >= 10:
        pos = 10 + ((data[6] & 0x7f) << 21 | (data[7] & 0x7f) << 14 | (data[8] & 0x7f) << 7 | (data[9] & 0x7f)) + (10 if data[5] & 0x10 else 0)
    if data[pos:pos + 4] == b'OggS':
        raise Refused('Ogg-encapsulated FLAC')
    if data[pos:pos + 4] != b'fLaC':
        raise Refused('no fLaC marker')
    pos += 4
    if len(data) < pos + 38 or data[pos] & 0x7f != 0 or data[pos + 1:pos + 4] != b'\x00\x00\x22':
        raise Refused('the first metadata block is not a 34-byte STREAMINFO')
    last = data[pos] >> 7
    s = data[pos + 4:pos + 38]
    word = int.from_bytes(s[10:18], 'big')
    info = {'min_block': int.from_bytes(s[0:2], 'big'), 'max_block': int.from_bytes(s[2:4], 'big'), 'rate': word >> 44,
            'channels': ((word >> 41) & 7) + 1, 'bps': ((word >> 36) & 31) + 1, 'total': word & ((1 << 36) - 1), 'md5': bytes(s[18:34])}
    pos += 38
    while not last and pos + 4 <= len(data):
        last = data[pos] >> 7
        pos += 4 + int.from_bytes(data[pos + 1:pos + 4], 'big')
    info['audio_off'] = min(pos, len(data))
    if info['bps'] not in (8, 12, 16, 20, 24):
        raise Refused(f"{info['bps']}-bit samples")
    if info['max_block'] > 16384:
        raise Refused(f"maximum block size {info['max_block']}")
    return info


def read_header(d):
    """The frame header at the start of d: dict with 'len', or None."""
    if len(d) < 6 or d[0] != 0xff or d[1] & 0xfe != 0xf8:
        return None
    bs_code, rate_code, assign, size_code = d[2] >> 4, d[2] & 15, d[3] >> 4, (d[3] >> 1) & 7
    if bs_code == 0 or rate_code == 15 or assign > 10 or size_code in (3, 7) or d[3] & 1:
        return None
    b0 = d[4]
    ones = 0
    while ones < 8 and (b0 >> (7 - ones)) & 1:
        ones += 1
    if ones == 1 or ones == 8:
        return None
    extra = max(ones - 1, 0)
    v = b0 & (0xff >> (ones + 1)) if ones else b0
    variable = d[1] & 1
    if extra == 6 and not variable:
        return None
    pos = 5
    if pos + extra + 1 > len(d):
        return None
    for _ in range(extra):
        if d[pos] & 0xc0 != 0x80:
            return None
        v = (v << 6) | (d[pos] & 0x3f)
        pos += 1
    need = {6: 1, 7: 2}.get(bs_code, 0) + {12: 1, 13: 2, 14: 2}.get(rate_code, 0)
    if pos + need >= len(d):
        return None
    if bs_code == 1:
        block = 192
    elif bs_code <= 5:
        block = 576 << (bs_code - 2)
    elif bs_code == 6:
        block = d[pos] + 1
        pos += 1
    elif bs_code == 7:
        block = int.from_bytes(d[pos:pos + 2], 'big') + 1
        pos += 2
    else:
        block = 256 << (bs_code - 8)
    rate = [0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000, None, None, None][rate_code]
    if rate_code == 12:
        rate = d[pos] * 1000
        pos += 1
    elif rate_code >= 13:
        rate = int.from_bytes(d[pos:pos + 2], 'big') * (1 if rate_code == 13 else 10)
        pos += 2
    if crc8(d[:pos]) != d[pos]:
        return None
    return {'len': pos + 1, 'variable': variable, 'block': block, 'rate': rate, 'assign': assign, 'channels': assign + 1 if assign < 8 else 2,
            'bps': {0: 0, 1: 8, 2: 12, 4: 16, 5: 20, 6: 24}[size_code], 'number': v}


def read_frame(d, info, block=None):
    """One frame from the start of d: (samples (block, ch) int64, bytes used); _Fail(reason) for anything wrong."""
    h = read_header(d)
    if h is None:
        raise _Fail('header')
    if (block is not None and h['block'] != block) or h['channels'] != info['channels'] or h['bps'] not in (0, info['bps']) or \
            h['rate'] not in (0, info['rate']):
        raise _Fail('mismatch')
    n, bps, assign = h['block'], info['bps'], h['assign']
    r = _Reader(d)
    r.pos = 8 * h['len']
    chans = []
    for c in range(h['channels']):
        w = bps + (1 if (assign, c) in ((8, 1), (9, 0), (10, 1)) else 0)
        if r.u(1):
            raise _Fail('subframe padding bit')
        kind = r.u(6)
        wasted = r.unary() + 1 if r.u(1) else 0
        if wasted >= w:
            raise _Fail('wasted bits')
        w -= wasted
        if kind == 0:
            s = [r.s(w)] * n
        elif kind == 1:
            s = [r.s(w) for _ in range(n)]
        elif 8 <= kind <= 12 or kind >= 32:
            order = kind - 8 if kind <= 12 else kind - 31
            if order > n:
                raise _Fail('order above block size')
            s = [r.s(w) for _ in range(order)]
            if kind >= 32:
                precision = r.u(4) + 1
                if precision == 16:
                    raise _Fail('precision')
                shift = r.s(5)
                if shift < 0:
                    raise _Fail('negative shift')
                coefs = [r.s(precision) for _ in range(order)]
            else:
                coefs, shift = FIXED[order], 0
            method = r.u(2)
            if method > 1:
                raise _Fail('residual method')
            pb, esc = (5, 31) if method else (4, 15)
            po = r.u(4)
            if n % (1 << po) or (n >> po) < order:
                raise _Fail('partition order')
            for p in range(1 << po):
                cnt = (n >> po) - (order if p == 0 else 0)
                k = r.u(pb)
                nb = r.u(5) if k == esc else 0
                for _ in range(cnt):
                    if k == esc:
                        res = r.s(nb)
                    else:
                        q = r.unary()
                        if q > (0xffffffff >> k):
                            raise _Fail('unary run')
                        u = (q << k) | r.u(k)
                        res = (u >> 1) ^ -(u & 1)
                    pred = sum(cf * s[-1 - j] for j, cf in enumerate(coefs)) >> shift
                    pred = ((pred + (1 << 31)) & 0xffffffff) - (1 << 31)
                    s.append(((res + pred + (1 << 31)) & 0xffffffff) - (1 << 31))
        else:
            raise _Fail('reserved subframe type')
        chans.append(np.array(s, np.int64) << wasted)
    r.u(-r.pos % 8)
    stated = r.u(16)
    used = r.pos // 8
    if crc16(d[:used - 2]) != stated:
        raise _Fail('crc16')
    if assign == 8:
        chans = [chans[0], chans[0] - chans[1]]
    elif assign == 9:
        chans = [chans[0] + chans[1], chans[1]]
    elif assign == 10:
        m = (chans[0] << 1) | (chans[1] & 1)
        chans = [(m + chans[1]) >> 1, (m - chans[1]) >> 1]
    return np.stack(chans, 1), used


def read_index(data):
    """(info, [(offset, n_bytes, first sample as coded, block size)]): the chain of frame headers, as nafp_flac_index_host."""
    info = read_streaminfo(data)
    frames, pos, prev = [], info['audio_off'], None
    while pos + 6 <= len(data):
        h = read_header(data[pos:pos + 16]) if data[pos] == 0xff and data[pos + 1] & 0xfe == 0xf8 else None
        ok = h is not None and h['block'] <= info['max_block']
        if ok and prev is not None:
            if h['variable'] != prev['variable']:
                ok = False
            elif h['variable']:
                ok = h['number'] == prev['number'] + prev['block']
            else:
                ok = h['number'] == prev['number'] + 1 and prev['block'] == info['max_block']
        if not ok:
            pos += 1
            continue
        if frames:
            frames[-1][1] = pos - frames[-1][0]
        frames.append([pos, 0, h['number'] if h['variable'] else h['number'] * info['max_block'], h['block']])
        prev = h
        pos += h['len']
    if frames:
        frames[-1][1] = len(data) - frames[-1][0]
        try:
            read_frame(data[frames[-1][0]:], info, frames[-1][3])
        except _Fail as e:
            if str(e) == 'truncated':
                frames.pop()
    return info, [tuple(f) for f in frames]


def n_frames_of(info, frames):
    indexed = sum(f[3] for f in frames)
    return info['total'] if 0 < info['total'] <= indexed else indexed


def read_stream(data):
    """(info, frames, samples (n, ch) int64 with failed frames as zeros, [failed?])."""
    info, frames = read_index(data)
    out, failed = [], []
    for off, nb, _, block in frames:
        try:
            x, _ = read_frame(data[off:off + nb], info, block)
            failed.append(False)
        except _Fail:
            x = np.zeros((block, info['channels']), np.int64)
            failed.append(True)
        out.append(x)
    x = np.concatenate(out) if out else np.zeros((0, info['channels']), np.int64)
    return info, frames, x[:n_frames_of(info, frames)], failed


if __name__ == '__main__':
    import os
    streams = golden_streams()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'flac_streams_v1.bin')
    with open(path, 'wb') as fh:
        fh.write(b'NAFPFLAC' + struct.pack('<I', len(streams)) + b''.join(struct.pack('<I', len(s.data)) + s.data for s in streams))
    print(path, os.path.getsize(path), 'bytes,', len(streams), 'streams')
