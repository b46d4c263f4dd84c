"""The leaner forms of the forward pass outside the GEMM K-loops (NAFP_OPT_NONMATRIX, include/nafp.h) change no byte.

Every bit of the option selects another form of one part of the forward -- conv0 as straight-line code, the two-part
in-kernel split-K finish on the last arriver's own accumulators -- and the value 0 selects the earlier forms.  Both run
here in ONE process on the same inputs and are compared bit for bit
(int32 views, so that the NaN rows of a poisoned sample compare too): fingerprints, the flatten output, the per-layer
LayerNorm statistics (64-bit fixed point, read from the forward's workspace) and conv0's activation.
"""
import pytest
import torch

import _inputs

pytestmark = pytest.mark.gpu

OPT_NONMATRIX = 8                                  # include/nafp.h
CONV0, KEEP_OWN, ALL = 1, 2, 3
DEFAULT = ALL


class _Raw:
    """What the front end hands over with defer=True (melspectrogram.DeferredFeatures): raw log-mel + (max, min) per group."""

    def __init__(self, raw, group_size, segment_norm=False):
        B = raw.shape[0]
        groups = [raw[g:g + group_size] for g in range(0, B, group_size)]
        self.raw = raw
        self.gstat = torch.stack([torch.stack([x[torch.isfinite(x)].max(), x[torch.isfinite(x)].min()]) for x in groups]).contiguous()
        self.group_size, self.segment_norm = group_size, segment_norm


def _raw(B, seed, shape=(256, 32)):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return 8.0 * torch.rand((B,) + shape + (1,), generator=g, device='cuda') - 6.0      # log10-mel of the front end: about -6 .. 2


@pytest.fixture(scope='module')
def model(nafp):
    m = nafp.FingerPrinter(seed=0)
    m.set_weights(_inputs.weight_list(_inputs.weights(seed=7)))
    return m


def _bits(t):
    return t.contiguous().view(torch.int32)


def _layer_stats(m, B):
    """(16, B, 2) int64: the statistics every layer left in the workspace of the current stream (api.hip: they lead it)."""
    ws = m._ws[torch.cuda.current_stream(m.device).cuda_stream]
    off = (-ws.data_ptr()) % 256
    st = ws[off:off + 16 * 2 * 8 * B].view(torch.int64).reshape(16, B, 2).clone()
    # ... which pins that layout: sums of squares are positive in every layer, layers differ, and layer 0 is what conv0 alone gives
    assert bool((st[:, :, 1] > 0).all()) and all(not torch.equal(st[j], st[j + 1]) for j in range(15))
    return st


def _forward(m, mask, feat):
    m.set_option(OPT_NONMATRIX, mask)
    try:
        flat, emb = m._forward(feat, True, True)
        B = emb.shape[0]
        torch.cuda.synchronize()
        return _bits(emb).clone(), _bits(flat).clone(), _layer_stats(m, B)
    finally:
        m.set_option(OPT_NONMATRIX, DEFAULT)


@pytest.mark.parametrize('B', [1, 9, 13, 640])
def test_whole_forward(model, B, mask=ALL):
    """The raw-feature entry with groups of 5 (ragged last group) at one ragged sample group of 8, one full + one ragged, and two
    groups with one ragged; 640: the bench launch, every compute unit shared by several workgroups."""
    feat = _Raw(_raw(B, 40 + B), 5)
    emb0, flat0, st0 = _forward(model, 0, feat)
    assert bool(torch.isfinite(emb0.view(torch.float32)).all())
    emb1, flat1, st1 = _forward(model, mask, feat)
    assert torch.equal(emb1, emb0) and torch.equal(flat1, flat0)
    assert torch.equal(st0[0], _conv0(model, 0, feat.raw.contiguous(), feat.gstat, 5, False)[1])      # the workspace view is the statistics
    for j in range(16):
        assert torch.equal(st1[j], st0[j]), f'statistics of layer {j}'


@pytest.mark.parametrize('B', [9, 640])
def test_keep_own_part(model, B):
    """Convs 7 and 9 (two parts, finished in-kernel).  At 640 every tile has two live arrivers in varying order: three runs, all
    equal to the earlier form."""
    feat = _Raw(_raw(B, 7 + B), 5)
    emb0, _, st0 = _forward(model, 0, feat)
    for run in range(3):
        emb1, _, st1 = _forward(model, KEEP_OWN, feat)
        assert torch.equal(emb1, emb0), run
        assert torch.equal(st1[7], st0[7]) and torch.equal(st1[9], st0[9]), run
    # the arrival counters are back at zero: the earlier form, which counts on that, still gives the same
    emb2, _, st2 = _forward(model, 0, feat)
    assert torch.equal(emb2, emb0) and torch.equal(st2, st0)


def test_whole_forward_with_a_nan_sample(model):
    """A NaN sample: its row stays NaN in both forms, the statistics carry the same poison, the other rows keep their bytes."""
    raw = _raw(9, 99)
    raw[4, 100, 7, 0] = float('nan')
    feat = _Raw(raw, 5)
    emb0, flat0, st0 = _forward(model, 0, feat)
    emb1, flat1, st1 = _forward(model, ALL, feat)
    assert bool(torch.isnan(emb1.view(torch.float32)[4]).all()) and bool(torch.isnan(flat1.view(torch.float32)[4]).all())
    assert torch.equal(emb1, emb0) and torch.equal(flat1, flat0) and torch.equal(st1, st0)


def _conv0(m, mask, feat, gstat, group_size, segment_norm):
    from neural_audio_fp_amd import _lib
    m._sync()
    B = feat.shape[0]
    n = int(m._lib.nafp_encoder_conv0_numel(m._h))
    z = torch.full((B, n), float('nan'), device='cuda')
    st = torch.full((B, 2), -1, dtype=torch.int64, device='cuda')
    m.set_option(OPT_NONMATRIX, mask)
    try:
        with torch.cuda.device(feat.device):
            _lib.check(m._lib.nafp_encoder_conv0(m._h, _lib.ptr(feat), _lib.ptr(gstat), group_size, int(segment_norm), B,
                                                 _lib.ptr(z), _lib.ptr(st), _lib.current_stream()), 'encoder_conv0')
        torch.cuda.synchronize()
    finally:
        m.set_option(OPT_NONMATRIX, DEFAULT)
    return _bits(z), st


@pytest.mark.parametrize('B', [3, 40])
@pytest.mark.parametrize('how', ['finished', 'raw', 'raw_segment_norm'])
def test_conv0(model, how, B):
    """z0 and the layer-0 statistics at B = 3 (groups of 2: a ragged one), without and with the deferred tail of the log-mel layer.
    B = 40: 640 workgroups, so that most of them start on a compute unit that is already running others -- a hazard between a
    store and the next write of its data registers shows only there (it did, with 16-byte buffer stores: conv.hip)."""
    raw = _raw(B, 5)
    d = _Raw(raw, 2, how == 'raw_segment_norm')
    feat = raw.contiguous()
    gstat = None if how == 'finished' else d.gstat
    z0, s0 = _conv0(model, 0, feat, gstat, 2, d.segment_norm)
    z1, s1 = _conv0(model, CONV0, feat, gstat, 2, d.segment_norm)
    assert bool(torch.isfinite(z0.view(torch.float32)).all()) and bool((s0[:, 1] > 0).all())
    assert torch.equal(z1, z0) and torch.equal(s1, s0)


def test_conv0_nan_sample(model):
    raw = _raw(3, 6)
    raw[1, 17, 31, 0] = float('nan')                # the last frame: taps of the last two output frames
    d = _Raw(raw, 2)
    z0, s0 = _conv0(model, 0, raw.contiguous(), d.gstat, 2, False)
    z1, s1 = _conv0(model, CONV0, raw.contiguous(), d.gstat, 2, False)
    assert int(s0[1, 1]) >> 62 == 1 and bool(torch.isnan(z0.view(torch.float32)[1]).any())
    assert torch.equal(z1, z0) and torch.equal(s1, s0)


def test_conv0_ragged_geometry(nafp):
    """A (248, 62) input: 31 output frames (a thread's positions wrap around the row at uneven places), 496 positions per full
    workgroup (fifteen whole batches of 32 and a ragged one) and a last workgroup of 8 rows."""
    m = nafp.FingerPrinter(input_shape=(248, 62, 1), seed=1)
    g = torch.Generator(device='cuda').manual_seed(3)
    m._vars[1].copy_(0.2 * torch.rand(m._vars[1].shape, generator=g, device='cuda') - 0.1)     # conv0 bias
    m._vars[2].copy_(torch.rand(m._vars[2].shape, generator=g, device='cuda') + 0.5)           # ln0 gamma
    m.mark_dirty()
    raw = _raw(3, 8, shape=(248, 62))
    d = _Raw(raw, 2, True)
    z0, s0 = _conv0(m, 0, raw.contiguous(), d.gstat, 2, True)
    z1, s1 = _conv0(m, CONV0, raw.contiguous(), d.gstat, 2, True)
    assert bool(torch.isfinite(z0.view(torch.float32)).all())
    assert torch.equal(z1, z0) and torch.equal(s1, s0)
