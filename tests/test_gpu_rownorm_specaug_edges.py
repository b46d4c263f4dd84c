"""GPU: nafp_l2_normalize_rows (csrc/tail.hip) and the spec-augment kernels (csrc/specaug.hip) through the C entry points, at their edges.

nafp_l2_normalize_rows against x / sqrt(max(sum x^2, 1e-12)) in float64, 16U relative per element (U = 2^-24) for dim <= 1024.  Count
from l2_normalize_rows_kernel: a lane fuses at most dim / 64 = 16 squares into its sum and the wave sum adds 6 levels: 22 additions of
non-negative terms, 0.5U each = 11U on the sum, 5.5U after the root; the clamp constant 1e-12f is 0.2U off 1e-12 (0.1U after the root);
rsqrtf is good to 1 ulp = 2U at worst; the product rounds once (0.5U): 8.1U < 16U.  A row scaled by a power of two gives the scaled
sum, the scaled inverse root and the same products: the same bits, while its sum of squares stays above the clamp.

nafp_specaug_range is exact: {max - min formed in float32, min}, bit for bit; its grid-stride loop wraps at 256 x 256 = 65536 elements.
nafp_specaug_mean: on lattice inputs (multiples of 1/8 in [-80, 0]) every float4 sum and every double sum is exact, so the result
is float32(sum / n) bit for bit; on 1000 + noise the float4 sums round (two sums of two at 0.5 ulp(2048), one of four at 0.5 ulp(4096),
per 4 elements: 2U mean|x|) and the result rounds once (0.5U |mean|): bound 2U mean|x| + U |mean|, which an all-float32 sum misses.
The two masking kernels bit for bit against oracle.specaug, including the second trip of their grid-stride loop (grid capped at 2048
workgroups: n_vec4 > 524288, B > 256 at (256, 32)) that every real training batch takes.

OBSERVED ON THE MI355X:
  nafp_l2_normalize_rows: 2.68U of 16U (dim 64, 1001 rows); nafp_specaug_mean on 1000 + noise: 0.16 of its bound; everything else
  is an exact comparison and holds.
"""
import numpy as np
import pytest
import torch

from oracle import specaug as o_sa

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope='module')
def lib(nafp):
    return nafp._lib.load()


@pytest.fixture(scope='module')
def call(nafp, lib):
    """call(name, *args): torch tensors become device pointers, the current stream is appended, the status must be OK."""
    def run(name, *args, expect=0):
        conv = [nafp._lib.ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
        assert getattr(lib, name)(*conv, nafp._lib.current_stream()) == expect, name
        torch.cuda.synchronize()
    return run


# ---------------------------------------------------------------- nafp_l2_normalize_rows ----------------------------------------------------------------
ROW_KINDS = ['normal', 'zero', 'below', 'above', 'big', 'small']


def _row(kind, dim, rng):
    x = rng.normal(size=dim)
    if kind == 'zero':
        x[:] = 0
    elif kind == 'below':                     # sum of squares below the clamp (dim x 1e-16 <= 1.1e-13): the row comes out as x * 1e6
        x[:] = 1e-8
    elif kind == 'above':                     # just above it: sum = 1.1e-12
        x[:] = np.sqrt(1.1e-12 / dim)
    elif kind == 'big':
        x *= 1e15
    elif kind == 'small':
        x *= 1e-15
    return x.astype(np.float32)


def _l2_reference(x):
    x64 = x.astype(np.float64)
    return x64 / np.sqrt(np.maximum((x64 * x64).sum(1, keepdims=True), 1e-12))


@pytest.mark.parametrize('n_rows', [1, 3, 4, 5, 1001])
@pytest.mark.parametrize('dim', [1, 3, 63, 64, 65, 128, 200, 256, 1024])
def test_l2_normalize_rows(call, observe, dim, n_rows):
    rng = np.random.default_rng(1000 * dim + n_rows)
    kinds = [ROW_KINDS[(i + dim + n_rows) % len(ROW_KINDS)] for i in range(n_rows)]        # every kind at every dim; all of them at 1001 rows
    x = np.stack([_row(k, dim, rng) for k in kinds])
    out = torch.full((n_rows + 1, dim), 777.0, device='cuda')                                # one spare row behind the last
    call('nafp_l2_normalize_rows', _dev(x), n_rows, dim, out)
    y = out.cpu().numpy()
    assert (y[n_rows] == 777.0).all() and np.isfinite(y).all()
    y, want = y[:n_rows], _l2_reference(x)
    zero = np.array([k == 'zero' for k in kinds])
    assert (y[zero] == 0).all()                                                              # zeros, no NaN
    below = np.array([k == 'below' for k in kinds])
    assert np.allclose(want[below], x[below].astype(np.float64) * 1e6, rtol=1e-12, atol=0)   # (what the reference says of such a row)
    nz = want != 0
    observe('relative error [U]', (np.abs(y - want)[nz] / np.abs(want[nz])).max() / U if nz.any() else 0.0, 16.0)
    assert (y[~nz] == 0).all()


@pytest.mark.parametrize('dim', [1, 3, 64, 65, 200, 1024])
def test_l2_normalize_rows_power_of_two_scaling(call, dim):
    rng = np.random.default_rng(dim)
    base = (rng.uniform(0.5, 2.0, dim) * np.where(rng.random(dim) < 0.5, -1, 1)).astype(np.float32)
    x = np.stack([base * np.float32(2.0 ** k) for k in (0, -8, 5, 40)])                     # sum of squares >= 2^-18 > 1e-12 at every scale
    out = torch.empty((4, dim), device='cuda')
    call('nafp_l2_normalize_rows', _dev(x), 4, dim, out)
    y = _bits(out.cpu().numpy())
    assert all(np.array_equal(y[0], y[k]) for k in (1, 2, 3))


# ---------------------------------------------------------------- nafp_specaug_range ----------------------------------------------------------------
@pytest.fixture(scope='module')
def ws(lib):
    return torch.zeros((int(lib.nafp_specaug_mean_workspace_bytes()),), dtype=torch.uint8, device='cuda')


def _range(call, ws, x_dev, n):
    out = torch.full((3,), 99.0, device='cuda')
    call('nafp_specaug_range', x_dev, n, out, ws, ws.numel())
    got = out.cpu().numpy()
    assert got[2] == 99.0
    return got[:2]


@pytest.mark.parametrize('n', [1, 2, 255, 256, 257, 65535, 65536, 65537, 70001])
def test_specaug_range_is_exact(call, ws, n):
    rng = np.random.default_rng(n)
    base = rng.uniform(0.001, 1.0, n).astype(np.float32) * np.where(rng.random(n) < 0.5, -1, 1).astype(np.float32)   # no zero of either sign
    lo_v, hi_v = np.float32(-7.3), np.float32(5.1)
    for pos in sorted({p for p in (0, n - 1, 65535, 65536, n - 2) if 0 <= p < n}):
        for swap in (False, True):
            x = base.copy()
            other = (pos + n // 2) % n
            a, b = (other, pos) if swap else (pos, other)
            x[a] = hi_v                                       # the maximum at `a`; the minimum at `b` (n == 1: one value is both)
            x[b] = lo_v
            want = np.array([x.max() - x.min(), x.min()], np.float32)                        # float32 arithmetic
            assert np.array_equal(_bits(_range(call, ws, _dev(x), n)), _bits(want)), (n, pos, swap)
    x = np.full(n, 1.25, np.float32)                                                          # all equal: scale +0
    assert np.array_equal(_bits(_range(call, ws, _dev(x), n)), _bits(np.array([0.0, 1.25], np.float32)))
    x = -np.abs(base) - np.float32(3.0)                                                       # all negative
    assert np.array_equal(_bits(_range(call, ws, _dev(x), n)), _bits(np.array([x.max() - x.min(), x.min()], np.float32)))
    buf = _dev(np.concatenate([np.array([1e9], np.float32), base]))                           # 4 bytes into an allocation: scalar loads
    assert buf[1:].data_ptr() % 16 == 4
    assert np.array_equal(_bits(_range(call, ws, buf[1:], n)), _bits(np.array([base.max() - base.min(), base.min()], np.float32)))


# ---------------------------------------------------------------- nafp_specaug_mean ----------------------------------------------------------------
def _mean(call, ws, x):
    out = torch.full((2,), 99.0, device='cuda')
    xd = _dev(x)
    assert xd.data_ptr() % 16 == 0
    call('nafp_specaug_mean', xd, x.size, out, ws, ws.numel())
    first = out.cpu().numpy().copy()
    call('nafp_specaug_mean', xd, x.size, out, ws, ws.numel())                                # the same workspace again
    assert np.array_equal(_bits(first), _bits(out.cpu().numpy())) and first[1] == 99.0
    return first[0]


@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 7, 1023, 1024, 1027, 65539, 5 * 256 * 32])
def test_specaug_mean_is_exact_on_a_lattice(call, ws, n):
    x = (np.random.default_rng(n).integers(-640, 1, n) / 8.0).astype(np.float32)
    want = np.float32(x.astype(np.float64).sum() / n)
    assert _bits(_mean(call, ws, x)) == _bits(want), (n, want)


def test_specaug_mean_accumulates_in_double(call, ws, observe):
    n = 40960
    x = (1000.0 + np.random.default_rng(7).normal(size=n)).astype(np.float32)
    want = x.astype(np.float64).mean()
    bound = 2 * U * np.abs(x.astype(np.float64)).mean() + U * abs(want)
    observe('error of the mean [bound]', abs(float(_mean(call, ws, x)) - want) / bound, 1.0)
    f32_sum = np.float32(0)
    for v in x[:n]:                                                                           # what an all-float32 accumulation would give
        f32_sum += v
    assert abs(float(f32_sum / np.float32(n)) - want) > bound


# ---------------------------------------------------------------- the masking kernels ----------------------------------------------------------------
def _rect_sets(F, T, rng, n_max):
    """Rectangle sets inside (F, T): edges inside a float4 quad (t0 % 4, t1 % 4 in 1..3), one element, everything, two overlapping,
    and exactly n_max random ones."""
    rand = []
    for _ in range(n_max):
        f0, t0 = int(rng.integers(0, F)), int(rng.integers(0, T))
        rand.append((f0, int(rng.integers(f0, F)), t0, int(rng.integers(t0, T))))
    return {'quad_edges': [(0, F - 1, 1, T - 2), (F // 2, F // 2, T - 3, T - 1)],
            'one_element': [(F - 1, F - 1, T - 3, T - 3)],
            'everything': [(0, F - 1, 0, T - 1)],
            'overlapping': [(0, F // 2, 0, T // 2), (F // 3, F - 1, T // 4 + 1, T - 1)],
            'full_table': rand}


def _uniform(nafp, call, x, rects, active, fill, fill_dev=False):
    xd = _dev(x)
    r = (nafp._lib.Rect * max(1, len(rects)))(*[nafp._lib.Rect(*q) for q in rects])
    B, F, T = x.shape[:3]
    act = None if active is None else _dev(np.asarray(active, np.uint8))
    if fill_dev:
        call('nafp_specaug_apply_fill_dev', xd, B, F, T, r, len(rects), act, _dev(np.array([fill], np.float32)))
    else:
        call('nafp_specaug_apply', xd, B, F, T, r, len(rects), act, float(fill))
    return xd.cpu().numpy()


def _general(call, x, rects, active, filler, scale, offset):
    xd = _dev(x)
    B, F, T = x.shape[:3]
    r = np.ascontiguousarray(rects, np.int32)
    n_rects = r.shape[-2]
    act = None if active is None else _dev(np.ascontiguousarray(active, np.uint8).reshape(B, n_rects))
    fd = None if filler is None else _dev(np.ascontiguousarray(filler, np.float32))
    call('nafp_specaug_apply_ex', xd, B, F, T, _dev(r), n_rects, 1 if r.ndim == 2 else B, act, fd, 0 if filler is None else len(filler),
         _dev(np.array([scale, offset], np.float32)))
    return xd.cpu().numpy()


@pytest.mark.parametrize('F,T', [(1, 4), (3, 8), (5, 12), (256, 32)])
def test_masking_small_geometries(nafp, call, F, T):
    rng = np.random.default_rng(F * 100 + T)
    B = 3
    x = rng.normal(size=(B, F, T, 1)).astype(np.float32)
    for name, rects in _rect_sets(F, T, rng, 8).items():
        for active in (None, [1, 0, 1]):
            got = _uniform(nafp, call, x, rects, active, -0.5)
            assert np.array_equal(_bits(got), _bits(o_sa.apply_holes(x, rects, active, -0.5))), (name, active)
    filler = rng.random((2, F, T)).astype(np.float32)                                         # fewer rows than the batch
    for name, rects in _rect_sets(F, T, rng, 32).items():
        n = len(rects)
        for active in (None, rng.random((B, n)) < 0.6):
            got = _general(call, x, rects, active, filler, 1.75, -0.3)
            want = o_sa.apply_holes_general(x, np.array(rects), active, filler, 1.75, -0.3)
            assert np.array_equal(_bits(got), _bits(want)), (name, 'shared set')
        per_sample = np.stack([np.roll(np.array(rects), b, axis=0) for b in range(B)])        # a set per sample: the same holes, permuted
        act = rng.random((B, n)) < 0.6
        got = _general(call, x, per_sample, act, None, 0.25, -1.0)
        assert np.array_equal(_bits(got), _bits(o_sa.apply_holes_general(x, per_sample, act, None, 0.25, -1.0))), (name, 'set per sample')


@pytest.fixture(scope='module')
def batch300():
    """B = 300 at (256, 32): n_vec4 = 614400 > 2048 x 256, so samples b >= 256 belong to the second trip of the grid-stride loop."""
    rng = np.random.default_rng(300)
    x = rng.normal(size=(300, 256, 32, 1)).astype(np.float32)
    x.setflags(write=False)
    return x


def test_masking_second_trip_uniform(nafp, call, batch300):
    x, rng = batch300, np.random.default_rng(301)
    active = np.zeros(300, np.uint8)
    active[:256] = rng.random(256) < 0.5
    active[256:] = 1 - active[:44]                                                             # other flags where the loop wraps
    active[299] = 1
    rects = [(10, 80, 3, 9), (200, 212, 0, 31), (255, 255, 29, 31), (0, 0, 1, 2)]
    want = o_sa.apply_holes(x, rects, active, -0.5).astype(np.float32)
    assert (want[256:] != x[256:]).any() and (want[:256] != x[:256]).any()
    assert np.array_equal(_bits(_uniform(nafp, call, x, rects, active, -0.5)), _bits(want))
    assert np.array_equal(_bits(_uniform(nafp, call, x, rects, active, -0.5, fill_dev=True)), _bits(want))      # the fill value read on the device
    assert np.array_equal(_bits(_uniform(nafp, call, x, rects, None, 0.0)), _bits(o_sa.apply_holes(x, rects, None, 0.0)))


def test_masking_second_trip_general(call, batch300):
    x, rng = batch300, np.random.default_rng(302)
    rects = np.zeros((300, 3, 4), np.int32)
    for b in range(300):
        lo = 0 if b < 256 else 128                                                             # other holes where the loop wraps
        for k in range(3):
            f0, t0 = int(rng.integers(lo, lo + 100)), int(rng.integers(0, 28))
            rects[b, k] = (f0, f0 + int(rng.integers(0, 28)), t0, t0 + int(rng.integers(0, 4)))
    act = rng.random((300, 3)) < 0.6
    act[256:] = ~act[:44]
    act[299] = True
    filler = rng.random((7, 256, 32)).astype(np.float32)                                       # row b % 7
    want = o_sa.apply_holes_general(x, rects, act, filler, 1.5, -0.25)
    assert (want[256:] != x[256:]).any()
    assert np.array_equal(_bits(_general(call, x, rects, act, filler, 1.5, -0.25)), _bits(want))


def test_masking_nothing_to_do(nafp, call):
    """n_rects == 0 and n_seg == 0 return OK and leave the data untouched (real buffers throughout)."""
    x = np.random.default_rng(9).normal(size=(2, 3, 8, 1)).astype(np.float32)
    xd, so, rd = _dev(x), _dev(np.array([2.0, 1.0], np.float32)), _dev(np.array([[0, 2, 0, 7]], np.int32))
    r = (nafp._lib.Rect * 1)(nafp._lib.Rect(0, 2, 0, 7))
    call('nafp_specaug_apply', xd, 2, 3, 8, None, 0, None, 5.0)
    call('nafp_specaug_apply', xd, 0, 3, 8, r, 1, None, 5.0)
    call('nafp_specaug_apply_fill_dev', xd, 2, 3, 8, None, 0, None, so)
    call('nafp_specaug_apply_ex', xd, 2, 3, 8, None, 0, 1, None, None, 0, so)
    call('nafp_specaug_apply_ex', xd, 0, 3, 8, rd, 1, 1, None, None, 0, so)
    call('nafp_specaug_apply_ex', xd, 0, 3, 8, rd, 1, 0, None, None, 0, so)                    # n_sets == n_seg == 0
    assert np.array_equal(_bits(xd.cpu().numpy()), _bits(x))
