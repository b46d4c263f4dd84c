"""GPU: nafp_triplet_forward at its edges, through the C entry point: pairs with 2(1 - dot) <= 0 (duplicate rows, rows of norm
above 1), dims other than 64 / 128, one replica, one anchor, more columns than one pass of the 256 threads, the n_anchor + n_pos =
8192 limit, every combination of the optional outputs, and a second call on the same workspace.

The inputs are LATTICE rows: every entry is 0, +-1/8 or +-1/4, so every product is a multiple of 1/64, every dot product is exact
in float32 in any summation order, d2 = 2(1 - dot) is exact, and the kernel and the float64 oracle see the same sign of d2 and the
same mask [d2 > 0] everywhere.  That is what lets the distances be held WITHOUT an exemption near zero:
    dd = sqrtf(fl(d2 + fl(1e-9)))    one rounding of the sum (2^-24), the float32 value of 1e-9 (2^-24 of it, and it is at most
                                     the whole radicand), halved by the root, plus one rounding of the root (2^-24): <= 2^-23,
held to 2^-22 relative.  The loss and the gradients keep the bounds of tests/test_gpu_triplet.py (2e-6 relative; 2e-4 * scale +
1e-9 against the float64 autograd of oracle.triplet.torch_loss, whose gradient through sqrt(d2 * [d2 > 0] + 1e-9) is 0 where
d2 <= 0).  The replicas of an anchor sit at pairwise different distances from it, so the hardest positive is unique (which of
several equal maxima reduce_max hands the gradient to is not this file's subject), and its smallest distance differs from anchor to
anchor: the loss is one float32 atomic per anchor, whose worst case of n_anchor * 2^-25 relative is reached only by equal terms.

Before the mask [d2 > 0] was carried from d2 itself, the duplicate cases missed the gradient bound in modes 0, 1 and 2 (and in mode
3 where the only replica equals its anchor) with errors of 27 to 659 against gradients of at most 0.09."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import triplet as T

pytestmark = pytest.mark.gpu

MODES = {0: 'semi-hard', 1: 'all', 2: 'all-balanced', 3: 'hardest'}
# margins at which the hinge of every mode has active AND inactive terms on these inputs (positives at 0.25 .. 0.97, unrelated rows near
# sqrt(2)): semi-hard max(hardest - d + m, 0), all max(+-d + m, 0), all-balanced max(mean_pos - mean_neg + m, 0), hardest max(max_pos + m, 0)
MARGIN = {0: 0.8, 1: 0.25, 2: 1.0, 3: 0.1}
DIST_REL = 2.0 ** -22


def _anchors(rng, n, d):
    """n rows with min(d, 64) non-zero entries at random places: +-1/8 (norm exactly 1) for d >= 64, +-1/4 below."""
    nz, amp = min(d, 64), (0.125 if d >= 64 else 0.25)
    a = np.zeros((n, d))
    where = np.argsort(rng.random((n, d)), axis=1)[:, :nz]
    np.put_along_axis(a, where, rng.choice([-amp, amp], size=(n, nz)), axis=1)
    return a


def _replicas(rng, a, npa):
    """replica k of an anchor = the anchor with j_k of its non-zero entries set to 0, the j_k of one anchor pairwise different:
    dot(anchor, replica) = |anchor|^2 - (what was removed), so the replicas lie at pairwise different distances.  The smallest j
    differs from anchor to anchor, so the anchors do not all contribute the same term to the loss."""
    n, d = a.shape
    nz = min(d, 64)
    p = np.repeat(a, npa, axis=0)
    for i in range(n):
        support = np.flatnonzero(a[i])
        base = rng.integers(2, 7)
        for k, r in enumerate(rng.permutation(npa)):
            j = base + 4 * r if nz >= 64 else 1 + r
            assert j < nz
            p[i * npa + k, rng.permutation(support)[:j]] = 0.0
    return p


def _inputs(nA, npa, d, seed, kind=None):
    rng = np.random.default_rng(seed)
    a = _anchors(rng, nA, d)
    if kind == 'two equal anchors':
        a[1] = a[0]                                            # row 0 x column nP + 1 (a negative): d2 = 0
    if kind == 'rows of norm above 1':
        a[0, np.flatnonzero(a[0])[0]] *= 2.0                   # |a0|^2 = 1 + 3/64 (less than one step between two replicas)
        a[1] = a[0]                                            # a negative with dot > 1: d2 < 0
    p = _replicas(rng, a, npa)
    if kind == 'a replica equal to its anchor':
        p[1] = a[0]                                            # a positive of anchor 0 with d2 = 0
    if kind == 'the only replica equal to its anchor':
        assert npa == 1
        p[0] = a[0]                                            # ... which is then the hardest positive as well
    if kind == 'a replica of one anchor equal to another anchor':
        p[2 * npa] = a[3]                                      # a negative of anchor 3 with d2 = 0 (and the far, hardest positive of anchor 2)
    if kind == 'rows of norm above 1':
        p[0] = a[0]                                            # a positive with dot > 1 (p[0] is not the hardest: d2 < 0)
    a, p = a.astype(np.float32), p.astype(np.float32)
    assert np.array_equal(a * 8, np.round(a * 8)) and np.array_equal(p * 8, np.round(p * 8)) and max(np.abs(a).max(), np.abs(p).max()) <= 0.25
    wd = T.pairwise_dist(a.astype(np.float64), p.astype(np.float64))
    for i in range(nA):                                        # the hardest positive of every anchor is unique
        own = np.sort(wd[i, i * npa:(i + 1) * npa])
        assert npa == 1 or own[-1] > own[-2]
    return a, p, wd


def _d2(a, p):
    return 2.0 * (1 - a.astype(np.float64) @ np.concatenate([p, a]).astype(np.float64).T)


def _run(lib, a, p, mode, margin, want_dist=True, want_grad=True, ws=None):
    """one call of the entry point; every output starts as NaN, the workspace as 0xFF bytes (NaN as floats)."""
    nA, d = a.shape
    nP = p.shape[0]
    ta, tp = torch.from_numpy(a).cuda(), torch.from_numpy(p).cuda()
    nan = float('nan')
    loss = torch.full((1,), nan, device='cuda')
    dist = torch.full((nA, nP + nA), nan, device='cuda') if want_dist else None
    da = torch.full((nA, d), nan, device='cuda') if want_grad else None
    dp = torch.full((nP, d), nan, device='cuda') if want_grad else None
    need = int(lib.nafp_triplet_workspace_bytes(nA, nP))
    assert need == nA * (nP + nA) * 4 + 256
    if ws is None:
        ws = torch.full((need,), 255, dtype=torch.uint8, device='cuda')
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = lib.nafp_triplet_forward(ptr(ta), ptr(tp), nA, nP, d, mode, float(margin), ptr(loss), ptr(dist), ptr(da), ptr(dp), ptr(ws),
                                  need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, st
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return float(loss[0]), host(dist), host(da), host(dp), ws


def _reference(a, p, mode, margin):
    ta = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tp = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    wl = T.torch_loss(ta, tp, MODES[mode], margin)
    wl.backward()
    return wl.item(), ta.grad.numpy(), tp.grad.numpy()


def _check(lib, a, p, wd, mode, what=''):
    margin = MARGIN[mode]
    loss, dist, da, dp, _ = _run(lib, a, p, mode, margin)
    wl, wda, wdp = _reference(a, p, mode, margin)
    assert abs(wl - T.compute_loss(a, p, MODES[mode], margin)[0]) < 1e-12 * max(1.0, abs(wl))        # the two restatements agree
    rel = (np.abs(dist - wd) / wd).max()
    scale = max(np.abs(wda).max(), np.abs(wdp).max(), 1e-12)
    ga, gp = np.abs(da - wda).max(), np.abs(dp - wdp).max()
    print(f'{what} mode {mode}: dist rel {rel:.3e} (bound {DIST_REL:.3e}), loss {loss:.9g} vs {wl:.9g}, '
          f'grad err {max(ga, gp):.3e} (scale {scale:.3e}, bound {2e-4 * scale + 1e-9:.3e})')
    assert rel <= DIST_REL
    assert abs(loss - wl) < 2e-6 * max(1.0, abs(wl))
    assert ga < 2e-4 * scale + 1e-9 and gp < 2e-4 * scale + 1e-9
    return loss, dist, da, dp


@pytest.fixture(scope='module')
def lib(nafp):
    return nafp._lib.load()


KINDS = [('a replica equal to its anchor', 3), ('two equal anchors', 3), ('a replica of one anchor equal to another anchor', 3),
         ('rows of norm above 1', 3), ('the only replica equal to its anchor', 1)]


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
@pytest.mark.parametrize('kind,npa', KINDS)
def test_zero_and_negative_d2(lib, kind, npa, mode):
    """the mask [d2 > 0] of the gradient where d2 is 0 or negative: the coefficient of such a pair is 0, not 1 / sqrt(1e-9)."""
    a, p, wd = _inputs(6, npa, 64, 11, kind)
    d2 = _d2(a, p)
    off_diag = np.ones_like(d2, bool)
    off_diag[np.arange(6), 6 * npa + np.arange(6)] = False
    assert (d2[off_diag] <= 0).any()                           # beside the anchors' own columns
    assert (d2 < 0).any() == (kind == 'rows of norm above 1')
    _check(lib, a, p, wd, mode, kind)


SHAPES = [(5, 3, 4), (5, 3, 100), (5, 3, 256), (6, 1, 64), (1, 5, 64), (300, 1, 64)]


@pytest.mark.parametrize('nA,npa,d,mode', [s + (m,) for s in SHAPES for m in (0, 1, 2, 3) if not (s[0] == 1 and m == 2)])
def test_dims_and_shapes(lib, nA, npa, d, mode):
    """d = 4 / 100 / 256; one replica; one anchor (all-balanced has no negatives there and is refused: tests/test_small_kernels_host.py);
    600 columns = two full passes of the 256 threads and a ragged third."""
    a, p, wd = _inputs(nA, npa, d, 100 * nA + d)
    _check(lib, a, p, wd, mode, f'{nA}x{npa} d{d}')


@pytest.fixture(scope='module')
def limit_case():
    return _inputs(1024, 7, 64, 8192)


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
def test_the_limit_of_8192_columns(lib, limit_case, mode):
    a, p, wd = limit_case
    assert len(a) + len(p) == 8192
    _check(lib, a, p, wd, mode, 'M = 8192')


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
def test_output_combinations_and_repetition(lib, mode):
    """distances and gradients asked for together == asked for separately, bit for bit; a second call on the same (now used)
    workspace reproduces them.  The loss is a sum of one float atomic per anchor: two orders of n terms of one sign differ by at
    most 2 (n - 1) 2^-24 of the sum."""
    a, p, wd = _inputs(7, 3, 64, 21, 'two equal anchors')
    margin = MARGIN[mode]
    loss_tol = lambda l: 2 * (len(a) - 1) * 2.0 ** -24 * abs(l)
    loss, dist, da, dp, ws = _run(lib, a, p, mode, margin)
    l_d, dist_d, _, _, _ = _run(lib, a, p, mode, margin, want_grad=False)
    l_g, _, da_g, dp_g, _ = _run(lib, a, p, mode, margin, want_dist=False)
    l_n, _, _, _, _ = _run(lib, a, p, mode, margin, want_dist=False, want_grad=False)
    assert np.array_equal(dist, dist_d) and np.array_equal(da, da_g) and np.array_equal(dp, dp_g)
    assert not np.isnan(dist).any() and not np.isnan(da).any() and not np.isnan(dp).any()
    assert max(abs(l_d - loss), abs(l_g - loss), abs(l_n - loss)) <= loss_tol(loss)
    l2, dist2, da2, dp2, _ = _run(lib, a, p, mode, margin, ws=ws)
    assert np.array_equal(dist2, dist) and np.array_equal(da2, da) and np.array_equal(dp2, dp)
    assert abs(l2 - loss) <= loss_tol(loss)
