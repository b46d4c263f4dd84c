"""GPU: the three IVF-PQ scans (csrc/ivf.hip ivf_pq_scan_kernel / ivf_pq_scan_f16_kernel / ivf_pq_scan_wide_kernel) pinned to
the bytes they put out: SHA-256 digests of the raw D and I of fixed searches against tests/golden/ivf_scan_digests_v1.json.  The
table fill, the split of a list into parts, the row loop and the 64-lookup sum are shared by the three kernels; a change to any of
them that moves one bit of one distance, or one id at a tie, shows here.  A digest that differs is a defect in the change: the
golden file is not re-recorded for it.

Inputs are seeded numpy arrays handed to `set_params` (no training on the GPU): nlist = nprobe = 8, 6 000 rows placed around 8
well-separated centres so that one list is empty, one holds 11 rows and one 1 300 (five trips of the 256-row loop and a ragged
sixth).  Every query probes every list.  With 3 queries a list is cut into dozens of parts (most parts of the short list are
empty); with 300 queries into one."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ivf_scan_digests_v1.json')
NLIST = 8
LIST_ROWS = (0, 11, 1300, 700, 1025, 937, 1100, 927)         # rows per list: 6 000 in all
DIMS = (64, 128, 256)
LUTS = ('f32', 'f16')
SEARCHES = {'plain-k20': (20, False), 'plain-k32': (32, False), 'stage-k80': (20, True), 'stage-k128': (32, True)}
QUERY_COUNTS = (3, 300)

_INDEX = {}


def _index(d):
    """One IVFPQ-RR index per d (k_factor 4) and its 300 queries on the device."""
    if d not in _INDEX:
        from neural_audio_fp_amd.eval import ivf
        rng = np.random.default_rng([2024, d])
        cent = (4.0 * rng.normal(size=(NLIST, d)) / np.sqrt(d)).astype(np.float32)
        of_row = rng.permutation(np.repeat(np.arange(NLIST), LIST_ROWS))
        x = (cent[of_row] + 0.3 * rng.normal(size=(len(of_row), d)) / np.sqrt(d)).astype(np.float32)
        pq = (0.3 * rng.normal(size=(64, 256, d // 64)) / np.sqrt(d)).astype(np.float32)
        refine = (0.1 * rng.normal(size=(4, 16, d // 4)) / np.sqrt(d)).astype(np.float32)
        q = (x[rng.permutation(len(x))[:max(QUERY_COUNTS)]] + 0.1 * rng.normal(size=(max(QUERY_COUNTS), d)) / np.sqrt(d)).astype(np.float32)
        idx = ivf.IVFPQRIndex(d, NLIST, k_factor=4)
        idx.set_params(cent, pq, refine)
        idx.add(x)
        idx.nprobe = NLIST
        offsets = idx.lists()[0].cpu().numpy()
        assert tuple(np.diff(offsets)) == LIST_ROWS               # the rows went where they were put
        _INDEX.clear()                                            # one at a time
        _INDEX[d] = (idx, torch.from_numpy(q).cuda())
    return _INDEX[d]


def scan_digest(d, lut, search, nq):
    """SHA-256 over the raw bytes of the search's outputs: D, I (float32, int32), preceded by D1, I1 for a first-stage search."""
    from neural_audio_fp_amd.eval import ivf
    idx, q = _index(d)
    k, stages = SEARCHES[search]
    idx.lut = lut
    out = idx.search_stages_device(q[:nq], k) if stages else ivf.IVFPQIndex.search_device(idx, q[:nq], k)
    assert [tuple(t.shape) for t in out] == ([(nq, 4 * k)] * 2 if stages else []) + [(nq, k)] * 2
    h = hashlib.sha256()
    for t in out:
        assert t.dtype == (torch.float32 if t.is_floating_point() else torch.int32)
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def case_key(d, lut, search, nq):
    return f'd{d}-{lut}-{search}-nq{nq}'


def test_the_lists_have_the_shapes_the_cases_need(nafp):
    lens = np.diff(_index(64)[0].lists()[0].cpu().numpy())
    assert (lens == 0).sum() == 1 and ((lens > 0) & (lens < 20)).sum() == 1
    assert ((lens >= 513) & (lens % 256 != 0)).any() and lens.sum() == 6000


@pytest.mark.parametrize('search', list(SEARCHES))
@pytest.mark.parametrize('lut', LUTS)
@pytest.mark.parametrize('d', DIMS)
def test_scan_bytes_are_the_recorded_ones(nafp, d, lut, search):
    with open(GOLDEN) as fh:
        want = json.load(fh)
    lens = np.diff(_index(d)[0].lists()[0].cpu().numpy())         # the shapes, before any search
    assert lens[0] == 0 and 0 < lens[1] < 20 and lens[2] >= 513 and lens[2] % 256 != 0
    for nq in QUERY_COUNTS:
        key = case_key(d, lut, search, nq)
        got = scan_digest(d, lut, search, nq)
        print(f'{key}: {got}')
        assert got == want[key], key
