"""GPU: set_weights against the passes that read what it writes, from ANOTHER stream.

The trainer re-packs the updated variables on a stream of the handle's own (`FingerPrinter.prefetch_weights`), and the next pass on
the caller's stream relies on the waits inside the library: `nafp_encoder_set_weights` records `sw_copied` (the plain copies),
`sw_l1` (+ layer 1's packed kernel, G / Hb and -- on the exact split -- its three bf16 terms) and `sw_done` (everything); the training
forward waits for them before conv0, conv1 and conv2, every other pass for `sw_done`.  Left to timing, such a race hides: conv0 and
the next batch's front end usually outlast the re-pack.  The library's test hook NAFP_OPT_DEBUG_SW_DELAY (option 7, accepted only
with NAFP_TEST_HOOKS=1) holds set_weights' stream for 20 ms right behind `sw_copied` and again behind `sw_l1`, so a pass that waits
for an early event but reads something written later reads the previous parameter set (or, on a fresh handle, uninitialised memory)
EVERY time.

Each case: weight sets A and B of different seeds (a stale layer differs at O(1)).  Reference: a fresh handle, B and the pass on one
stream.  Test: A and one pass (A packed, and split under x6), the hook on, B through the trainer's route (`load_state_dict`,
`prefetch_weights`: the re-pack runs on the handle's prep stream), the pass at once on a third stream without a host synchronisation.
Embeddings of both passes bit-equal to the reference; gradients within 2e-5 of each tensor's largest entry (the float atomics of
the backward pass, as tests/test_gpu_backward.py's side-stream bound); the B embeddings against the float64 oracle too, so that a
wrong answer both runs share is caught as well."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import nnfp as o_nnfp
import _inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMS = ['layer_norm2d', 'layer_norm1d', 'batch_norm']
PASSES = ['forward', 'forward_train', 'backward']
SEED_A, SEED_B = 41, 42
DELAY_US = 20000
ROWS = [0, 31]             # oracle rows (in both batch sizes)


@functools.lru_cache(maxsize=None)
def _weights(norm, seed):
    w = _inputs.weights(seed=seed)
    return w if norm == 'layer_norm2d' else o_nnfp.convert_norm(w, norm, seed=seed + 1)


def _state(nafp, norm, seed):
    return dict(zip(nafp.model.fp.nnfp.tensor_names(norm), _inputs.weight_list(_weights(norm, seed))))


@functools.lru_cache(maxsize=None)
def _host_inputs():
    rng = np.random.default_rng(5)
    feat = (-rng.uniform(0, 1.2, size=(640, 256, 32, 1))).astype(np.float32)
    d_emb = rng.normal(size=(640, 128)).astype(np.float32)
    return feat, d_emb


@functools.lru_cache(maxsize=None)
def _oracle(norm, seed):
    return o_nnfp.fingerprinter(_host_inputs()[0][ROWS], _weights(norm, seed), norm=norm)


def _inputs_on_gpu(B):
    feat, d_emb = _host_inputs()
    return torch.from_numpy(feat[:B]).cuda(), torch.from_numpy(d_emb[:B]).cuda()


def _run(m, which, feat, d_emb):
    """[embeddings] (+ the 68 gradients for 'backward'), cloned on the current stream."""
    if which == 'forward':
        return [m(feat).clone()]
    out = [m.forward_train(feat).clone()]
    if which == 'backward':
        out += [g.clone() for g in m.backward(d_emb)]
    return out


def _reference(nafp, norm, which, feat, d_emb, x6, seed=SEED_B):
    """(outputs, handle): the caller keeps the handle alive, so that the test run's handle cannot be given its freed memory -- which
    holds the very parameter set a too-early read should miss."""
    m = nafp.FingerPrinter(seed=0, norm=norm)
    if x6 is not None:
        m.set_option(3, 2 if x6 else 0)
    m.load_state_dict(_state(nafp, norm, seed))
    out = _run(m, which, feat, d_emb)
    torch.cuda.synchronize()
    return out, m


def _prefetched(nafp, m, norm, which, feat, d_emb, switch_x6_on=False, seed=SEED_B):
    """The hook on, B through load_state_dict + prefetch_weights, the pass at once on another stream."""
    torch.cuda.synchronize()
    m.set_option(7, DELAY_US)
    m.load_state_dict(_state(nafp, norm, seed))
    m.prefetch_weights()
    if switch_x6_on:
        m.set_option(3, 2)
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        out = _run(m, which, feat, d_emb)
    torch.cuda.synchronize()
    m.set_option(7, 0)
    return out


def _compare(norm, which, got, want, observe, seed=SEED_B):
    assert torch.equal(got[0], want[0]), \
        f'embeddings differ from the one-stream run by up to {float((got[0] - want[0]).abs().max()):.3e}'
    if which == 'backward':
        worst = 0.0
        for a, b in zip(got[1:], want[1:]):
            worst = max(worst, float((a - b).abs().max()) / (float(b.abs().max()) + 1e-20))
        observe('prefetched vs one-stream gradients, rel. to the tensor max', worst, 2e-5)
    # the suite's bounds against float64: the inference forward 5e-6 (tests/test_gpu_parity_forward.py; the alternates 2e-5,
    # tests/test_gpu_norm_alternates.py), the training forward 2e-5 (tests/test_gpu_backward.py)
    tol = 5e-6 if which == 'forward' and norm == 'layer_norm2d' else 2e-5
    observe('|d emb| vs float64 oracle', np.abs(got[0][ROWS].cpu().numpy() - _oracle(norm, seed)).max(), tol)


@pytest.mark.parametrize('B', [32, 640])
@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('which', PASSES)
def test_a_pass_on_another_stream_sees_the_prefetched_weights(nafp, which, norm, B, observe, arith):
    """A packed (and split) by an earlier pass, B re-packed on the prep stream: the alternates' training forward runs on the f32
    kernels under x6 too -- still an ordering check of their own positional images."""
    feat, d_emb = _inputs_on_gpu(B)
    want, _ref = _reference(nafp, norm, which, feat, d_emb, None)
    m = nafp.FingerPrinter(seed=0, norm=norm)
    assert m.split_arithmetic == (2 if arith == 'x6' else 0)
    m.load_state_dict(_state(nafp, norm, SEED_A))
    old = _run(m, which, feat, d_emb)
    assert float((old[0] - want[0]).abs().max()) > 1e-2            # a stale parameter set is visible at O(1)
    got = _prefetched(nafp, m, norm, which, feat, d_emb)
    _compare(norm, which, got, want, observe)


@pytest.mark.parametrize('B', [32, 640])
@pytest.mark.parametrize('which', PASSES)
def test_the_first_set_weights_on_another_stream(nafp, which, B, observe, arith):
    """A fresh handle whose first set_weights is the prefetched one: what a too-early read finds (under x6 the split blob) is
    uninitialised memory, not an older parameter set.  Memory the runtime hands out again may hold what a freed handle left in
    it, so each case loads a parameter set of its own that no handle of this process held before."""
    seed = 100 + 4 * PASSES.index(which) + 2 * (B == 640) + (arith == 'x6')
    feat, d_emb = _inputs_on_gpu(B)
    want, _ref = _reference(nafp, 'layer_norm2d', which, feat, d_emb, None, seed=seed)
    m = nafp.FingerPrinter(seed=0)
    got = _prefetched(nafp, m, 'layer_norm2d', which, feat, d_emb, seed=seed)
    _compare('layer_norm2d', which, got, want, observe, seed=seed)


@pytest.mark.parametrize('B', [32, 640])
@pytest.mark.parametrize('which', PASSES)
def test_the_split_switched_on_after_a_set_weights_made_under_f32(nafp, which, B, observe, monkeypatch):
    """NAFP_OPT_BF16X3 = 2 switched on after the prefetched set_weights ran under f32: that set_weights split nothing, the first pass
    splits the new parameter set itself (`x6_dirty`) -- behind `sw_done`, not behind the early events."""
    monkeypatch.delenv('NAFP_BF16X3', raising=False)
    feat, d_emb = _inputs_on_gpu(B)
    want, _ref = _reference(nafp, 'layer_norm2d', which, feat, d_emb, True)
    m = nafp.FingerPrinter(seed=0)
    assert m.split_arithmetic == 0
    m.load_state_dict(_state(nafp, 'layer_norm2d', SEED_A))
    _run(m, which, feat, d_emb)
    got = _prefetched(nafp, m, 'layer_norm2d', which, feat, d_emb, switch_x6_on=True)
    assert m.split_arithmetic == 2
    _compare('layer_norm2d', which, got, want, observe)


def test_the_delay_hooks_are_refused_outside_a_test_process(nafp):
    """Options 6 and 7 hold a stream on purpose: accepted here (conftest.py sets NAFP_TEST_HOOKS=1), refused in any other process."""
    m = nafp.FingerPrinter(seed=0)
    for opt in (6, 7):
        assert m._lib.nafp_encoder_set_option(m._h, opt, 100) == 0
        assert m._lib.nafp_encoder_set_option(m._h, opt, 0) == 0
    code = ('import neural_audio_fp_amd as n\n'
            'm = n.FingerPrinter(seed=0)\n'
            'print([m._lib.nafp_encoder_set_option(m._h, o, 100) for o in (6, 7)])\n')
    env = {k: v for k, v in os.environ.items() if k != 'NAFP_TEST_HOOKS'}
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == '[2, 2]', r.stdout       # NAFP_ERR_UNSUPPORTED, both
