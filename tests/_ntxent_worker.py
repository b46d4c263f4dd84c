"""The call harness of the NT-Xent edge tests, and the child process of tests/test_gpu_ntxent_edges.py::test_environment_selected_paths.

HARNESS (`call`).  nafp_ntxent_forward through the C ABI with a workspace of need + 4096 bytes, of which the call is given `need`.
The workspace, its guard, loss_sum, sim_mtx and both gradients are filled with 0xFF bytes (a NaN as float and as double) before
the call: a partial that is read before it is written, or an output element that is never written, comes out as NaN, and a write
past the stated size changes the guard.

CHILD.  `python tests/_ntxent_worker.py` runs the reduced table `_ntxent_ref.WORKER` under whatever NAFP_NTXENT_* variables the
parent set (the library reads them once per process) and prints one JSON line: {"ok": bool, "worst": {kind: error / bound},
"cases": {name: {kind: ratio, "guard": bool, "finite": bool}}}.  Exit status 0 only if every ratio is below 1, every guard intact
and every output finite."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import _ntxent_ref as nr  # noqa: E402

GUARD = 4096
_DEV = {}


def device_pair(a, b):
    """The embeddings on the GPU, uploaded once per input set."""
    key = (id(a), id(b))
    if key not in _DEV:
        _DEV[key] = (a, b, torch.from_numpy(np.array(a)).cuda(), torch.from_numpy(np.array(b)).cuda())
    return _DEV[key][2:]


def _nan_filled(byte_shape):
    """float32 tensor of shape (rows, bytes / 4), every element the NaN 0xFFFFFFFF."""
    return torch.full(byte_shape, 0xFF, dtype=torch.uint8, device='cuda').view(torch.float32)


def call(a, b, n_local, off, tau, clone=False):
    """One guarded call.  Local buffers: the gathered arrays themselves when n_local = n_global and not `clone` (the pointer-identical
    single-device call), else copies of the rows [off, off + n_local).  Returns {'loss', 'sim', 'd_org', 'd_rep', 'guard'}."""
    from neural_audio_fp_amd import _lib
    lib = _lib.load()
    ta, tb = device_pair(a, b)
    ng, d = ta.shape
    if n_local == ng and not clone:
        la, lb = ta, tb
    else:
        la, lb = ta[off:off + n_local].clone(), tb[off:off + n_local].clone()
    need = int(lib.nafp_ntxent_workspace_bytes(n_local, ng))
    assert need > 0
    ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device='cuda')
    loss = _nan_filled((1, 4))
    sim = _nan_filled((n_local, (2 * ng - 1) * 4))
    d_org, d_rep = _nan_filled((ng, d * 4)), _nan_filled((ng, d * 4))
    assert sim.shape == (n_local, 2 * ng - 1) and d_org.shape == (ng, d) and bool(torch.isnan(sim).all())
    _lib.check(lib.nafp_ntxent_forward(_lib.ptr(la), _lib.ptr(lb), _lib.ptr(ta), _lib.ptr(tb), n_local, ng, off, d, float(tau),
                                       _lib.ptr(loss), _lib.ptr(sim), _lib.ptr(d_org), _lib.ptr(d_rep), _lib.ptr(ws), need,
                                       _lib.current_stream()), 'ntxent_forward')
    torch.cuda.synchronize()
    return {'loss': float(loss[0, 0]), 'sim': sim.cpu().numpy(), 'd_org': d_org.cpu().numpy(), 'd_rep': d_rep.cpu().numpy(),
            'guard': bool((ws[need:] == 0xFF).all())}


def all_finite(out):
    return bool(np.isfinite(out['loss']) and all(np.isfinite(out[k]).all() for k in ('sim', 'd_org', 'd_rep')))


def run_case(case):
    """Guarded call of a case and its comparison: (outputs, {'loss', 'sim', 'grad': error / bound})."""
    a, b = case.inputs()
    out = call(a, b, case.n_local, case.off, case.tau, clone=case.clone)
    return out, nr.compare(out, case.ref())


def main():
    cases, worst, ok = {}, {k: 0.0 for k in nr.KINDS}, True
    for case in nr.WORKER:
        out, ratios = run_case(case)
        rec = dict(ratios, guard=out['guard'], finite=all_finite(out))
        cases[case.name] = rec
        for k in nr.KINDS:
            worst[k] = max(worst[k], ratios[k], key=lambda v: np.inf if v != v else v)
        ok = ok and rec['guard'] and rec['finite'] and all(ratios[k] < 1.0 for k in nr.KINDS)
    print(json.dumps({'ok': bool(ok), 'worst': worst, 'cases': cases}))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
