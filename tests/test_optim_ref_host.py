"""CPU: (1) the float32 emulation of the optimizer kernels stays inside the bounds of tests/_optim_ref.py against the float64 oracle
at every case of the GPU test; (2) every mutation of the emulation is caught by at least one of those cases through the same
comparison -- the evidence that the bounds are tight enough, gathered without touching a kernel; (3) the argument checks of the
optimizer, spec-augment and row-norm entry points of the C ABI that return BEFORE the first launch (the line is named at each call).
The pointers of (3) are fake and never dereferenced; this file also runs on the GPU box, so no call here may pass its checks.

What (2) finds (`pytest -s` prints it; the first case of the list that notices, and the figure that misses its bound of 4 / 4 / K):
  eps_inside_root, eps_x10, eps_div10         full_table_60: w 3.4e4 .. 3.4e5 (Adam), 1.9e4 .. 6.3e6 (LAMB)
  no_weight_decay, no_bias_correction_v       full_table_60: w 1.9e7          weight_decay_after_norms   full_table_60: w 2.0e3
  ratio_per_tensor                            full_table_60: w 4.4e9          segment_off_by_one_variable full_table_60: w 1.4e7
  zero_norm_gives_0                           zero_weights:  w 1.7e7          adam_lr_t_without_sqrt_bc2 full_table_60: w 2.9e8
  last_partial_block_skipped                  full_table_60: m, v, w 1.7e7    double_hyper_parameters    full_table_60: m 5.3, v 219
The emulation itself stays at m <= 1.89, v <= 2.76, w <= 1.89 (Adam) / 5.47 (LAMB) over all cases."""
import ctypes

import numpy as np
import pytest

import _optim_ref as R

NULL = None
FAKE = ctypes.c_void_p(4096)                # 16-byte aligned, never dereferenced
OK, INV, UNS, WS = 0, 1, 2, 4               # NAFP_OK, NAFP_ERR_INVALID_ARG, NAFP_ERR_UNSUPPORTED, NAFP_ERR_WORKSPACE


def _emulate_case(kind, case, mutation=None):
    """The observed maxima of one case with the emulation in the kernel's place."""
    hp = case.hp(kind)
    worst = {'m': 0.0, 'v': 0.0, 'w': 0.0}
    for t in case.tensors:
        new = R.emulate(kind, t.w, t.g, t.m, t.v, t.var_len, hp, case.step, mutation, aligned=t.misalign is None)
        obs = R.compare(kind, (t.w, t.g, t.m, t.v), (new[0], new[1], new[2]), t.var_len, hp, case.step)
        worst = {k: max(worst[k], obs[k]) for k in worst}
    return worst


def test_case_list_is_what_the_issue_asks_for():
    full = R.cases()[0]
    assert len(full.tensors) == 60 and R.n_elements(full) < 200_000
    shapes = [(t.w.size // t.var_len, t.var_len) for t in full.tensors]
    assert {n for nv, n in shapes if nv == 1} >= set(R.SINGLE_NUMELS) and set(shapes) >= set(R.STACKED)
    ragged = lambda s: s[0] * s[1] > R.OPT_BLK and (s[0] * s[1]) % R.OPT_BLK
    for launch in (shapes[:R.OPT_MAX_T], shapes[R.OPT_MAX_T:]):          # each launch: a stacked and a ragged multi-block tensor
        assert any(nv > 1 for nv, _ in launch) and any(ragged(s) for s in launch)
    assert [len(c.tensors) for c in R.cases()[1:3]] == [48, 49]
    assert [c.tensors[0].misalign for c in R.cases()[3:7]] == ['p', 'g', 'm', 'v'] and R.cases()[3].tensors[0].w.size == 8193


@pytest.mark.parametrize('kind', R.KINDS)
def test_formula_matches_oracle(kind):
    """Stage (b)'s formula at the oracle's own float64 moments is the oracle's step."""
    rng = np.random.default_rng(5)
    for step, over in ((1, {}), (7, dict(wd=0.1, eps=1e-3)), (10 ** 6, {})):
        hp = R.HP(kind, **over)
        w, g, m = (rng.normal(size=96).astype(np.float32) for _ in range(3))
        v = (rng.random(96) * 0.1).astype(np.float32)
        w_o, m_o, v_o = R.ref_moments(kind, w, g, m, v, 32, hp, step)
        assert np.allclose(R.ref_weights(kind, w, m_o, v_o, 32, hp, step), w_o, rtol=1e-13, atol=0)
    # ... and the oracle is called with the float32 values: 1 - b2 differs by 1.3e-5 from the plain double's
    assert abs((1 - R.HP('adam').b2) / (1 - 0.999) - 1) > 1e-5


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('case', R.cases(), ids=R.case_ids())
def test_emulation_within_bounds(kind, case):
    obs = _emulate_case(kind, case)
    assert not R.misses(kind, obs), (case.name, obs)
    print(f'{case.name} {kind}: ' + ', '.join(f'{k} {obs[k]:.2f} / {b:g}' for k, b in R.bounds(kind).items()))


@pytest.mark.parametrize('mutation', list(R.MUTATIONS))
def test_mutation_is_caught(mutation):
    """Each mutation of the emulation misses a bound at one case, at least, of the GPU test's own list."""
    caught = []
    for kind in R.MUTATIONS[mutation]:
        hit = None
        for case in R.cases():
            obs = _emulate_case(kind, case, mutation)
            if R.misses(kind, obs):
                hit = (case.name, {k: float(f'{x:.3g}') for k, x in obs.items()})
                break
        assert hit, f'{mutation} ({kind}): no case of the list notices it'
        caught.append((kind, hit))
    print(f'{mutation}: caught by ' + '; '.join(f'{k}: {c} {o}' for k, (c, o) in caught))


# ---------------------------------------------------------------- refusals through the C ABI ----------------------------------------------------------------
def _table(nafp, specs, ptr=FAKE):
    arr = (nafp._lib.OptTensor * len(specs))()
    for i, (numel, var_len) in enumerate(specs):
        arr[i] = nafp._lib.OptTensor(ptr.value, ptr.value, ptr.value, ptr.value, numel, var_len)
    return arr


def test_optimizer_refusals(nafp):
    lib = nafp._lib.load()
    good = _table(nafp, [(4096, 32), (10, 10)])
    adam = lambda tb, n, step=1: lib.nafp_adam_step(tb, n, 1e-3, 0.9, 0.999, 1e-7, step, NULL)
    lamb = lambda tb, n, step=1, ws=FAKE, ws_bytes=1 << 20: lib.nafp_lamb_step(tb, n, 1e-3, 0.9, 0.999, 1e-6, 1e-6, step, ws, ws_bytes, NULL)
    # nafp_adam_step, first line: `if (!tensors_host || n <= 0 || step < 1) return NAFP_ERR_INVALID_ARG;`
    assert adam(good, 0) == INV and adam(good, -1) == INV and adam(NULL, 2) == INV and adam(good, 2, step=0) == INV
    # nafp_lamb_step, first line: `if (!tensors_host || n <= 0 || step < 1 || !workspace) return NAFP_ERR_INVALID_ARG;`
    assert lamb(good, 0) == INV and lamb(NULL, 2) == INV and lamb(good, 2, step=0) == INV and lamb(good, 2, ws=NULL) == INV
    # nafp_lamb_workspace_bytes: 2 doubles per keras variable + 256; -1 for a bad table
    assert lib.nafp_lamb_workspace_bytes(good, 2) == (128 + 1) * 16 + 256
    assert lib.nafp_lamb_workspace_bytes(_table(nafp, [(128, 1), (7000, 1000), (5, 5)]), 3) == (128 + 7 + 1) * 16 + 256
    assert lib.nafp_lamb_workspace_bytes(NULL, 2) == -1 and lib.nafp_lamb_workspace_bytes(good, 0) == -1
    # nafp_lamb_step: `if (workspace_bytes < need) return NAFP_ERR_WORKSPACE;`, before the hipMemsetAsync
    need = lib.nafp_lamb_workspace_bytes(good, 2)
    assert lamb(good, 2, ws_bytes=need - 1) == WS and lamb(good, 2, ws_bytes=0) == WS
    # a bad FIRST tensor: the table check of the first 48 tensors precedes the first launch (check_tensors / fill_table: `t.var_len <= 0 ||
    # t.numel % t.var_len != 0`); LAMB already refuses at `if (need < 0)`
    for bad in ([(4096, 0), (10, 10)], [(4096, -32), (10, 10)], [(4096, 33), (10, 10)]):
        tb = _table(nafp, bad)
        assert lib.nafp_lamb_workspace_bytes(tb, 2) == -1
        assert adam(tb, 2) == INV and lamb(tb, 2) == INV


def test_specaug_and_rownorm_refusals(nafp):
    lib = nafp._lib.load()
    need = lib.nafp_specaug_mean_workspace_bytes()
    assert need == 256 * 8 + 256
    mis = ctypes.c_void_p(4096 + 4)
    for fn in (lib.nafp_specaug_mean, lib.nafp_specaug_range):
        # first line of each: null pointers and n <= 0 (nafp_specaug_mean: also `(uintptr_t)feat & 15`); second line: the workspace
        assert fn(FAKE, 0, FAKE, FAKE, need, NULL) == INV and fn(FAKE, -4, FAKE, FAKE, need, NULL) == INV
        assert fn(NULL, 8, FAKE, FAKE, need, NULL) == INV and fn(FAKE, 8, NULL, FAKE, need, NULL) == INV and fn(FAKE, 8, FAKE, NULL, need, NULL) == INV
        assert fn(FAKE, 8, FAKE, FAKE, need - 1, NULL) == WS and fn(FAKE, 8, FAKE, FAKE, 0, NULL) == WS
    assert lib.nafp_specaug_mean(mis, 8, FAKE, FAKE, need, NULL) == INV
    # specaug_launch: `if (n_rects > MAX_RECTS || (T % 4) != 0) return NAFP_ERR_UNSUPPORTED;` precedes the launch
    rects = (nafp._lib.Rect * 9)(*[nafp._lib.Rect(0, 1, 0, 1)] * 9)
    assert lib.nafp_specaug_apply(FAKE, 4, 256, 32, rects, 9, NULL, 0.0, NULL) == UNS
    assert lib.nafp_specaug_apply(FAKE, 4, 256, 30, rects, 8, NULL, 0.0, NULL) == UNS
    assert lib.nafp_specaug_apply(FAKE, 4, 256, 32, NULL, 1, NULL, 0.0, NULL) == INV
    assert lib.nafp_specaug_apply_fill_dev(FAKE, 4, 256, 32, rects, 8, NULL, NULL, NULL) == INV          # no fill value
    # nafp_specaug_apply_ex: the four checks in front of `if (n_seg == 0 || n_rects == 0) return NAFP_OK;`
    ex = lambda n_rects=2, n_sets=1, filler=NULL, n_fill=0, T=32, so=FAKE: lib.nafp_specaug_apply_ex(FAKE, 4, 256, T, FAKE, n_rects, n_sets, NULL,
                                                                                                       filler, n_fill, so, NULL)
    assert ex(n_rects=33) == UNS and ex(T=30) == UNS
    assert ex(n_sets=2) == INV and ex(n_sets=0) == INV and ex(n_sets=5) == INV                             # neither 1 nor n_seg = 4
    assert ex(filler=mis, n_fill=4) == INV and ex(filler=FAKE, n_fill=0) == INV and ex(so=NULL) == INV
    # nafp_l2_normalize_rows: first line, then `if (n_rows == 0) return NAFP_OK;`
    assert lib.nafp_l2_normalize_rows(FAKE, 4, 0, FAKE, NULL) == INV and lib.nafp_l2_normalize_rows(FAKE, 4, -1, FAKE, NULL) == INV
    assert lib.nafp_l2_normalize_rows(FAKE, -1, 64, FAKE, NULL) == INV
    assert lib.nafp_l2_normalize_rows(NULL, 4, 64, FAKE, NULL) == INV and lib.nafp_l2_normalize_rows(FAKE, 4, 64, NULL, NULL) == INV
    assert lib.nafp_l2_normalize_rows(FAKE, 0, 64, FAKE, NULL) == OK
