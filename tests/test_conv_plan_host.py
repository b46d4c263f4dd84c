"""CPU: the plan of the conv GEMM launches (csrc/conv_plan.hip: plan_conv_gemm, seen through nafp_conv_plan of include/nafp.h)
against tests/golden/conv_plan_v1.json.

The fixture was NOT written by the planner.  It was recorded from the launcher as it stood before the planner existed (one function that
decided tile, split, finish, grid and kernel in line): that launcher, made to print instead of launch, was walked over the five call
kinds of csrc/api.hip (inference at the planning batch, inference with conv0 fused, training forward, transposed conv, PLAIN weight
image) x layers 1-15 x arithmetic x arrival counters given or not, for several launch sizes, two input sizes, the slab as the call
sites size it and as the layer alone would, and a few knob settings.  So a passing test means "the launches are what they were", and a
failing one names the query and the fields that moved: tile shape and split factor also fix the fp32 summation order, i.e. the last
bits of a fingerprint.  A deliberate change of the policy re-records the rows it moves and says so."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'conv_plan_v1.json')
N_FIELDS = 30
# the 3-stage forms of the three 64-column kernels that have a 2-stage form: taken only with NAFP_N64S2=0
KNOB_ONLY = {'conv_gemm_n64k16s3_infer', 'conv_gemm_n64k16s3_train', 'conv_gemm_n64k16s3_splitfin'}


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def _answers(group):
    """[(rc, record, kernel symbol)] of the group's queries, under the knobs of THIS process."""
    from neural_audio_fp_amd import _lib
    lib = _lib.load()
    out = []
    for (layer, n_seg, plan_b, flags, slab, _rc, _plan, _launches) in group['queries']:
        rec = (ctypes.c_int64 * N_FIELDS)()
        name = ctypes.create_string_buffer(96)
        rc = lib.nafp_conv_plan(group['in_f'], group['in_t'], layer, n_seg, plan_b, flags, slab, rec, name, len(name))
        out.append((rc, list(rec), name.value.decode()))
    return out


def _compare(fix, group, answers):
    names, fields = fix['kernels'], fix['record_fields']
    bad, seen = [], set()
    for q, (rc, rec, name) in zip(group['queries'], answers):
        want_rc, want = q[5], fix['plans'][q[6]]
        diff = [] if rc == want_rc else [f'rc {want_rc} -> {rc}']
        diff += [f'slab_wanted {want[29]} -> {rec[29]}'] if rec[29] != want[29] else []
        if rc == 0 and want_rc == 0:
            seen.add(name)
            diff += [f'kernel {names[want[0]]} -> {name}'] if name != names[want[0]] else []
            diff += [f'{fields[i]} {want[i]} -> {rec[i]}' for i in range(1, 29) if rec[i] != want[i]]
            launches = -(-q[1] // rec[27]) if rec[27] else 1
            diff += [f'launches {q[7]} -> {launches}'] if launches != q[7] else []
        if diff:
            bad.append((dict(zip(fix['query_fields'], q), **{k: group[k] for k in ('knob_set', 'in_f', 'in_t')}), diff))
    return bad, seen


def _table_rows():
    src = open(os.path.join(ROOT, 'neural-audio-fp_amd', 'csrc', 'conv.hip')).read()
    return re.findall(r'^\s*NAFP_ROW\((conv_gemm_\w+),', src, re.M)


def test_fixture_is_not_trivial():
    fix = _fixture()
    assert os.path.getsize(FIXTURE) < 200 * 1024
    assert len(fix['record_fields']) == N_FIELDS and fix['knob_sets'][0] == {}
    n = sum(len(g['queries']) for g in fix['groups'])
    assert n >= 1500
    assert {(g['in_f'], g['in_t']) for g in fix['groups']} >= {(256, 32), (256, 63)}
    assert {g['knob_set'] for g in fix['groups']} == set(range(len(fix['knob_sets']))) and len(fix['knob_sets']) >= 5
    plans = [fix['plans'][q[6]] for g in fix['groups'] for q in g['queries']]
    assert sum(p[14] == 1 for p in plans) >= 300 and sum(p[14] == 2 for p in plans) >= 20 and sum(p[14] == 3 for p in plans) >= 20
    assert sum(p[27] > 0 for p in plans) >= 5                       # launches cut into sample ranges
    assert {p[20] for p in plans} == {0, 1, 2}                      # every class order of the positions


def test_default_knob_plans_match_the_record(nafp):
    for k in os.environ:
        assert not (k.startswith('NAFP_') and k not in ('NAFP_TEST_HOOKS', 'NAFP_LIB')), f'{k} is set: this test holds the DEFAULT plan'
    fix = _fixture()
    bad, seen = [], set()
    for g in fix['groups']:
        if g['knob_set'] == 0:
            b, s = _compare(fix, g, _answers(g))
            bad += b
            seen |= s
    assert not bad, f'{len(bad)} plans moved, e.g. ' + '; '.join(f'{q}: {", ".join(d)}' for q, d in bad[:6])
    # every row of the launcher's table that the default knobs can reach is held by at least one query
    rows = _table_rows()
    assert len(rows) >= 30 and KNOB_ONLY < set(rows)
    assert set(rows) - seen == KNOB_ONLY, sorted(set(rows) - seen - KNOB_ONLY)


CHILD = '''
import json, sys
sys.path[:0] = [%r, %r]
import test_conv_plan_host as t
fix = t._fixture()
bad, seen = [], set()
for g in fix['groups']:
    if g['knob_set'] == int(sys.argv[1]):
        b, s = t._compare(fix, g, t._answers(g))
        bad += b; seen |= s
print(json.dumps({'bad': bad, 'seen': sorted(seen)}))
'''


@pytest.mark.parametrize('knob_set', [1, 2, 3, 4])
def test_plans_under_knobs_match_the_record(nafp, knob_set):
    """The knobs are read once per process: each set is asked in a child process of its own."""
    fix = _fixture()
    env = dict(os.environ, **fix['knob_sets'][knob_set])
    res = subprocess.run([sys.executable, '-c', CHILD % (ROOT, os.path.join(ROOT, 'tests')), str(knob_set)], env=env, check=True,
                         stdout=subprocess.PIPE, text=True)
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert sum(g['knob_set'] == knob_set for g in fix['groups']) >= 1
    assert not got['bad'], f'{len(got["bad"])} plans moved under {fix["knob_sets"][knob_set]}, e.g. {got["bad"][:4]}'
    if fix['knob_sets'][knob_set] == {'NAFP_N64S2': '0'}:
        assert KNOB_ONLY <= set(got['seen'])
