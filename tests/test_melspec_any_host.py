"""CPU: nafp_melspec_create_ex refuses what it must before any HIP call, and nafp_melspec_plan_host describes the plan it
would build -- kernel, frame count, the mel bank's sparsity against the oracle's bank, LDS bytes."""
import ctypes

import numpy as np
import pytest

from oracle import melspec as o_mel

ANY, FORCE = 1, 2
FIELDS = 10
BASE = (8000, 8000, 1024, 256, 256, 300., 4000.)
# (fs, seg_len, n_fft, hop, n_mels, f_min, f_max), and (non-zeros, widest filter, empty rows) where the bank was counted by hand
GEOM = {
    'A': ((8000, 8000, 512, 256, 256, 300., 4000.), (470, 4, 0)),
    'B': ((16000, 16000, 2048, 512, 256, 300., 8000.), (1958, 22, 0)),
    'C': ((8000, 8000, 1024, 256, 100, 300., 4000.), (934, 21, 0)),
    'D': ((8000, 1001, 256, 100, 40, 0., 4000.), None),
    'E': ((16000, 16000, 4096, 1024, 128, 50., 8000.), None),
    'H': ((8000, 2000, 256, 64, 256, 300., 4000.), (235, 2, 63)),
    'L': ((16000, 16000, 256, 64, 64, 300., 8000.), None),
    'S': ((8000, 300, 512, 128, 64, 300., 4000.), None),
}


def _plan(lib, g, flags):
    rec = np.full(FIELDS, -1, np.int64)
    rc = lib.nafp_melspec_plan_host(*g, flags, rec.ctypes.data_as(ctypes.c_void_p))
    return rc, rec


def test_create_ex_without_flags_is_create(nafp):
    lib = nafp._lib.load()
    h = ctypes.c_void_p()
    assert lib.nafp_melspec_create_ex(ctypes.byref(h), 8000, 8000, 512, 256, 256, 300., 4000., 0) == 2
    assert lib.nafp_melspec_create_ex(ctypes.byref(h), 8000, 8000, 1024, 256, 100, 300., 4000., 0) == 2
    assert not h.value
    for g in (GEOM['A'][0], GEOM['C'][0]):
        assert _plan(lib, g, 0)[0] == 2


def test_create_ex_refusals_precede_any_hip_call(nafp):
    lib = nafp._lib.load()
    h = ctypes.c_void_p()
    for n_fft, hop, n_mels in ((1000, 256, 256), (8192, 256, 256), (1024, 256, 513), (1024, 0, 256), (64, 16, 32), (512, 513, 64),
                               (1024, 256, 0)):
        for flags in (ANY, FORCE, ANY | FORCE):
            assert lib.nafp_melspec_create_ex(ctypes.byref(h), 8000, 8000, n_fft, hop, n_mels, 300., 4000., flags) == 2
            assert _plan(lib, (8000, 8000, n_fft, hop, n_mels, 300., 4000.), flags)[0] == 2
    assert lib.nafp_melspec_create_ex(ctypes.byref(h), 8000, (1 << 22) + 1, 512, 256, 64, 300., 4000., ANY) == 2
    assert not h.value
    assert lib.nafp_melspec_create_ex(None, 8000, 8000, 512, 256, 256, 300., 4000., ANY) == 1
    assert lib.nafp_melspec_create_ex(ctypes.byref(h), 8000, 8000, 512, 256, 256, 4000., 300., ANY) == 1
    assert lib.nafp_melspec_create_ex(ctypes.byref(h), 0, 8000, 512, 256, 256, 300., 4000., ANY) == 1
    assert lib.nafp_melspec_create_ex(ctypes.byref(h), 8000, 8000, 512, 256, 256, 300., 4000., 4) == 1     # an unknown flag bit
    assert lib.nafp_melspec_plan_host(*GEOM['A'][0], ANY, None) == 1
    assert lib.nafp_melspec_kernel(None) == -1


@pytest.mark.parametrize('tag', sorted(GEOM))
def test_plan_record_against_the_oracle_bank(nafp, tag):
    lib = nafp._lib.load()
    g, counted = GEOM[tag]
    fs, seg_len, n_fft, hop, n_mels, f_min, f_max = g
    rc, rec = _plan(lib, g, ANY)
    assert rc == 0
    fb = o_mel.mel_filterbank(fs, n_fft, n_mels, f_min, f_max)
    nz = fb != 0
    width = [int(np.flatnonzero(r)[-1] - np.flatnonzero(r)[0] + 1) if r.any() else 0 for r in nz]
    bank = (int(nz.sum()), max(width), int((~nz.any(axis=1)).sum()))
    if counted is not None:
        assert bank == counted
    assert rec[0] == 1                                   # the general kernel
    assert rec[1] == 1 + seg_len // hop
    assert rec[2] == n_fft // 2 + 1
    assert tuple(rec[3:6]) == bank
    assert rec[6] >= 2 and rec[6] % 2 == 0               # frames are transformed in pairs
    assert rec[8] == -(-rec[1] // rec[6])
    assert rec[9] >= 1
    assert 0 < rec[7] <= 160 * 1024


def test_kernel_choice_at_the_base_geometry(nafp):
    lib = nafp._lib.load()
    rc0, r0 = _plan(lib, BASE, 0)
    rc1, r1 = _plan(lib, BASE, ANY)
    rc2, r2 = _plan(lib, BASE, FORCE)
    rc3, r3 = _plan(lib, BASE, ANY | FORCE)
    assert (rc0, rc1, rc2, rc3) == (0, 0, 0, 0)
    assert r0[0] == 0 and r1[0] == 0 and r2[0] == 1 and r3[0] == 1
    assert np.array_equal(r0, r1)
    fb = o_mel.mel_filterbank()
    for r in (r0, r2):
        assert r[1] == 32 and r[2] == 513 and r[3] == np.count_nonzero(fb) == 941 and r[4] <= 8 and r[5] == 0
    assert r0[6] == 16 and r0[8] == 2 and 64 * 1024 < r0[7] < 80 * 1024        # two workgroups of the tuned kernel share a CU
    # at the tuned kernel's own window a bank goes to the general kernel exactly when a filter is wider than the 8 taps the tuned
    # one gathers: then, and only then, nafp_melspec_create (flags 0) refuses it
    for g in ((8000, 8000, 1024, 256, 64, 300., 4000.), (8000, 8000, 1024, 256, 128, 300., 4000.),
              (8000, 8000, 1024, 256, 192, 300., 4000.), (16000, 16000, 1024, 256, 64, 0., 8000.)):
        rc, r = _plan(lib, g, ANY)
        assert rc == 0 and (r[0] == 1) == (r[4] > 8)
        assert _plan(lib, g, 0)[0] == (2 if r[4] > 8 else 0)


def test_lds_within_a_compute_unit_at_every_corner(nafp):
    lib = nafp._lib.load()
    seen = {}
    for n_fft in (128, 256, 512, 1024, 2048, 4096):
        for hop in (1, n_fft // 4, n_fft):
            for n_mels in (1, 256, 512):
                for seg_len in (1, 8000, 1 << 22):
                    rc, r = _plan(lib, (16000, seg_len, n_fft, hop, n_mels, 0., 8000.), ANY | FORCE)
                    assert rc == 0 and r[0] == 1
                    assert r[1] == 1 + seg_len // hop
                    assert 0 < r[7] <= 160 * 1024
                    assert seen.setdefault((n_fft, n_mels), r[7]) == r[7]           # LDS depends on the window and the bank only
    assert seen[(4096, 512)] == 108576
    assert seen[(2048, 256)] == 54304
