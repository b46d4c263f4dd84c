"""CPU: what the audio ingest loaders hand to the device, pinned byte for byte -- the catalog of files that `SegmentSource` and
`PcmStore` build under each of the five switch settings, and every launch of `SegmentSource.iter_windows` (raw arena, windows,
pre-pass records, pieces) as a SHA-256 digest.  The catalogs and digests below were recorded from the loaders as they stood
before they were given one file catalog and one span planner; `_stages` is the only part of this file that follows that change.
No GPU call."""
import hashlib
import os

import numpy as np
import pytest

import _codec_ref as cref
import _flac_ref as fref
import _ingest_ref as iref

FS, DUR, HOP = 8000, .125, .0625             # 1000-sample segments every 500: files of 9000 to 20000 frames span several


def _stages(work):
    """[(pre-pass or None, {rate: pieces})] of a launch's work in the order the stages run."""
    return [(s.prepass, s.by_rate) for s in work.stages]


def _tri(n, period, amp, ch=1):
    """(n, ch) int64 triangle waves by integer arithmetic, a little integer hash on top so that no predictor is exact."""
    k = np.arange(n, dtype=np.int64)[:, None] + 37 * np.arange(ch, dtype=np.int64)[None, :]
    return amp - 2 * amp * np.abs(k % period - period // 2) // (period // 2) + (k * k * 7 + k * 3) % 13 - 6


def _pcm(fmt, n, fs, ch, period):
    q = _tri(n, period, 1 << 21, ch)                                         # 2^-23 of full scale, a quarter of it
    return iref.wav_bytes(fmt, iref.encode(fmt, q.reshape(-1)), fs, ch)


def _codec(codec, n, fs, ch, align, period, fact=None):
    return cref.wav_bytes(codec, cref.encode(codec, _tri(n, period, 8000, ch), ch, align), fs, ch, align, fact=fact)


def _flac(n, fs, ch, bps, block, period):
    return fref.write_stream(_tri(n, period, 1 << (bps - 3), ch), bps, fs, block=block).data


# name -> (first switch setting that takes it, bytes); settings in the order each includes the one before
SETTINGS = ('none', 'NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS', 'NAFP_INGEST_FLAC')
CORPUS = (('a_native.wav', 0, lambda: _pcm('s16', 9500, 8000, 1, 90)),
          ('b_s16x2_44100.wav', 1, lambda: _pcm('s16', 20000, 44100, 2, 300)),
          ('c_s24x2_48000.wav', 2, lambda: _pcm('s24', 19999, 48000, 2, 350)),
          ('d_alaw.wav', 3, lambda: _codec('alaw', 9001, 8000, 1, 1, 80)),
          ('e_flac16x2_44100.flac', 4, lambda: _flac(20000, 44100, 2, 16, 4096, 310)),        # 4 frames of 4096 and one of 3616
          ('f_short.wav', 0, lambda: _pcm('s16', 700, 8000, 1, 70)),                          # shorter than one segment
          ('g_f32_44100.wav', 2, lambda: _pcm('f32', 15000, 44100, 1, 280)),
          ('h_ima4x2_22050.wav', 3, lambda: _codec('ima4', 12201, 22050, 2, 256, 200, fact=12000)),   # 49 blocks of 249; fact ends inside the last
          ('i_zero.wav', 0, lambda: _pcm('s16', 0, 8000, 1, 70)),                             # no frame at all
          ('j_u8_6000.wav', 2, lambda: _pcm('u8', 9000, 6000, 1, 60)),                        # upsampling
          ('k_ms4_11025.wav', 3, lambda: _codec('ms4', 10000, 11025, 1, 128, 110)),           # 41 blocks of 244
          ('l_flac24_8000.flac', 4, lambda: _flac(9500, 8000, 1, 24, 1024, 95)))              # 9 frames of 1024 and one of 284


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    root = tmp_path_factory.mktemp('launch_plan')
    for name, _, make in CORPUS:
        (root / name).write_bytes(make())
    return root


def _setting(monkeypatch, corpus, level):
    for k in SETTINGS[1:]:
        monkeypatch.delenv(k, raising=False)
    if level:
        monkeypatch.setenv(SETTINGS[level], '1')
    return [str(corpus / name) for name, first, _ in CORPUS if first <= level]


def _plain(v):
    if isinstance(v, (list, tuple, np.ndarray)):
        return [_plain(x) for x in v]
    return v if isinstance(v, (str, type(None))) else (bool(v) if isinstance(v, (bool, np.bool_)) else int(v))


CATALOG_KEYS = ('n_frames', 'data_offset', 'rate', 'channels', 'n_in', 'resampled', 'format', 'block_align', 'spb', 'flac', 'codecs',
                'ingest', 'resample')


def catalog(source, more):
    """The catalog attributes of a SegmentSource / PcmStore as plain Python values."""
    d = {k: _plain(getattr(source, k)) for k in CATALOG_KEYS + more}
    d['fns'] = [os.path.basename(f) for f in source.fns]
    d['flac_index'] = {f: [len(ix), ix.channels, ix.bps, ix.rate, int(ix.start[-1]), int(ix.offset[0]), int(ix.n_bytes.sum())]
                       for f, ix in source.flac_index.items()}
    return d


def _failed_base(source):
    return None if source.flac_failed is None else _plain(source.flac_failed.base)


def launches_digest(src, rows):
    """SHA-256 over every launch of iter_windows(0, n_samples, rows): arena[:used], used, seg_offset, seg_valid, out_total, and per
    stage in run order the pre-pass records, scratch size and failed-frame ids, then (rate, pieces) sorted by rate."""
    h = hashlib.sha256()
    i64 = lambda *v: h.update(np.asarray(v, '<i8').tobytes())
    for start, n, arena, used, off, valid, *work in src.iter_windows(0, src.n_samples, rows, alloc=lambda k: np.zeros(max(k, 1), np.int16)):
        i64(start, n, used, len(work))
        h.update(np.ascontiguousarray(arena[:used]).tobytes())
        h.update(np.asarray(off, '<i8').tobytes())
        h.update(np.asarray(valid, '<i4').tobytes())
        if not work or work[0] is None:
            continue
        i64(work[0].out_total)
        for prepass, by_rate in _stages(work[0]):
            if prepass is None:
                h.update(b'direct')
            else:
                records = prepass.pieces if hasattr(prepass, 'pieces') else prepass.frames
                scratch = prepass.scratch_samples if hasattr(prepass, 'scratch_samples') else prepass.scratch_bytes
                h.update(b'prepass')
                i64(len(records), scratch)
                h.update(records.tobytes())
                h.update(np.asarray(getattr(prepass, 'ids', []), '<i8').tobytes())
            for rate in sorted(by_rate):
                i64(rate, len(by_rate[rate]))
                h.update(by_rate[rate].tobytes())
    return h.hexdigest()


# ---- recorded from commit 85b1d22 (the loaders before the change), per switch setting: the digest of every launch for rows per
# launch of 1, 3 and 1000; SegmentSource's catalog; what PcmStore(base=16) adds to the same catalog ----
LAUNCHES = {
    ('none', 1): '8c540b82d28181799918029540cd518fa0268f708992afb98bdf4e7e5f008f9f',
    ('none', 3): '5097e3ae8ba9c2655b7dddd80c760170509ea29397c179a8f9789bb224302cd0',
    ('none', 1000): '13ba7af635caf770d2c23ec30c43477263d64763e6976c91051e35c2fe48577c',
    ('NAFP_RESAMPLE', 1): '4be4770d046fd49aba28a277020b65ab16cff773d49e02c9eddaa08464c074e7',
    ('NAFP_RESAMPLE', 3): '34fc68366001865db1a84302111bedfeb4c5d3d0d73776c9cc6ccd68f2ea6bbe',
    ('NAFP_RESAMPLE', 1000): 'dbbe779e4f290dc99dafca8294fc6c5f3415cb5f3764f6471a32e34dcf4dda25',
    ('NAFP_INGEST_ANY', 1): 'f1236aa7bc110e93a093228f55a15ecfbec052688197507f8512264f957decfd',
    ('NAFP_INGEST_ANY', 3): 'f2abd474d367a6973703d50dc40ed251b47016106b4aa0a4f9bf49c9f2eba717',
    ('NAFP_INGEST_ANY', 1000): '2fae72436411a2706f7c83abd093e240712d48522d81bd28ba57b524dc7925ac',
    ('NAFP_INGEST_CODECS', 1): 'e37d6e2478b0edb6ee9d023c1e489921c90da080ee92b25c8503b912b737a7ad',
    ('NAFP_INGEST_CODECS', 3): 'f4a33619ad37f4222cc21678b44fb0af3e425d34f3f4d53f8d1add1b3dbf592a',
    ('NAFP_INGEST_CODECS', 1000): '8effdc7e337a748eb1c209f5f20de608e651c71caf4482d9b5e7aa667861699d',
    ('NAFP_INGEST_FLAC', 1): '17359a2196762bc94d09b5c86c1ba666b6b7f47a900452749df52bf841a8af79',
    ('NAFP_INGEST_FLAC', 3): '9de424889bec30ee4a40bd7527270087c83ac86a11589043e0006f5e62544e48',
    ('NAFP_INGEST_FLAC', 1000): '7d4b3644e34d0f0fecacfd0145dc308e509a670936be30a0b121202d0e092744',
}
SOURCE = {
    'none': {'block_align': [],
             'channels': [1, 1, 1],
             'codecs': False,
             'data_offset': [44, 44, 44],
             'file_first': [0, 18, 19, 20],
             'flac': False,
             'flac_failed': None,
             'flac_index': {},
             'fns': ['a_native.wav', 'f_short.wav', 'i_zero.wav'],
             'format': [],
             'ingest': False,
             'n_frames': [9500, 700, 0],
             'n_in': [9500, 700, 0],
             'n_samples': 20,
             'rate': [8000, 8000, 8000],
             'resample': False,
             'resampled': [False, False, False],
             'spb': []},
    'NAFP_RESAMPLE': {'block_align': [],
                      'channels': [1, 2, 1, 1],
                      'codecs': False,
                      'data_offset': [44, 44, 44, 44],
                      'file_first': [0, 18, 24, 25, 26],
                      'flac': False,
                      'flac_failed': None,
                      'flac_index': {},
                      'fns': ['a_native.wav', 'b_s16x2_44100.wav', 'f_short.wav', 'i_zero.wav'],
                      'format': [],
                      'ingest': False,
                      'n_frames': [9500, 3629, 700, 0],
                      'n_in': [9500, 20000, 700, 0],
                      'n_samples': 26,
                      'rate': [8000, 44100, 8000, 8000],
                      'resample': True,
                      'resampled': [False, True, False, False],
                      'spb': []},
    'NAFP_INGEST_ANY': {'block_align': [2, 4, 6, 2, 4, 2, 1],
                        'channels': [1, 2, 2, 1, 1, 1, 1],
                        'codecs': False,
                        'data_offset': [44, 44, 44, 44, 44, 44, 44],
                        'file_first': [0, 18, 24, 29, 30, 34, 35, 58],
                        'flac': False,
                        'flac_failed': None,
                        'flac_index': {},
                        'fns': ['a_native.wav', 'b_s16x2_44100.wav', 'c_s24x2_48000.wav', 'f_short.wav', 'g_f32_44100.wav', 'i_zero.wav', 'j_u8_6000.wav'],
                        'format': ['s16', 's16', 's24', 's16', 'f32', 's16', 'u8'],
                        'ingest': True,
                        'n_frames': [9500, 3629, 3334, 700, 2722, 0, 12000],
                        'n_in': [9500, 20000, 19999, 700, 15000, 0, 9000],
                        'n_samples': 58,
                        'rate': [8000, 44100, 48000, 8000, 44100, 8000, 6000],
                        'resample': True,
                        'resampled': [False, True, True, False, True, False, True],
                        'spb': [1, 1, 1, 1, 1, 1, 1]},
    'NAFP_INGEST_CODECS': {'block_align': [2, 4, 6, 1, 2, 4, 256, 2, 1, 128],
                           'channels': [1, 2, 2, 1, 1, 1, 2, 1, 1, 1],
                           'codecs': True,
                           'data_offset': [44, 44, 44, 46, 44, 44, 60, 44, 44, 78],
                           'file_first': [0, 18, 24, 29, 46, 47, 51, 58, 59, 82, 95],
                           'flac': False,
                           'flac_failed': None,
                           'flac_index': {},
                           'fns': ['a_native.wav', 'b_s16x2_44100.wav', 'c_s24x2_48000.wav', 'd_alaw.wav', 'f_short.wav', 'g_f32_44100.wav', 'h_ima4x2_22050.wav',
                                   'i_zero.wav', 'j_u8_6000.wav', 'k_ms4_11025.wav'],
                           'format': ['s16', 's16', 's24', 'alaw', 's16', 'f32', 'ima4', 's16', 'u8', 'ms4'],
                           'ingest': True,
                           'n_frames': [9500, 3629, 3334, 9001, 700, 2722, 4354, 0, 12000, 7260],
                           'n_in': [9500, 20000, 19999, 9001, 700, 15000, 12000, 0, 9000, 10004],
                           'n_samples': 95,
                           'rate': [8000, 44100, 48000, 8000, 8000, 44100, 22050, 8000, 6000, 11025],
                           'resample': True,
                           'resampled': [False, True, True, True, False, True, True, False, True, True],
                           'spb': [1, 1, 1, 1, 1, 1, 249, 1, 1, 244]},
    'NAFP_INGEST_FLAC': {'block_align': [2, 4, 6, 1, 0, 2, 4, 256, 2, 1, 128, 0],
                         'channels': [1, 2, 2, 1, 2, 1, 1, 2, 1, 1, 1, 1],
                         'codecs': True,
                         'data_offset': [44, 44, 44, 46, 0, 44, 44, 60, 44, 44, 78, 0],
                         'file_first': [0, 18, 24, 29, 46, 52, 53, 57, 64, 65, 88, 101, 119],
                         'flac': True,
                         'flac_failed': [0, 0, 0, 0, 0, 5, 5, 5, 5, 5, 5, 5, 15],
                         'flac_index': {4: [5, 2, 16, 44100, 20000, 52, 28605], 11: [10, 1, 24, 8000, 9500, 52, 17719]},
                         'fns': ['a_native.wav', 'b_s16x2_44100.wav', 'c_s24x2_48000.wav', 'd_alaw.wav', 'e_flac16x2_44100.flac', 'f_short.wav',
                                 'g_f32_44100.wav', 'h_ima4x2_22050.wav', 'i_zero.wav', 'j_u8_6000.wav', 'k_ms4_11025.wav', 'l_flac24_8000.flac'],
                         'format': ['s16', 's16', 's24', 'alaw', 'flac16', 's16', 'f32', 'ima4', 's16', 'u8', 'ms4', 'flac24'],
                         'ingest': True,
                         'n_frames': [9500, 3629, 3334, 9001, 3629, 700, 2722, 4354, 0, 12000, 7260, 9500],
                         'n_in': [9500, 20000, 19999, 9001, 20000, 700, 15000, 12000, 0, 9000, 10004, 9500],
                         'n_samples': 119,
                         'rate': [8000, 44100, 48000, 8000, 44100, 8000, 44100, 22050, 8000, 6000, 11025, 8000],
                         'resample': True,
                         'resampled': [False, True, True, True, True, False, True, True, False, True, True, True],
                         'spb': [1, 1, 1, 1, 1, 1, 1, 249, 1, 1, 244, 1]},
}
PLACEMENT = {
    'none': {'start': [16, 9520, 10224], 'base': 16, 'end': 10224},
    'NAFP_RESAMPLE': {'start': [16, 9520, 13152, 13856], 'base': 16, 'end': 13856},
    'NAFP_INGEST_ANY': {'start': [16, 9520, 13152, 16488, 17192, 19920, 19920], 'base': 16, 'end': 31920},
    'NAFP_INGEST_CODECS': {'start': [16, 9520, 13152, 16488, 25496, 26200, 28928, 33288, 33288, 45288], 'base': 16, 'end': 52552},
    'NAFP_INGEST_FLAC': {'start': [16, 9520, 13152, 16488, 25496, 29128, 29832, 32560, 36920, 36920, 48920, 56184], 'base': 16, 'end': 65688},
}


@pytest.mark.parametrize('level', range(5), ids=SETTINGS)
def test_catalog_of_both_loaders(nafp, corpus, monkeypatch, level):
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    from neural_audio_fp_amd.model.utils.dataloader_keras import PcmStore
    fns = _setting(monkeypatch, corpus, level)
    src = SegmentSource(fns, 4, DUR, HOP, FS)
    got = catalog(src, ('file_first', 'n_samples'))
    got['flac_failed'] = _failed_base(src)
    assert got == SOURCE[SETTINGS[level]]
    store = PcmStore(fns, FS, base=16)
    assert store.n_frames.dtype == np.int64 and store.start.dtype == np.int64 and isinstance(src.n_frames, list)
    shared = {k: v for k, v in got.items() if k not in ('file_first', 'n_samples', 'flac_failed')}
    assert catalog(store, ('start', 'base', 'end')) == dict(shared, **PLACEMENT[SETTINGS[level]])
    assert _failed_base(store) == got['flac_failed']        # both loaders count failed FLAC frames in the same places


@pytest.mark.parametrize('rows', (1, 3, 1000))
@pytest.mark.parametrize('level', range(5), ids=SETTINGS)
def test_launches_of_iter_windows(nafp, corpus, monkeypatch, level, rows):
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    src = SegmentSource(_setting(monkeypatch, corpus, level), 4, DUR, HOP, FS)
    first = next(src.iter_windows(0, src.n_samples, rows))
    assert len(first) == (6 if level == 0 else 7)
    assert launches_digest(src, rows) == LAUNCHES[SETTINGS[level], rows]


# ---- one file through a small staging buffer: the planning half of PcmArena.device's run loop (ingest.file_runs) ----
RUN_FILES = ((1, 'b_s16x2_44100.wav', 'resample from 44100 Hz'), (4, 'c_s24x2_48000.wav', 'convert from 48000 Hz'),
             (4, 'j_u8_6000.wav', 'convert from 6000 Hz'), (4, 'h_ima4x2_22050.wav', 'convert from 22050 Hz'),
             (4, 'k_ms4_11025.wav', 'convert from 11025 Hz'), (4, 'e_flac16x2_44100.flac', 'convert FLAC from 44100 Hz'),
             (4, 'l_flac24_8000.flac', 'convert FLAC from 8000 Hz'))


@pytest.mark.parametrize('level,name,what', RUN_FILES, ids=[r[1] for r in RUN_FILES])
def test_runs_of_one_file_through_a_small_staging_buffer(nafp, corpus, monkeypatch, level, name, what):
    """The runs' outputs tile the file once and in order, every run's bytes fit the buffer, every piece and pre-pass record passes
    the kernels' own host checks, a FLAC file's frames are claimed by the runs that decode them (consecutive runs share boundary
    frames only) -- at a buffer derived from the file: the smallest the loader takes, plus room for an eighth of the file."""
    from neural_audio_fp_amd.model.utils.audio_utils import FileCatalog
    from neural_audio_fp_amd.model.utils import codecs as cd, flac as fl, ingest as ig
    fns = _setting(monkeypatch, corpus, level)
    cat = FileCatalog(fns, FS)
    e = cat.files[[os.path.basename(f) for f in fns].index(name)]
    fam = ig.family(e)
    refusal = f'^{e.fn}: staging buffer too small to {what}$'.replace('.', r'\.')

    def taken(size):
        try:
            next(ig.file_runs(e, FS, 0, size, cat.flac_failed))
        except NotImplementedError as err:
            assert str(err) == f'{e.fn}: staging buffer too small to {what}'
            return False
        return True

    lo, hi = 0, 1 << 22                                  # the floor room * L >= M: the smallest even size that is taken
    assert not taken(lo) and taken(hi)
    while hi - lo > 2:
        mid = (lo + hi) // 4 * 2
        lo, hi = (lo, mid) if taken(mid) else (mid, hi)
    with pytest.raises(NotImplementedError, match=refusal):
        next(ig.file_runs(e, FS, 0, hi - 2, cat.flac_failed))
    per_frame = 2 * e.flac.n_bytes.sum() / e.flac.start[-1] if e.kind == 'flac' else e.block_align / e.spb
    size = hi + int(e.n_in / 8 * per_frame) // 2 * 2
    out_off = 24
    total = out_off + (e.n_frames + 7) // 8 * 8
    runs = list(ig.file_runs(e, FS, out_off, size, cat.flac_failed))
    print(f'{name}: floor {hi} bytes, buffer {size} bytes, {len(runs)} runs')
    assert len(runs) >= 5
    assert [r[0] for r in runs] == [0] + [r[1] for r in runs[:-1]] and runs[-1][1] == e.n_frames and all(a < b for a, b, _ in runs)
    claimed = []
    for n0, n1, run in runs:
        (fn, file_off, n_bytes, at), = run.reads
        assert fn == e.fn and at == 0 and 0 < n_bytes <= size and file_off + n_bytes <= os.path.getsize(fn)
        raw_size = 2 * max((n_bytes + 1) // 2, 1)                            # what the loader uploads of its int16 staging buffer
        stages = _stages(run.work(total))
        assert len(stages) == 1 + (e.kind in ('codec', 'flac')) and bool(stages[0][1]) == (e.kind in ('pcm16', 'pcm'))
        prepass, by_rate = stages[-1]
        (rate, pieces), = by_rate.items()
        assert rate == e.rate and len(pieces) == 1 and (pieces['out0'][0], pieces['n_out'][0], pieces['out_off'][0]) == (n0, n1 - n0, out_off + n0)
        if e.kind == 'codec':
            cd.check_pieces(prepass.pieces, raw_size, max(prepass.scratch_samples, 1))
            raw_size = 2 * max(prepass.scratch_samples, 1)
        elif e.kind == 'flac':
            fl.check_frames(prepass.frames, raw_size, max(prepass.scratch_bytes, 1))
            raw_size = max(prepass.scratch_bytes, 1)
            assert prepass.failed is cat.flac_failed and len(prepass.ids) == len(prepass.frames)
            claimed.append(np.asarray(prepass.ids))
        fam.check_pieces(e.rate, FS, pieces, raw_size // 2 if e.kind == 'pcm16' else raw_size, total)
    if e.kind == 'flac':
        for a, b in zip(claimed, claimed[1:]):
            # in order; the filter's reach (under 200 input frames) is shorter than a FLAC frame, so at most the boundary frame twice
            assert np.all(np.diff(a) == 1) and a[0] <= b[0] and b[0] - a[-1] in (0, 1)
        assert np.array_equal(np.unique(np.concatenate(claimed)), e.frame_base + np.arange(len(e.flac)))
