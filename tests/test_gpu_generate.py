"""GPU: golden fixtures through the C ABI, larger-batch properties, and the generate
driver end to end (WAV files -> .mm memmap) against the oracle."""
import copy
import os
import wave

import numpy as np
import pytest
import torch

from oracle import melspec as o_mel, nnfp as o_nnfp, segments as o_seg
import _inputs

pytestmark = pytest.mark.gpu


def test_golden_fixtures_on_gpu(nafp, cfg, golden, observe, arith):
    x = _inputs.audio(4, seed=11)
    m_pre, m_fp = nafp.get_melspec_layer(cfg), nafp.get_fingerprinter(cfg)
    m_fp.set_weights(_inputs.weight_list(_inputs.weights(seed=3)))
    xt = torch.from_numpy(x).cuda()
    feat = m_pre(xt)
    observe('|d log-mel|', np.abs(feat.cpu().numpy() - golden['mel_seed11']).max(), 2e-5)
    observe('|d log-mel|', np.abs(m_pre(xt, group_size=2).cpu().numpy() - golden['mel_seed11_group2']).max(), 2e-5)
    # encoder on the GOLDEN features (isolates the encoder from front-end rounding)
    gfeat = torch.from_numpy(golden['mel_seed11']).cuda()
    observe('|d flat|', np.abs(m_fp.front_conv(gfeat).cpu().numpy() - golden['flat_seed11_w3']).max(), 5e-5)
    emb = m_fp(gfeat).cpu().numpy()
    observe('|d emb|', np.abs(emb - golden['emb_seed11_w3']).max(), 5e-6)
    observe('1 - cos', (1 - (emb * golden['emb_seed11_w3']).sum(1)).max(), 1e-6)      # contract 1e-3


def test_batch_independence_and_ragged_sizes(nafp, cfg):
    """Size-independent properties at full launch size: a segment's fingerprint does not
    depend on which other segments share the launch (given its feature), and ragged batch
    sizes (1, 3, 127, 129, 640) agree with each other."""
    rng = np.random.default_rng(0)
    feat = torch.from_numpy((-rng.uniform(0, 1.2, size=(640, 256, 32, 1))).astype(np.float32)).cuda()
    m_fp = nafp.FingerPrinter(seed=7)
    full = m_fp(feat)
    assert bool(torch.isfinite(full).all())
    assert float((full.norm(dim=1) - 1).abs().max()) < 1e-5
    for n in (1, 3, 127, 129, 1000):
        # [r5] bit for bit: every launch is planned (tile shape, split-K factor) as at the reference size of 640 segments
        # (csrc/conv.hip fwd_plan_b()) and the LayerNorm statistics are order-free integers -- until round 4 the split-K factor
        # of the late convs followed the batch size and these agreed to a few f32 ulps only
        src = feat[:n] if n <= 640 else torch.cat([feat, feat[:n - 640]])
        part = m_fp(src)
        assert torch.equal(part[:min(n, 640)], full[:min(n, 640)]), n
    perm = torch.randperm(640, device='cuda')
    assert torch.equal(m_fp(feat[perm]), full[perm])
    # oracle spot check on 3 rows of the full-size launch
    w = {k: v for k, v in zip(
        [n for j in range(16) for n in (f'conv{j}.kernel', f'conv{j}.bias', f'ln{j}.gamma', f'ln{j}.beta')] +
        ['div.w1', 'div.b1', 'div.w2', 'div.b2'], [v.cpu().numpy() for v in m_fp.trainable_variables])}
    idx = [0, 311, 639]
    want = o_nnfp.fingerprinter(feat[idx].cpu().numpy(), w)
    assert (1 - (full[idx].cpu().numpy() * want).sum(1)).max() < 1e-6


def test_launch_size_independence_beyond_the_arrival_counters(nafp, arith):
    """Round-5 ADVICE: convs 7 and 9 finish their split-K in-kernel on one arrival counter per output tile (4096 of them); a launch of
    more than ~4096 segments used to fall back to the finish kernel, which groups a sample's statistics into other partial sums -- the
    last bits of a fingerprint depended on the launch size again.  Now such a launch runs those layers as sample ranges: 4,500 rows in
    ONE launch == the same rows in launches of 640 and of 3, byte for byte -- under both arithmetics (the exact split plans every
    layer as at the reference launch size as well)."""
    g = torch.Generator(device='cuda').manual_seed(11)
    B = 4500
    feat = -1.2 * torch.rand((B, 256, 32, 1), generator=g, device='cuda')
    m_fp = nafp.FingerPrinter(seed=5)
    assert m_fp.split_arithmetic == (2 if arith == 'x6' else 0)
    whole = m_fp(feat).clone()
    assert bool(torch.isfinite(whole).all())
    for lo, n in ((0, 640), (640 * 6, 640), (4096, 404), (4497, 3)):
        assert torch.equal(m_fp(feat[lo:lo + n]), whole[lo:lo + n]), (lo, n)


def test_melspec_full_batch_properties(nafp, cfg):
    x = torch.from_numpy(_inputs.audio(640, seed=21)).cuda()
    m_pre = nafp.get_melspec_layer(cfg)
    f_all = m_pre(x, group_size=125)                                    # 5 full groups + 15
    assert f_all.shape == (640, 256, 32, 1)
    for g0 in range(0, 640, 125):
        assert float(f_all[g0:g0 + 125].max()) == 0.0                   # each group has its own zero max
        assert torch.equal(f_all[g0:g0 + 125], m_pre(x[g0:g0 + 125]))   # == the reference's per-batch call
    # linearity of the pre-log path: scaling audio by 0 gives log10(0.06) - max everywhere
    z = m_pre(torch.zeros(2, 1, 8000, device='cuda'))
    assert float(z.abs().max()) == 0.0


def _write_wav(path, pcm, fs=8000):
    with wave.open(path, 'w') as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(fs)
        w.writeframes(pcm.astype('<i2').tobytes())


def test_generate_fingerprint_end_to_end(nafp, cfg, tmp_path):
    from neural_audio_fp_amd.model import generate as g
    c = copy.deepcopy(cfg)
    c['BSZ']['TS_BATCH_SZ'] = 5
    c['DIR']['LOG_ROOT_DIR'] = str(tmp_path) + '/logs/'
    c['DIR']['OUTPUT_ROOT_DIR'] = str(tmp_path) + '/logs/emb/'
    src = tmp_path / 'src'; src.mkdir()
    rng = np.random.default_rng(5)
    t = np.arange(40000) / 8000.0
    for i, n in enumerate([5000, 8000, 12001, 30000, 9000]):
        pcm = rng.integers(-3000, 3000, size=n) + (6000 * np.sin(2 * np.pi * (500 + 300 * i) * t[:n])).astype(int)
        _write_wav(str(src / f'{i}.wav'), pcm)
    m_fp = nafp.get_fingerprinter(c)
    w = _inputs.weights(seed=8)
    m_fp.set_weights(_inputs.weight_list(w))
    g.save_checkpoint(c['DIR']['LOG_ROOT_DIR'] + 'checkpoint/', 'exp', 7, m_fp)
    g.generate_fingerprint(c, 'exp', None, str(src), None, True)
    out_dir = c['DIR']['OUTPUT_ROOT_DIR'] + '/exp/7/'
    shape = np.load(out_dir + 'custom_source_shape.npy')
    assert shape.dtype == np.int64 and tuple(shape) == (1 + 1 + 2 + 6 + 1, 128)
    got = np.asarray(np.memmap(out_dir + 'custom_source.mm', dtype='float32', mode='r', shape=tuple(shape)))
    # eval_faiss.load_memmap_data opens it exactly like this (eval/eval_faiss.py:47-59)
    paths = sorted(str(p) for p in src.glob('*.wav'))
    want = np.concatenate([o_nnfp.fingerprinter(o_mel.melspec_layer(b), w) for b in o_seg.load_batches(paths, 5)])
    assert (1 - (got * want).sum(1)).max() < 1e-5                       # contract 1e-3
    assert np.abs(got - want).max() < 1e-4


def test_fused_conv0_option_is_bit_identical(nafp):
    """NAFP_OPT_FUSE_CONV0 re-generates conv0's activation inside conv1 with the same FMA order: the conv input is
    identical bit for bit; what differs is the order in which the per-sample statistics are accumulated (double atomics),
    so the fingerprints may move by ulps, not more (ragged and full batch sizes)."""
    rng = np.random.default_rng(4)
    m_fp = nafp.FingerPrinter(seed=9)
    for n in (3, 130, 640):
        feat = torch.from_numpy((-rng.uniform(0, 1.2, size=(n, 256, 32, 1))).astype(np.float32)).cuda()
        m_fp.set_option(1, 0)
        ref_flat, ref = m_fp.front_conv(feat), m_fp(feat)
        m_fp.set_option(1, 1)
        got_flat, got = m_fp.front_conv(feat), m_fp(feat)
        m_fp.set_option(1, 0)
        # statistics are accumulated with double atomics in a different order: allow 1 ulp-level noise
        assert float((got_flat - ref_flat).abs().max()) < 3e-5          # values of magnitude ~3; the oracle bound is 2e-4
        assert float((got - ref).abs().max()) < 3e-6        # unit-norm fingerprints: a few f32 ulps (measured 1.2e-6)


def test_run_py_generate_default_sources(nafp, cfg, tmp_path):
    """`python run.py generate NAME` on the reference's dataset directory convention
    (test-dummy-db-100k-full/, test-query-db-500-30s/{query,db}/): three memmaps, row counts,
    query/db of equal size, files readable the way eval_faiss.load_memmap_data reads them."""
    import subprocess
    import sys
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    music = tmp_path / 'music'
    rng = np.random.default_rng(9)
    layout = {'test-dummy-db-100k-full/a': [12000, 9000, 30000], 'test-query-db-500-30s/query/x': [16000, 8000],
              'test-query-db-500-30s/db/x': [16000, 8000]}
    for sub, lens in layout.items():
        d = music / sub; d.mkdir(parents=True)
        for i, n in enumerate(lens):
            _write_wav(str(d / f'{i:03d}.wav'), rng.integers(-5000, 5000, size=n))
    c = copy.deepcopy(cfg)
    c['DIR']['SOURCE_ROOT_DIR'] = str(music) + '/'
    c['DIR']['LOG_ROOT_DIR'] = str(tmp_path) + '/logs/'
    c['DIR']['OUTPUT_ROOT_DIR'] = str(tmp_path) + '/logs/emb/'
    c['BSZ']['TS_BATCH_SZ'] = 4
    (tmp_path / 'config').mkdir()
    yaml.safe_dump(c, open(tmp_path / 'config' / 'tiny.yaml', 'w'))
    from neural_audio_fp_amd.model import generate as g
    m_fp = nafp.get_fingerprinter(c)
    g.save_checkpoint(c['DIR']['LOG_ROOT_DIR'] + 'checkpoint/', 'exp', 1, m_fp)
    r = subprocess.run([sys.executable, os.path.join(root, 'run.py'), 'generate', 'exp', '-c', 'tiny'],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = c['DIR']['OUTPUT_ROOT_DIR'] + '/exp/1/'
    want_rows = {'dummy_db': 2 + 1 + 6, 'query': 3 + 1, 'db': 3 + 1}
    for key, n in want_rows.items():
        shape = np.load(out + f'{key}_shape.npy')
        assert tuple(shape) == (n, 128)
        arr = np.memmap(out + f'{key}.mm', dtype='float32', mode='r', shape=(shape[0], shape[1]))
        assert np.allclose(np.linalg.norm(np.asarray(arr), axis=1), 1.0, atol=1e-5)
    # missing config -> sys.exit message of run.py:18
    r2 = subprocess.run([sys.executable, os.path.join(root, 'run.py'), 'generate', 'exp', '-c', 'nope'],
                        cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r2.returncode != 0 and 'is missing' in (r2.stdout + r2.stderr)


def test_window_ingest_is_bit_identical_to_row_ingest(nafp, cfg, tmp_path):
    """nafp_melspec_forward_windows_i16 (whole files uploaded once, windows indexed on the device) vs the
    materialised int16 rows: same arithmetic, so the log-mel features are equal bit for bit across file boundaries,
    short files, zero-padded tails and ragged launches; the fingerprints agree to the run-to-run noise of the encoder
    (its per-sample LayerNorm statistics meet through atomics whose order is not fixed: DESIGN.md)."""
    from neural_audio_fp_amd.model import generate as g
    from neural_audio_fp_amd.model.utils.audio_utils import SegmentSource
    rng = np.random.default_rng(11)
    paths = []
    for i, n in enumerate([100, 8000, 8001, 23999, 64000, 4000, 40000]):
        p = str(tmp_path / f'{i:02d}.wav')
        _write_wav(p, rng.integers(-9000, 9000, size=n))
        paths.append(p)
    src = SegmentSource(paths, bsz=7)
    m_pre, m_fp = g.build_fp(cfg)
    outs = []
    for windows in (False, True):
        arr = np.zeros((src.n_samples, 128), np.float32)
        g.write_fingerprints(src, g.StreamedEmbedder(m_pre, m_fp, windows=windows), arr, group=7, launch_rows=21)
        outs.append(arr)
    assert np.abs(outs[0]).sum() > 0
    assert np.abs(outs[0] - outs[1]).max() < 1e-6
    # the front end itself, bit for bit: rows [0, 21) as materialised int16 rows and as windows of the uploaded files
    rows = torch.from_numpy(src.read_rows(0, 21)).cuda()
    _, n, arena, used, off, valid = next(src.iter_windows(0, 21, 21))
    pcm = torch.from_numpy(np.asarray(arena[:max(used, 1)])).cuda()
    f_rows = m_pre(rows, group_size=7)
    f_win = m_pre.forward_windows(pcm, torch.from_numpy(off).cuda(), torch.from_numpy(valid).cuda(), group_size=7)
    assert n == 21 and torch.equal(f_rows, f_win)


def test_generate_with_synthesised_queries(nafp, cfg, tmp_path):
    """DATA_SEL.TEST_QUERY_DB = 'unseen_syn': query.mm holds fingerprints of on-the-fly augmented replicas of the DB
    segments (bg mix + IR + offset), row-aligned with db.mm; most of them retrieve their own DB row."""
    from neural_audio_fp_amd.model import generate as g
    from neural_audio_fp_amd.eval.eval_faiss import FlatL2Index
    rng = np.random.default_rng(77)
    t = np.arange(100000) / 8000.0
    base = str(tmp_path) + '/ds/'
    os.makedirs(base + 'music/val-query-db-500-30s/db/x'); os.makedirs(base + 'aug/bg/ts'); os.makedirs(base + 'aug/ir/ts')
    for i in range(3):
        x = rng.integers(-800, 800, size=100000) + sum(4000 * np.sin(2 * np.pi * f * t + p) for f, p in zip(rng.uniform(300, 3500, 4), rng.uniform(0, 6, 4)))
        _write_wav(base + f'music/val-query-db-500-30s/db/x/{i}.wav', x)
    _write_wav(base + 'aug/bg/ts/0.wav', rng.integers(-1500, 1500, size=50000))
    _write_wav(base + 'aug/ir/ts/0.wav', 15000 * np.exp(-np.arange(400) / 30.0) * rng.normal(size=400))
    c = copy.deepcopy(cfg)
    c['DIR'].update({'SOURCE_ROOT_DIR': base + 'music/', 'BG_ROOT_DIR': base + 'aug/bg/', 'IR_ROOT_DIR': base + 'aug/ir/',
                     'LOG_ROOT_DIR': str(tmp_path) + '/logs/', 'OUTPUT_ROOT_DIR': str(tmp_path) + '/logs/emb/'})
    c['DATA_SEL']['TEST_QUERY_DB'] = 'unseen_syn'
    c['TD_AUG']['TS_SNR'] = [10, 15]
    c['BSZ']['TS_BATCH_SZ'] = 20
    m_fp = nafp.get_fingerprinter(c)
    g.save_checkpoint(c['DIR']['LOG_ROOT_DIR'] + 'checkpoint/', 'syn', 1, m_fp)
    g.generate_fingerprint(c, 'syn', None, None, None, True)
    out = c['DIR']['OUTPUT_ROOT_DIR'] + '/syn/1/'
    n = 3 * 24                                                # 12.5-s clips: 24 segments each
    assert tuple(np.load(out + 'query_shape.npy')) == tuple(np.load(out + 'db_shape.npy')) == (n, 128)
    q = np.asarray(np.memmap(out + 'query.mm', dtype='float32', mode='r', shape=(n, 128)))
    d = np.asarray(np.memmap(out + 'db.mm', dtype='float32', mode='r', shape=(n, 128)))
    assert np.allclose(np.linalg.norm(q, axis=1), 1, atol=1e-4) and not np.allclose(q, d, atol=1e-3)
    idx = FlatL2Index(128); idx.add(d)
    hit = idx.search(q, 3)[1]
    # random-weight network, augmented + shifted queries of stationary tones: the right CLIP is found (its segments look alike)
    assert (hit[:, 0] // 24 == np.arange(n) // 24).mean() > 0.8


def test_split_k_arrival_counters_are_left_clean(nafp):
    """The split-K launches that finish in-kernel (conv.hip, EPI 4) count arrivals per output tile in the workspace and the
    last arriver resets its counter.  Alternating batch sizes -- different tile counts, with and without such launches, on
    the SAME workspace -- must therefore reproduce the first result, and two identical launches must agree to the ulp level
    (the parts are summed in part order; only the double atomics of the statistics have no fixed order)."""
    rng = np.random.default_rng(21)
    feat = torch.from_numpy((-rng.uniform(0, 1.2, size=(640, 256, 32, 1))).astype(np.float32)).cuda()
    m_fp = nafp.FingerPrinter(seed=2)
    first = m_fp(feat).clone()
    for n in (129, 640, 37, 320, 640):
        out = m_fp(feat[:n]).clone()
        assert bool(torch.isfinite(out).all())
        assert float((out - first[:n]).abs().max()) < 3e-6
    again = m_fp(feat).clone()
    assert float((again - first).abs().max()) < 1e-6
