"""Kernel cost of the general ingest (NAFP_INGEST_ANY=1, csrc/ingest.hip) for one generate launch of 640 segments.

    python tools/ingest_bench.py [reps=7] [launches_per_rep=20] [--varispeed | --aiff]

Device-event times, every shape warmed up first, `reps` windows of `launches_per_rep` launches each per case, the cases
alternating inside a rep so that drift hits them alike; median and range over the reps, per launch:
  1. the one class of input both kernels serve, 16-bit stereo at 44.1 kHz: nafp_ingest_i16 next to nafp_resample_i16 on the same
     samples and pieces (outputs compared byte for byte on the way), and their ratio;
  2. 24-bit stereo at 48 kHz -> 8 kHz and 16-bit mono 11.025 kHz -> 16 kHz, next to the log-mel kernel of the same launch
     (640 windows over the ingest's output; the 16 kHz front end needs NAFP_MELSPEC_ANY=1, which this tool sets for that case).
  3. the codec pre-pass (NAFP_INGEST_CODECS=1, csrc/codec.hip) of G.711 8 kHz mono, IMA ADPCM 22.05 kHz stereo in 1024-byte
     blocks, MS ADPCM 44.1 kHz stereo in 2048-byte blocks and IMA ADPCM 44.1 kHz mono in 4096-byte blocks -- blocks of random
     bytes: the decoders have no data-dependent loop -- next to two figures of the same launch: the 16-bit ingest of the samples
     it decoded, and the log-mel kernel.
  4. the FLAC pre-pass (NAFP_INGEST_FLAC=1, csrc/flac.hip) of 44.1 kHz stereo 16-bit and 48 kHz stereo 24-bit in blocks of 4096 and
     8 kHz mono 16-bit in blocks of 1152 -- LPC order 8, Rice-coded, music-like input from the writer of tests/_flac_ref.py (one
     30-s file written once, every file of the launch holds its bytes: the decoder's loops ARE data-dependent) -- next to the
     ingest of the PCM it decoded and the log-mel kernel; `prepass_all_failed` is the same launch with every record cut to 8
     bytes, i.e. the launch overhead, the allocations and the store stage's zero fill without the serial stage; `index` is the
     host's one pass over the file (nafp_flac_index_host), in MB/s.
  5. the varispeed pass (`identify --speeds`, csrc/varispeed.hip) at sigma = 1 / 1.04 and 1 / 0.96 over the launch's 640 stretched
     segments, next to the ingest it follows (16-bit stereo at 44.1 kHz, the model-rate samples the stretched outputs read) and the
     log-mel kernel of the same launch.  `--varispeed` runs this row alone.
  6. what NAFP_INGEST_AIFF=1 adds: 16-bit stereo at 44.1 kHz BIG-endian (NAFP_INGEST_S16 | NAFP_INGEST_BE) next to the little-endian
     file of the same samples, the same pieces, alternating (outputs compared byte for byte on the way), and their ratio; and the
     codec pre-pass of Apple IMA4 at 44.1 kHz stereo (34-byte packets of random bytes) next to the 16-bit ingest it feeds and the
     log-mel kernel, as in 3.  `--aiff` runs these two rows alone.
A launch is 640 one-second segments at a hop of 0.5 s: 320.5 s of audio, cut into 30-s files as generate would (11 pieces).
One JSON line at the end."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

args = [a for a in sys.argv[1:] if not a.startswith('--')]
REPS = int(args[0]) if args else 7
PER_REP = int(args[1]) if len(args) > 1 else 20
SEGMENTS, FILE_SECONDS = 640, 30


def pieces_for(mod, fs_in, fs_out, frame_bytes, unit, extra):
    """The launch as generate cuts it: consecutive 30-s files, each one piece; raw offsets in `unit`-byte units (1: the ingest's
    bytes, 2: the resampler's int16), 16-byte aligned.  -> (piece array, raw bytes, outputs)."""
    total_out = (SEGMENTS - 1) * (fs_out // 2) + fs_out
    rows, raw_pos, out_pos = [], 0, 0
    while out_pos < total_out:
        n_in = FILE_SECONDS * fs_in
        n_out = min(mod.n_out(n_in, fs_in, fs_out), total_out - out_pos)
        first, last = mod.input_range(0, n_out, n_in, fs_in, fs_out)
        rows.append((raw_pos // unit, first, last - first, n_in, 0, out_pos, n_out) + extra)
        raw_pos += ((last - first) * frame_bytes + 15) // 16 * 16
        out_pos += (n_out + 7) // 8 * 8
    return np.array(rows, dtype=mod.PIECE_DTYPE), raw_pos, out_pos


def codec_pieces(ig, cd, codec, fs_in, fs_out, ch, align):
    """The launch of a codec tree as SegmentSource.iter_windows cuts it (ingest.LaunchPlan): per 30-s file the whole blocks that cover the frames its
    outputs read, decoded into a scratch arena that the file's ingest piece (16-bit PCM) indexes.
    -> (codec piece array, ingest piece array, raw bytes, scratch int16, outputs)."""
    spb = cd.samples_per_block(codec, ch, align)
    total_out = (SEGMENTS - 1) * (fs_out // 2) + fs_out
    c_rows, i_rows, raw_pos, scratch, out_pos = [], [], 0, 0, 0
    while out_pos < total_out:
        n_in = FILE_SECONDS * fs_in
        n_out = min(ig.n_out(n_in, fs_in, fs_out), total_out - out_pos)
        b0, b1 = cd.block_range(*ig.input_range(0, n_out, n_in, fs_in, fs_out), spb)
        c_rows.append((raw_pos, b1 - b0, scratch, cd.CODECS[codec], ch, align, spb))
        i_rows.append((2 * scratch, b0 * spb, min((b1 - b0) * spb, n_in - b0 * spb), n_in, 0, out_pos, n_out, ch, ig.FORMATS['s16'][0], 0))
        raw_pos += ((b1 - b0) * align + 15) // 16 * 16
        scratch += ((b1 - b0) * spb * ch + 7) // 8 * 8
        out_pos += (n_out + 7) // 8 * 8
    return np.array(c_rows, dtype=cd.PIECE_DTYPE), np.array(i_rows, dtype=ig.PIECE_DTYPE), raw_pos, scratch, out_pos


def flac_launch(ig, fl, index, fs_in, fs_out, file_bytes):
    """The launch of a FLAC tree as SegmentSource.iter_windows cuts it (ingest.LaunchPlan): per 30-s file the whole frames that cover the samples its
    outputs read.  -> (frame records, ingest piece array, raw bytes, scratch bytes, outputs, [(raw offset, file byte range)])."""
    total_out = (SEGMENTS - 1) * (fs_out // 2) + fs_out
    n_in = int(index.start[-1])
    f_rows, i_rows, copies, raw_pos, scratch, out_pos = [], [], [], 0, 0, 0
    while out_pos < total_out:
        n_out = min(ig.n_out(n_in, fs_in, fs_out), total_out - out_pos)
        k0, k1 = fl.frame_range(index, *ig.input_range(0, n_out, n_in, fs_in, fs_out))
        rows, n_raw, n_pcm = fl.records(index, k0, k1, raw_pos, scratch)
        f_rows.append(rows)
        copies.append((raw_pos, int(index.offset[k0]), n_raw))
        covered = int(index.start[k1] - index.start[k0])
        i_rows.append((scratch, int(index.start[k0]), min(covered, n_in - int(index.start[k0])), n_in, 0, out_pos, n_out, index.channels,
                       ig.FORMATS['s16' if index.bps <= 16 else 's24'][0], 0))
        raw_pos += (n_raw + 15) // 16 * 16
        scratch += (n_pcm + 15) // 16 * 16
        out_pos += (n_out + 7) // 8 * 8
    raw = np.zeros(raw_pos, np.uint8)
    data = np.frombuffer(file_bytes, np.uint8)
    for at, off, n in copies:
        raw[at:at + n] = data[off:off + n]
    return np.concatenate(f_rows), np.array(i_rows, dtype=ig.PIECE_DTYPE), raw, scratch, out_pos


def varispeed_launch(vs, ig, step, fs_in, ch, code, width):
    """The launch of recordings under a step as SegmentSource.iter_windows cuts it: per 30-s file the stretched outputs, the
    model-rate samples they read, and the file's frames those need.  -> (varispeed pieces, ingest pieces, raw bytes, model-rate
    samples, outputs)."""
    total_out = (SEGMENTS - 1) * 4000 + 8000
    n_model, n_file = FILE_SECONDS * 8000, FILE_SECONDS * fs_in
    v_rows, i_rows, raw_pos, mid_pos, out_pos = [], [], 0, 0, 0
    while out_pos < total_out:
        n_out = min(vs.n_out(n_model, step), total_out - out_pos)
        m0, m1 = vs.input_range(0, n_out, n_model, step)
        first, last = ig.input_range(m0, m1, n_file, fs_in, 8000)
        i_rows.append((raw_pos, first, last - first, n_file, m0, mid_pos, m1 - m0, ch, code, 0))
        v_rows.append((mid_pos, m0, m1 - m0, n_model, 0, out_pos, n_out, 0))
        raw_pos += ((last - first) * ch * width + 15) // 16 * 16
        mid_pos += (m1 - m0 + 7) // 8 * 8
        out_pos += (n_out + 7) // 8 * 8
    return np.array(v_rows, dtype=vs.PIECE_DTYPE), np.array(i_rows, dtype=ig.PIECE_DTYPE), raw_pos, mid_pos, out_pos


def varispeed_rows(res, rng):
    """5. the varispeed pass next to the ingest it follows and the log-mel of the same launch."""
    from neural_audio_fp_amd import _lib
    from neural_audio_fp_amd.model.utils import ingest as ig
    from neural_audio_fp_amd.model.utils import varispeed as vs
    lib, st = _lib.load(), _lib.current_stream()
    code, width = _lib.INGEST_FORMATS['s16']
    for name, speed in (('varispeed_1.04', 1.04), ('varispeed_0.96', 0.96)):
        step = vs.step_for(speed)
        v_p, i_p, raw_bytes, n_mid, n_out = varispeed_launch(vs, ig, step, 44100, 2, code, width)
        raw = torch.from_numpy(rng.integers(-32768, 32768, size=raw_bytes // 2).astype(np.int16)).cuda().view(torch.uint8)
        mid = torch.zeros((n_mid,), dtype=torch.int16, device='cuda')
        out = torch.zeros((n_out,), dtype=torch.int16, device='cuda')
        ig.check_pieces(44100, 8000, i_p, raw_bytes, n_mid)
        vs.check_pieces(step, v_p, n_mid, n_out)
        d_i = torch.from_numpy(i_p.view(np.uint8).reshape(-1)).cuda()
        d_v = torch.from_numpy(v_p.view(np.uint8).reshape(-1)).cuda()
        p_ing, p_vs = ig.plan_for(44100, 8000), vs.plan_for(step)
        f_ing = lambda: _lib.check(lib.nafp_ingest_i16(p_ing.handle, _lib.ptr(raw), raw_bytes, _lib.ptr(d_i), len(i_p), _lib.ptr(mid), n_mid,
                                                       st), 'ingest_i16')
        f_vs = lambda: _lib.check(lib.nafp_varispeed_i16(p_vs.handle, _lib.ptr(mid), n_mid, _lib.ptr(d_v), len(v_p), _lib.ptr(out), n_out, st),
                                  'varispeed_i16')
        f_ing()
        mel = mel_for(8000, out, n_out)
        t = timed([f_ing, f_vs, mel])
        res[name] = {'step': step, 'sigma': step / vs.ONE, 'pieces': len(v_p), 'model_rate_samples': int(n_mid), 'outputs': int(n_out),
                     'taps_per_output': p_vs.T, 'ingest_s16x2_44100': t[0], 'varispeed': t[1], 'log_mel': t[2],
                     'varispeed_over_ingest': round(t[1]['median_ms'] / t[0]['median_ms'], 3)}


CODEC_CASES = (('alaw_x1_8000', 'alaw', 8000, 1, 1), ('ima4_x2_22050_block1024', 'ima4', 22050, 2, 1024),
               ('ms4_x2_44100_block2048', 'ms4', 44100, 2, 2048), ('ima4_x1_44100_block4096', 'ima4', 44100, 1, 4096))
QT_CASE = ('qtima4_x2_44100', 'qtima4', 44100, 2, 68)


def codec_rows(res, rng, cases):
    """3. the codec pre-pass next to the 16-bit ingest of what it decoded and the log-mel of the same launch."""
    from neural_audio_fp_amd import _lib
    from neural_audio_fp_amd.model.utils import codecs as cd
    from neural_audio_fp_amd.model.utils import ingest as ig
    lib, st = _lib.load(), _lib.current_stream()
    for name, codec, fs_in, ch, align in cases:
        c_p, i_p, raw_bytes, scratch, n_out = codec_pieces(ig, cd, codec, fs_in, 8000, ch, align)
        raw = torch.from_numpy(rng.integers(0, 256, size=raw_bytes).astype(np.uint8)).cuda()
        pcm = torch.zeros((scratch,), dtype=torch.int16, device='cuda')
        out = torch.zeros((n_out,), dtype=torch.int16, device='cuda')
        cd.check_pieces(c_p, raw_bytes, scratch)
        ig.check_pieces(fs_in, 8000, i_p, 2 * scratch, n_out)
        d_c = torch.from_numpy(c_p.view(np.uint8).reshape(-1)).cuda()
        d_i = torch.from_numpy(i_p.view(np.uint8).reshape(-1)).cuda()
        plan = ig.plan_for(fs_in, 8000)
        f_dec = lambda: _lib.check(lib.nafp_codec_decode_i16(_lib.ptr(raw), raw_bytes, _lib.ptr(d_c), len(c_p), _lib.ptr(pcm), scratch, st),
                                   'codec_decode_i16')
        f_ing = lambda: _lib.check(lib.nafp_ingest_i16(plan.handle, _lib.ptr(pcm), 2 * scratch, _lib.ptr(d_i), len(i_p), _lib.ptr(out), n_out,
                                                       st), 'ingest_i16')
        mel = mel_for(8000, out, n_out)
        t = timed([f_dec, f_ing, mel])
        res[name] = {'pieces': len(c_p), 'raw_bytes': int(raw_bytes), 'decoded_samples': int(scratch), 'outputs': int(n_out),
                     'blocks_per_group': int(lib.nafp_codec_blocks_per_group(cd.CODECS[codec], ch, align)),
                     'prepass': t[0], 'ingest_s16': t[1], 'log_mel': t[2],
                     'prepass_over_ingest': round(t[0]['median_ms'] / t[1]['median_ms'], 3)}


def big_endian_row(res, rng):
    """6. 16-bit stereo 44.1 kHz big-endian next to the little-endian file of the same samples."""
    from neural_audio_fp_amd import _lib
    from neural_audio_fp_amd.model.utils import ingest as ig
    lib, st = _lib.load(), _lib.current_stream()
    plan = ig.plan_for(44100, 8000)
    runs, outs = [], []
    x = None
    for fmt in ('s16', 's16be'):
        pcs, raw_bytes, n_out = pieces_for(ig, 44100, 8000, 4, 1, (2, _lib.INGEST_FORMATS[fmt][0], 0))
        x = rng.integers(-32768, 32768, size=raw_bytes // 2).astype(np.int16) if x is None else x
        raw = torch.from_numpy(x if fmt == 's16' else x.byteswap()).cuda()
        out = torch.zeros((n_out,), dtype=torch.int16, device='cuda')
        d_p = torch.from_numpy(pcs.view(np.uint8).reshape(-1)).cuda()
        ig.check_pieces(44100, 8000, pcs, raw_bytes, n_out)
        runs.append(lambda raw=raw, d_p=d_p, out=out, n=len(pcs), raw_bytes=raw_bytes, n_out=n_out: _lib.check(
            lib.nafp_ingest_i16(plan.handle, _lib.ptr(raw), raw_bytes, _lib.ptr(d_p), n, _lib.ptr(out), n_out, st), 'ingest_i16'))
        outs.append(out)
    t_le, t_be = timed(runs)
    res['s16bex2_44100_to_8000'] = {'little_endian': t_le, 'big_endian': t_be, 'ratio': round(t_be['median_ms'] / t_le['median_ms'], 3),
                                    'identical': bool(torch.equal(outs[0], outs[1])), 'outputs': int(outs[0].numel()), 'taps_per_output': plan.T}


def timed(fns):
    """Per-launch milliseconds of each callable: median and (min, max) over REPS windows of PER_REP launches, alternating."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(REPS):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(PER_REP):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / PER_REP)
    return [{'median_ms': round(float(np.median(m)), 4), 'min_ms': round(min(m), 4), 'max_ms': round(max(m), 4)} for m in ms]


def mel_for(fs, out, n_out_total):
    """The log-mel launch over the 640 windows of `out` (deferred finish, as generate runs it)."""
    from neural_audio_fp_amd.model.fp.melspec.melspectrogram import Melspec_layer
    if fs != 8000:
        os.environ['NAFP_MELSPEC_ANY'] = '1'
    layer = Melspec_layer(input_shape=(1, fs), fs=fs, f_max=fs / 2.0)
    off = torch.arange(SEGMENTS, dtype=torch.int64, device='cuda') * (fs // 2)
    valid = torch.full((SEGMENTS,), fs, dtype=torch.int32, device='cuda')
    assert int(off[-1]) + fs <= n_out_total
    return lambda: layer.forward_windows(out, off, valid, group_size=SEGMENTS, defer=True)


def main():
    from neural_audio_fp_amd.model.utils import ingest as ig
    from neural_audio_fp_amd.model.utils import resample as rs
    from neural_audio_fp_amd import _lib
    res = {'device': torch.cuda.get_device_name(0), 'segments': SEGMENTS, 'reps': REPS, 'launches_per_rep': PER_REP}
    rng = np.random.default_rng(7)
    if '--varispeed' in sys.argv:
        varispeed_rows(res, rng)
        print(json.dumps(res))
        return
    if '--aiff' in sys.argv:
        big_endian_row(res, rng)
        codec_rows(res, rng, (QT_CASE,))
        print(json.dumps(res))
        return

    # 1. 16-bit stereo 44.1 kHz: both kernels on the same samples
    p_new, raw_bytes, n_out = pieces_for(ig, 44100, 8000, 4, 1, (2, _lib.INGEST_FORMATS['s16'][0], 0))
    p_old, _, _ = pieces_for(rs, 44100, 8000, 4, 2, (2,))
    raw = torch.from_numpy(rng.integers(-32768, 32768, size=raw_bytes // 2).astype(np.int16)).cuda()
    out_new = torch.zeros((n_out,), dtype=torch.int16, device='cuda')
    out_old = torch.zeros((n_out,), dtype=torch.int16, device='cuda')
    d_new = torch.from_numpy(p_new.view(np.uint8).reshape(-1)).cuda()
    d_old = torch.from_numpy(p_old.view(np.uint8).reshape(-1)).cuda()
    plan_new, plan_old = ig.plan_for(44100, 8000), rs.plan_for(44100, 8000)
    ig.check_pieces(44100, 8000, p_new, raw.numel() * 2, n_out)
    rs.check_pieces(44100, 8000, p_old, raw.numel(), n_out)
    lib, st = _lib.load(), _lib.current_stream()
    # the library entry points themselves: the timed window holds no host-side piece checks
    f_new = lambda: _lib.check(lib.nafp_ingest_i16(plan_new.handle, _lib.ptr(raw), raw.numel() * 2, _lib.ptr(d_new), len(p_new),
                                                   _lib.ptr(out_new), n_out, st), 'ingest_i16')
    f_old = lambda: _lib.check(lib.nafp_resample_i16(plan_old.handle, _lib.ptr(raw), raw.numel(), _lib.ptr(d_old), len(p_old),
                                                     _lib.ptr(out_old), n_out, st), 'resample_i16')
    t_new, t_old = timed([f_new, f_old])
    res['s16x2_44100_to_8000'] = {'ingest': t_new, 'resample': t_old, 'ratio': round(t_new['median_ms'] / t_old['median_ms'], 3),
                                  'identical': bool(torch.equal(out_new, out_old)), 'pieces': len(p_new), 'outputs': int(n_out),
                                  'taps_per_output': plan_new.T}

    # 2. 24-bit stereo 48 kHz -> 8 kHz and 16-bit mono 11.025 kHz -> 16 kHz, next to the log-mel of the same launch
    for name, fs_in, fs_out, fmt, ch in (('s24x2_48000_to_8000', 48000, 8000, 's24', 2), ('s16x1_11025_to_16000', 11025, 16000, 's16', 1)):
        code, width = _lib.INGEST_FORMATS[fmt]
        pcs, raw_bytes, n_out = pieces_for(ig, fs_in, fs_out, ch * width, 1, (ch, code, 0))
        raw = torch.from_numpy(rng.integers(0, 256, size=raw_bytes).astype(np.uint8)).cuda()
        out = torch.zeros((n_out,), dtype=torch.int16, device='cuda')
        d_p = torch.from_numpy(pcs.view(np.uint8).reshape(-1)).cuda()
        plan = ig.plan_for(fs_in, fs_out)
        ig.check_pieces(fs_in, fs_out, pcs, raw_bytes, n_out)
        fns = [lambda: _lib.check(lib.nafp_ingest_i16(plan.handle, _lib.ptr(raw), raw_bytes, _lib.ptr(d_p), len(pcs), _lib.ptr(out),
                                                      n_out, st), 'ingest_i16')]
        entry = {'pieces': len(pcs), 'outputs': int(n_out), 'taps_per_output': plan.T, 'raw_bytes': int(raw_bytes)}
        try:
            mel = mel_for(fs_out, out, n_out)
            mel()
            fns.append(mel)
        except Exception as e:                                    # the ingest figure stands without its neighbour
            entry['log_mel_error'] = repr(e)
        t = timed(fns)
        entry['ingest'] = t[0]
        if len(t) > 1:
            entry['log_mel'] = t[1]
        res[name] = entry

    codec_rows(res, rng, CODEC_CASES)
    # 4. the FLAC pre-pass next to the ingest of what it decoded and the log-mel of the same launch
    import time
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import _flac_ref as fr
    from neural_audio_fp_amd.model.utils import flac as fl
    for name, fs_in, ch, bps, block in (('flac16_x2_44100_block4096', 44100, 2, 16, 4096), ('flac24_x2_48000_block4096', 48000, 2, 24, 4096),
                                        ('flac16_x1_8000_block1152', 8000, 1, 16, 1152)):
        x = fr.music(FILE_SECONDS * fs_in, fs_in, ch, bps, seed=bps + ch, scale=.5)
        data = fr.write_stream(x, bps, fs_in, block=block, sub=fr.lpc_recipe(x[:fs_in, 0], 8, 12, porder=4, method=0)).data
        t0 = time.perf_counter()
        info, index = fl.scan(data)
        t_index = time.perf_counter() - t0
        idx = fl.Index(index, ch, bps, fs_in)
        f_p, i_p, raw_np, scratch, n_out = flac_launch(ig, fl, idx, fs_in, 8000, data)
        raw_bytes = len(raw_np)
        raw = torch.from_numpy(raw_np).cuda()
        pcm = torch.zeros((scratch,), dtype=torch.uint8, device='cuda')
        out = torch.zeros((n_out,), dtype=torch.int16, device='cuda')
        status = torch.zeros((len(f_p),), dtype=torch.int32, device='cuda')
        fl.check_frames(f_p, raw_bytes, scratch)
        ig.check_pieces(fs_in, 8000, i_p, scratch, n_out)
        f_cut = f_p.copy()
        f_cut['n_bytes'] = 8
        d_f = torch.from_numpy(f_p.view(np.uint8).reshape(-1)).cuda()
        d_cut = torch.from_numpy(f_cut.view(np.uint8).reshape(-1)).cuda()
        d_i = torch.from_numpy(i_p.view(np.uint8).reshape(-1)).cuda()
        plan = ig.plan_for(fs_in, 8000)
        f_dec = lambda: _lib.check(lib.nafp_flac_decode(_lib.ptr(raw), raw_bytes, _lib.ptr(d_f), len(f_p), _lib.ptr(pcm), scratch,
                                                        _lib.ptr(status), st), 'flac_decode')
        f_fail = lambda: _lib.check(lib.nafp_flac_decode(_lib.ptr(raw), raw_bytes, _lib.ptr(d_cut), len(f_p), _lib.ptr(pcm), scratch,
                                                         None, st), 'flac_decode')
        f_ing = lambda: _lib.check(lib.nafp_ingest_i16(plan.handle, _lib.ptr(pcm), scratch, _lib.ptr(d_i), len(i_p), _lib.ptr(out), n_out,
                                                       st), 'ingest_i16')
        f_dec()
        torch.cuda.synchronize()
        assert int((status != 0).sum()) == 0, 'the measured launch must decode'
        mel = mel_for(8000, out, n_out)
        t = timed([f_dec, f_fail, f_ing, mel])
        f_dec()                                                   # leave decoded PCM behind, not the zero fill
        res[name] = {'frames': len(f_p), 'raw_bytes': int(raw_bytes), 'decoded_bytes': int(scratch), 'outputs': int(n_out),
                     'file_bytes': len(data), 'bits_per_sample': round(8 * len(data) / x.size, 2),
                     'index': {'seconds': round(t_index, 4), 'mb_per_s': round(len(data) / 1e6 / t_index, 1), 'frames': len(index)},
                     'prepass': t[0], 'prepass_all_failed': t[1], 'ingest': t[2], 'log_mel': t[3],
                     'prepass_over_ingest': round(t[0]['median_ms'] / t[2]['median_ms'], 3)}
    varispeed_rows(res, rng)
    big_endian_row(res, rng)
    codec_rows(res, rng, (QT_CASE,))
    print(json.dumps(res))


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('ingest_bench: no GPU; a CPU run measures nothing')
    main()
