"""Identification: which track is this recording, and where in the track was it taken from.

`run.py identify NAME INDEX PATH...` fingerprints unlabelled recordings in memory (the `SegmentSource.iter_windows` +
`StreamedEmbedder` path of `generate`, every ingest switch included; nothing is written to .mm), searches the library's
fingerprints ({dummy_db, db}.mm or custom_source.mm, as `evaluate` loads them) with whatever `get_index` returns for `-i`,
and matches analysis windows of `--window` segments every `--window_hop` against the library's TRACKS with one kernel launch
(`FlatL2Index.identify` -> nafp_search_identify, include/nafp.h): alignments may be negative, a window is scored only where it
overlaps its track, votes are counted.  The mapping from row to file is the `<key>_tracks.json` that `generate` writes under
NAFP_TRACK_TABLE=1; without it there is nothing to name a match by, and the command says so before any GPU call.

The windowing (`plan_windows`) and the merge of per-window results into matches (`merge_windows`) are pure numpy.

`--speeds`: a recording played a few percent fast or slow, tempo and pitch together, matches nothing as it
is.  Each speed hypothesis fingerprints the recordings again with the speed undone on the device (`SegmentSource(step=...)`,
nafp_varispeed_*), runs the unchanged search, matcher and merge, and `select_across_speeds` chooses among the hypotheses' matches
per recording.  The model, the checkpoint and the index are built once; the cost is linear in the number of hypotheses.
`--tempos`: a time-stretched recording (tempo changed, pitch kept) is found by the segment search as it is,
but segment i of a window falls on library row a + round(i * tempo), not a + i.  All tempo hypotheses are matched in ONE launch of
`FlatL2Index.identify_tempo` (nafp_search_identify_tempo) on the fingerprints already computed; `merge_windows(..., rho=)` follows the
slanted lines from window to window.  With `--speeds p` in front, a pitch shift by p becomes a tempo of 1 / p.
No rejection threshold is built in: nobody has measured one on trained weights.  Every window is reported with its score
and votes, and `--min_score` is the user's to set.
"""
import json
import os
import sys

import numpy as np

MAX_SLOTS = 8192            # nafp_search_identify: k * max_len
MAX_SPEEDS = 64             # speed hypotheses of one run
MAX_TEMPOS = 16             # nafp_search_identify_tempo: hypotheses of one launch
TEMPO_ONE = 1 << 16         # a tempo hypothesis is 16.16 fixed point
TEMPO_MIN, TEMPO_MAX = 0.8, 1.25
MAX_SHORT = 256             # n_short of either matcher


def _grid(spec, opt, what, limit):
    """A comma list of values and / or ranges `lo:hi:inc` with both ends included -> the floats in the order given.  ValueError
    naming the option `opt` for anything that is not such a list, and for a range of more than `limit` values."""
    values = []
    for item in str(spec).split(','):
        item = item.strip()
        try:
            parts = [float(v) for v in item.split(':')]
        except ValueError:
            raise ValueError(f'{opt}: {item!r} is not a {what} or a range lo:hi:inc')
        if not all(np.isfinite(parts)):
            raise ValueError(f'{opt}: {item!r} is outside the supported range: every number must be finite')
        if len(parts) == 1:
            values.append(parts[0])
        elif len(parts) == 3:
            lo, hi, inc = parts
            if not (inc > 0 and lo <= hi):
                raise ValueError(f'{opt}: the range {item!r} needs lo <= hi and inc > 0')
            n = (hi - lo) / inc + 1e-9                             # (a float: a tiny inc makes it huge or infinite)
            n = limit + 1 if n > limit else int(n) + 1
            if n > limit:
                raise ValueError(f'{opt}: the range {item!r} holds more than {limit} hypotheses; at most {limit} are taken')
            values += [round(lo + k * inc, 10) for k in range(n)]
        else:
            raise ValueError(f'{opt}: {item!r} is not a {what} or a range lo:hi:inc')
    return values


def parse_speeds(spec):
    """`--speeds`: a comma list of speeds (`0.96,1,1.04`) and / or ranges `lo:hi:inc` with both ends included
    (`0.94:1.06:0.01`) -> [(step, reported speed)] in the order given, a step named twice kept once.  A speed s (the recording
    plays s times too fast) is undone by step = round(2^24 / s) and reported back as 2^24 / step.  ValueError by name for
    anything that is not such a list, for a speed outside 0.8 .. 1.25 and for more than MAX_SPEEDS hypotheses."""
    from ..model.utils import varispeed as vs
    out = []
    for v in _grid(spec, '--speeds', 'speed', MAX_SPEEDS):
        if not vs.SPEED_MIN <= v <= vs.SPEED_MAX:                  # (a NaN fails the comparison too)
            raise ValueError(f'--speeds: speed {v!r} is outside the supported range {vs.SPEED_MIN} .. {vs.SPEED_MAX}')
        step = vs.step_for(v)
        if step not in [st for st, _ in out]:
            out.append((step, vs.speed_of(step)))
    if len(out) > MAX_SPEEDS:
        raise ValueError(f'--speeds: {len(out)} hypotheses; at most {MAX_SPEEDS} are taken')
    return out


def parse_tempos(spec):
    """`--tempos`: the grammar of `--speeds` -> the hypotheses as the kernel takes them: rho = round(2^16 * tempo), the library rows
    advanced per segment of the recording in 16.16 fixed point, a rho named twice kept once, sorted by |rho - 2^16| and then by
    value, so that the kernel's tie rule (the hypothesis first in the list) means "nearest 1".  ValueError by name for anything
    that is not such a list, for a tempo outside 0.8 .. 1.25 and for more than MAX_TEMPOS hypotheses."""
    out = set()
    for v in _grid(spec, '--tempos', 'tempo', MAX_TEMPOS):
        if not TEMPO_MIN <= v <= TEMPO_MAX:
            raise ValueError(f'--tempos: tempo {v!r} is outside the supported range {TEMPO_MIN} .. {TEMPO_MAX}')
        out.add(int(round(TEMPO_ONE * v)))
    if len(out) > MAX_TEMPOS:
        raise ValueError(f'--tempos: {len(out)} hypotheses; at most {MAX_TEMPOS} are taken')
    return sorted(out, key=lambda rho: (abs(rho - TEMPO_ONE), rho))


def tempo_off(n, rho):
    """off(n) of nafp_search_identify_tempo: the library rows that n segments of the recording advance under rho."""
    return (int(n) * int(rho) + 32768) >> 16


def select_across_speeds(matches):
    """The matches of every speed hypothesis (dicts with `recording`, `recording_span_s`, `score`, `speed`) -> the ones kept, per
    recording (told apart by `_rec`, its place among the recordings, where a match carries one: a path may be given twice).  Candidates are taken by score descending, then |log speed| ascending, then |log tempo| ascending (`--tempos`; 1 where a
    match carries none), then speed, tempo and start of the span ascending; one is accepted unless its span overlaps an already accepted span of the same recording by more than half of the
    shorter of the two.  Returned in the order of the recordings' first appearance, then by start of the span.  Pure host code."""
    import math
    which = lambda m: m.get('_rec', m['recording'])
    order = {}
    for m in matches:
        order.setdefault(which(m), len(order))
    tempo = lambda m: m.get('tempo', 1.0)                          # (`--tempos`: then the tempo nearer to 1, after the speed)
    ranked = sorted(matches, key=lambda m: (-m['score'], abs(math.log(m['speed'])), abs(math.log(tempo(m))), m['speed'], tempo(m),
                                            m['recording_span_s'][0]))
    kept = []
    for m in ranked:
        a0, a1 = m['recording_span_s']
        clash = False
        for k in kept:
            if which(k) != which(m):
                continue
            b0, b1 = k['recording_span_s']
            if min(a1, b1) - max(a0, b0) > 0.5 * min(a1 - a0, b1 - b0):
                clash = True
                break
        if not clash:
            kept.append(m)
    return sorted(kept, key=lambda m: (order[which(m)], m['recording_span_s'][0]))


def plan_windows(n_segments, window, window_hop):
    """Windows of `window` segments every `window_hop` over recordings of n_segments[r] segments each.  A recording shorter than
    a window is one window of its own length; the window that reaches the end of a recording is its last one, shortened, never
    dropped.  Returns (rec, s0, length) int64 arrays, one entry per window, recordings in order."""
    window, window_hop = int(window), int(window_hop)
    if window < 1 or window_hop < 1:
        raise ValueError('plan_windows: window and window_hop >= 1')
    rec, s0, ln = [], [], []
    for r, n in enumerate(n_segments):
        n, s = int(n), 0
        while s < n:
            rec.append(r); s0.append(s); ln.append(min(window, n - s))
            if s + window >= n:
                break
            s += window_hop
    return np.asarray(rec, np.int64), np.asarray(s0, np.int64), np.asarray(ln, np.int64)


def merge_windows(rec, s0, length, track, align, score, votes, min_score=None, align_tol=1, rho=None):
    """Per-window best results -> matches.  Window w of recording rec[w] starts at segment s0[w]; its best result is
    (track[w], align[w], score[w], votes[w]), track -1 = none.  The alignment in the recording's frame is a_rec = align - s0: the
    library row the recording's segment 0 falls on.  Consecutive windows of one recording with the same track whose a_rec differ
    by at most `align_tol` from the window before merge into one match; a window without a result, or with a score below
    `min_score` (None: no threshold), is no match and breaks the run.  Returns a list of dicts: rec, seg0, seg1 (the segments
    [seg0, seg1) of the recording the match spans), track, a_rec (of the best-scoring window), score (mean), votes (minimum),
    windows.
    rho (`--tempos`): the tempo hypothesis of each window's result, 16.16 fixed point.  Window w then continues the run of the
    window before it if align_w is within `align_tol` of align_prev + off_prev(s0_w - s0_prev), the row the line of the window
    before reaches at s0_w (`tempo_off`; with rho = 2^16 this is the rule above).  The hypothesis may differ from window to
    window -- neighbouring ones cannot be told apart on a short window -- a match reports `rho`, that of its best-scoring
    window, and a_rec is extrapolated along that window's line to the recording's segment 0."""
    one = rho is None
    out, run, prev = [], None, None
    for w in range(len(rec)):
        ok = int(track[w]) >= 0 and np.isfinite(score[w]) and (min_score is None or float(score[w]) >= float(min_score))
        rho_w = TEMPO_ONE if one else int(rho[w])
        cur = (int(rec[w]), int(track[w]), int(align[w]), int(s0[w]), rho_w) if ok else None
        if (cur is not None and prev is not None and cur[:2] == prev[:2]
                and abs(cur[2] - (prev[2] + tempo_off(cur[3] - prev[3], prev[4]))) <= int(align_tol)):
            run['seg1'] = int(s0[w]) + int(length[w])
            run['_scores'].append(float(score[w])); run['_w'].append(cur)
            run['votes'] = min(run['votes'], int(votes[w]))
        else:
            run = None
            if cur is not None:
                run = {'rec': cur[0], 'seg0': int(s0[w]), 'seg1': int(s0[w]) + int(length[w]), 'track': cur[1], 'votes': int(votes[w]),
                       '_scores': [float(score[w])], '_w': [cur]}
                out.append(run)
        prev = cur
    for m in out:
        sc, ws = m.pop('_scores'), m.pop('_w')
        _, _, al, at, rho_w = ws[int(np.argmax(sc))]
        m['a_rec'] = al - tempo_off(at, rho_w)
        if not one:
            m['rho'] = rho_w
        m['score'] = float(np.mean(sc))
        m['windows'] = len(sc)
    return out


def recording_files(paths):
    """A file is taken as it is; a directory is globbed the way the dataset loader globs (`.flac` with NAFP_INGEST_FLAC=1; AIFF and AU names with NAFP_INGEST_AIFF=1)."""
    from ..model.dataset import _audio_files
    files = []
    for p in paths:
        if os.path.isdir(p):
            files += _audio_files(p.rstrip('/') + '/**/')
        else:
            files.append(p)
    return files


def library_keys(emb_dir):
    """[dummy_db ; db] as `evaluate` concatenates them, or custom_source when that is what the directory holds."""
    if os.path.exists(emb_dir + 'custom_source.mm') and not os.path.exists(emb_dir + 'db.mm'):
        return ['custom_source']
    return ['dummy_db', 'db']


def load_track_tables(emb_dir, keys, shapes):
    """The <key>_tracks.json files concatenated in the order of `keys`: (files, first (n_tracks + 1,) int32, hop_s, duration_s).
    Exits, naming NAFP_TRACK_TABLE=1, when one is missing or does not describe its .mm file."""
    files, first, base, hop_s, dur_s = [], [0], 0, None, None
    for key, shape in zip(keys, shapes):
        path = f'{emb_dir}{key}_tracks.json'
        if not os.path.exists(path):
            sys.exit(f'identify: {path} is missing.  The track table maps fingerprint rows to files; write it by running '
                     '`generate` with NAFP_TRACK_TABLE=1 in the environment.')
        with open(path) as f:
            t = json.load(f)
        if len(t['first']) != len(t['files']) + 1 or t['first'][0] != 0 or t['first'][-1] != int(shape[0]):
            sys.exit(f'identify: {path} does not describe {key}.mm ({int(shape[0])} rows); run `generate` again with NAFP_TRACK_TABLE=1.')
        if hop_s is not None and (t['hop_s'], t['duration_s']) != (hop_s, dur_s):
            sys.exit(f'identify: {path} was written with another hop / duration than the tables before it')
        hop_s, dur_s = t['hop_s'], t['duration_s']
        files += t['files']
        first += [base + int(v) for v in t['first'][1:]]
        base += int(shape[0])
    return files, np.asarray(first, np.int32), float(hop_s), float(dur_s)


def load_model(cfg, checkpoint_name, checkpoint_index):
    from ..model.generate import build_fp, load_checkpoint
    m_pre, m_fp = build_fp(cfg)
    load_checkpoint(cfg['DIR']['LOG_ROOT_DIR'] + 'checkpoint/', checkpoint_name, checkpoint_index, m_fp)
    return m_pre, m_fp


def fingerprint_recordings(cfg, checkpoint_name, checkpoint_index, files, step=None, model=None):
    """Fingerprints of `files` in memory: (rows (n, d) float32, rec_first (n_files + 1,)), through the path `generate` uses.
    step: the files are taken as played step / 2^24 times as fast (SegmentSource).  model: (m_pre, m_fp) of `load_model`, for
    a caller that fingerprints more than once."""
    from ..model.generate import StreamedEmbedder, write_fingerprints
    from ..model.utils.audio_utils import SegmentSource
    m_pre, m_fp = model or load_model(cfg, checkpoint_name, checkpoint_index)
    bsz = int(cfg['BSZ']['TS_BATCH_SZ'])
    src = SegmentSource(files, bsz, cfg['MODEL']['DUR'], cfg['MODEL']['HOP'], cfg['MODEL']['FS'], step=step)
    rows = np.empty((src.n_samples, int(cfg['MODEL']['EMB_SZ'])), np.float32)
    write_fingerprints(src, StreamedEmbedder(m_pre, m_fp), rows, bsz)
    return rows, np.asarray(src.file_first, np.int64)


def match_windows(flat, index, rows, rec_first, track_first, window, window_hop, k_probe, min_overlap, min_votes, n_short, rhos=None):
    """Top-k search of every recording row on `index`, then one nafp_search_identify launch over all windows on `flat` (the
    resident fp32 rows).  Returns the window plan and the best result per window as numpy arrays.  rhos (`--tempos`): the launch
    is nafp_search_identify_tempo's over these hypotheses.  The last member returned is the tempo of each window's result (a member of
    rhos, 2^16 where there is no result), None without rhos."""
    import torch
    rec, s0, ln = plan_windows(np.diff(rec_first), window, window_hop)
    dev = flat.device
    q = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(dev)
    _, ids = index.search_device(q, int(k_probe))
    ids = ids.to(torch.int32).contiguous()
    q0 = torch.from_numpy((rec_first[rec] + s0).astype(np.int32)).to(dev)
    tl = torch.from_numpy(ln.astype(np.int32)).to(dev)
    kw = dict(n_out=1, n_short=int(n_short), min_overlap=int(min_overlap), min_votes=int(min_votes), max_len=int(window))
    host = lambda t: t.cpu().numpy()
    if rhos is None:
        track, align, score, votes, overlap, n_cand = flat.identify(q, ids, q0, tl, track_first, **kw)
        return rec, s0, ln, host(track)[:, 0], host(align)[:, 0], host(score)[:, 0], host(votes)[:, 0], host(overlap)[:, 0], host(n_cand), None
    track, align, score, votes, overlap, n_cand, r = flat.identify_tempo(q, ids, q0, tl, track_first, rhos, **kw)
    r = host(r)[:, 0]
    rho = np.where(r >= 0, np.asarray(rhos, np.int64)[np.maximum(r, 0)], TEMPO_ONE)
    return (rec, s0, ln, host(track)[:, 0], host(align)[:, 0], host(score)[:, 0], host(votes)[:, 0], host(overlap)[:, 0], host(n_cand),
            rho)


def identify(cfg, checkpoint_name, checkpoint_index, paths, index_type='l2', window=20, window_hop=10, k_probe=20,
             min_overlap=4, min_votes=2, n_short=32, min_score=None, align_tol=1, output=None, emb_dir=None, speeds=None,
             tempos=None):
    """`run.py identify`.  Returns the dict written to identify.json.  speeds: the `--speeds` text, or None -- then the command
    prints and writes exactly what it did before the option existed.  tempos: the `--tempos` text, or None, likewise: without it
    the matcher is nafp_search_identify as before, with it every window is matched under all tempo hypotheses in one launch of
    nafp_search_identify_tempo, on the fingerprints of each speed hypothesis (the grid is the product of the two)."""
    from .eval_faiss import FlatL2Index, get_index, load_memmap_data
    hypotheses = None
    if speeds is not None:
        try:
            hypotheses = parse_speeds(speeds)                      # before any GPU call
        except ValueError as e:
            sys.exit(f'identify: {e}')
    rhos = None
    if tempos is not None:
        try:
            rhos = parse_tempos(tempos)                            # before any GPU call
        except ValueError as e:
            sys.exit(f'identify: {e}')
        if int(window) * int(k_probe) * len(rhos) > MAX_SLOTS:
            sys.exit(f'identify: --window {window} x --k_probe {k_probe} x {len(rhos)} tempos (--tempos) = '
                     f'{int(window) * int(k_probe) * len(rhos)} slots per window; the matcher (nafp_search_identify_tempo) takes at '
                     f'most {MAX_SLOTS}')
        # every true alignment has near-duplicates at the neighbouring tempos, which would crowd it out of a shortlist of n_short
        n_short = min(MAX_SHORT, int(n_short) * len(rhos))
    if int(window) * int(k_probe) > MAX_SLOTS:
        sys.exit(f'identify: --window {window} x --k_probe {k_probe} = {int(window) * int(k_probe)} slots per window; the matcher '
                 f'(nafp_search_identify) takes at most {MAX_SLOTS}')
    if int(window) < 1 or int(window_hop) < 1 or not 1 <= int(k_probe) <= 32:
        sys.exit('identify: --window and --window_hop >= 1, --k_probe in 1..32')
    if emb_dir is None:
        emb_dir = f"{cfg['DIR']['OUTPUT_ROOT_DIR']}{checkpoint_name}/{checkpoint_index}/"
    keys = library_keys(emb_dir)
    for key in keys:
        if not os.path.exists(f'{emb_dir}{key}.mm'):
            sys.exit(f'identify: {emb_dir}{key}.mm is missing; run `generate` first')
    shapes = [load_memmap_data(emb_dir, key, shape_only=True) for key in keys]
    track_files, track_first, hop_s, dur_s = load_track_tables(emb_dir, keys, shapes)      # before any GPU call
    files = recording_files(paths)
    if not files:
        sys.exit(f'identify: no recordings under {" ".join(paths)}')

    parts = [load_memmap_data(emb_dir, key)[0] for key in keys]
    index = get_index(index_type, parts[0], parts[0].shape, True)
    # the fp32 rows stay resident for scoring: the exact index itself, or the rows an approximate index keeps in insertion order
    flat = index if isinstance(index, FlatL2Index) else getattr(index, '_flat', None)
    own = not isinstance(flat, FlatL2Index)
    if own:
        flat = FlatL2Index(int(parts[0].shape[1]))
    for p in parts:
        index.add(p)
        if own:
            flat.add(p)
    if flat.ntotal != index.ntotal:
        sys.exit(f'identify: the index holds {index.ntotal} rows, its fp32 rows {flat.ntotal}')
    print(f'identify: {index.ntotal} library rows in {len(track_files)} tracks')

    from ..model.utils import varispeed as vs
    model = load_model(cfg, checkpoint_name, checkpoint_index)
    result_matches, n_windows, best_scores = [], 0, []
    for step, speed in hypotheses or [(vs.ONE, 1.0)]:
        # the hypothesis "as it is" runs the path without a step: no varispeed launch
        rows, rec_first = fingerprint_recordings(cfg, checkpoint_name, checkpoint_index, files, None if step == vs.ONE else step, model)
        rec, s0, ln, track, align, score, votes, overlap, n_cand, rho = match_windows(
            flat, index, rows, rec_first, track_first, window, window_hop, k_probe, min_overlap, min_votes, n_short, rhos)
        n_windows += int(len(rec))
        sigma = step / vs.ONE                                      # recording seconds per stretched second
        best = [None] * len(files)
        for w in range(len(rec)):
            if int(track[w]) >= 0 and np.isfinite(score[w]) and (best[int(rec[w])] is None or float(score[w]) > best[int(rec[w])]):
                best[int(rec[w])] = float(score[w])
        best_scores.append(best)
        for m in merge_windows(rec, s0, ln, track, align, score, votes, min_score, align_tol, rho):
            tr = m['track']
            span = [m['seg0'] * hop_s, (m['seg1'] - 1) * hop_s + dur_s]
            row = {'_rec': m['rec'], 'recording': files[m['rec']],
                   'recording_span_s': span if hypotheses is None else [span[0] * sigma, span[1] * sigma],
                   'track': track_files[tr], 'track_index': tr,
                   'track_position_s': (m['a_rec'] - int(track_first[tr])) * hop_s,
                   'score': m['score'], 'min_votes': m['votes'], 'windows': m['windows']}
            if hypotheses is not None:
                row['speed'] = speed
            if rhos is not None:
                row['tempo'] = m['rho'] / TEMPO_ONE                # library seconds per second of the (speed-undone) recording
            result_matches.append(row)
    if hypotheses is not None:
        result_matches = select_across_speeds(result_matches)

    sp_head, sp_cell = (f' {"speed":>7s}', lambda row: f' {row["speed"]:7.4f}') if hypotheses is not None else ('', lambda row: '')
    if rhos is not None:
        sp_head, speed_cell = sp_head + f' {"tempo":>7s}', sp_cell
        sp_cell = lambda row: speed_cell(row) + f' {row["tempo"]:7.4f}'
    print(f'{"recording":<32s} {"from":>8s} {"to":>8s}  {"track":<32s} {"at":>9s} {"score":>7s} {"votes":>5s} {"win":>4s}{sp_head}')
    for row in result_matches:
        print(f'{os.path.basename(row["recording"])[-32:]:<32s} {row["recording_span_s"][0]:8.1f} {row["recording_span_s"][1]:8.1f}  '
              f'{os.path.basename(row["track"])[-32:]:<32s} {row["track_position_s"]:9.1f} {row["score"]:7.4f} {row["min_votes"]:5d} '
              f'{row["windows"]:4d}{sp_cell(row)}')
    matched = {row.pop('_rec') for row in result_matches}
    for r, f in enumerate(files):
        if r not in matched:
            print(f'{os.path.basename(f)[-32:]:<32s} no match')
    requested = getattr(index, 'requested_type', index_type)
    used = index.index_description if hasattr(index, 'index_description') else 'L2 (exact, HIP FlatL2Index)'
    result = {'index_type_requested': requested, 'index_type_used': used, 'k_probe': int(k_probe), 'window': int(window),
              'window_hop': int(window_hop), 'min_overlap': int(min_overlap), 'min_votes': int(min_votes), 'n_short': int(n_short),
              'min_score': None if min_score is None else float(min_score), 'align_tol': int(align_tol), 'hop_s': hop_s,
              'duration_s': dur_s, 'recordings': files, 'n_windows': n_windows, 'matches': result_matches}
    if hypotheses is not None:
        # n_windows counts every hypothesis' windows; speed_best_scores[h][r]: the best window score of recording r under hypothesis h
        result['speeds'] = [speed for _, speed in hypotheses]
        result['speed_best_scores'] = best_scores
    if rhos is not None:
        # n_short above is the shortlist the launch used; the time scale of a match is speed x tempo
        result['tempos'] = [rho / TEMPO_ONE for rho in rhos]
    out_path = output or f'{emb_dir}identify.json'
    with open(out_path, 'w') as f:
        json.dump(result, f, indent=1)
    print(f'Saved {len(result_matches)} matches to {out_path}.')
    return result
