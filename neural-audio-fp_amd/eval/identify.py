"""Identification: which track is this recording, and where in the track was it taken from.

`run.py identify NAME INDEX PATH...` fingerprints unlabelled recordings in memory (the `SegmentSource.iter_windows` +
`StreamedEmbedder` path of `generate`, every ingest switch included; nothing is written to .mm), searches the library's
fingerprints ({dummy_db, db}.mm or custom_source.mm, as `evaluate` loads them) with whatever `get_index` returns for `-i`,
and matches analysis windows of `--window` segments every `--window_hop` against the library's TRACKS with one kernel launch
(`FlatL2Index.identify` -> nafp_search_identify, include/nafp.h): alignments may be negative, a window is scored only where it
overlaps its track, votes are counted.  The mapping from row to file is the `<key>_tracks.json` that `generate` writes under
NAFP_TRACK_TABLE=1; without it there is nothing to name a match by, and the command says so before any GPU call.

The windowing (`plan_windows`) and the merge of per-window results into matches (`merge_windows`) are pure numpy.
No rejection threshold is built in: nobody has measured one on trained weights.  Every window is reported with its score
and votes, and `--min_score` is the user's to set.
"""
import json
import os
import sys

import numpy as np

MAX_SLOTS = 8192            # nafp_search_identify: k * max_len


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


def merge_windows(rec, s0, length, track, align, score, votes, min_score=None, align_tol=1):
    """Per-window best results -> matches.  Window w of recording rec[w] starts at segment s0[w]; its best result is
    (track[w], align[w], score[w], votes[w]), track -1 = none.  The alignment in the recording's frame is a_rec = align - s0: the
    library row the recording's segment 0 falls on.  Consecutive windows of one recording with the same track whose a_rec differ
    by at most `align_tol` from the window before merge into one match; a window without a result, or with a score below
    `min_score` (None: no threshold), is no match and breaks the run.  Returns a list of dicts: rec, seg0, seg1 (the segments
    [seg0, seg1) of the recording the match spans), track, a_rec (of the best-scoring window), score (mean), votes (minimum),
    windows."""
    out, run, prev = [], None, None
    for w in range(len(rec)):
        ok = int(track[w]) >= 0 and np.isfinite(score[w]) and (min_score is None or float(score[w]) >= float(min_score))
        a_rec = int(align[w]) - int(s0[w])
        cur = (int(rec[w]), int(track[w]), a_rec) if ok else None
        if cur is not None and prev is not None and cur[:2] == prev[:2] and abs(cur[2] - prev[2]) <= int(align_tol):
            run['seg1'] = int(s0[w]) + int(length[w])
            run['_scores'].append(float(score[w])); run['_a'].append(a_rec)
            run['votes'] = min(run['votes'], int(votes[w]))
        else:
            run = None
            if cur is not None:
                run = {'rec': cur[0], 'seg0': int(s0[w]), 'seg1': int(s0[w]) + int(length[w]), 'track': cur[1], 'votes': int(votes[w]),
                       '_scores': [float(score[w])], '_a': [a_rec]}
                out.append(run)
        prev = cur
    for m in out:
        sc, al = m.pop('_scores'), m.pop('_a')
        m['a_rec'] = al[int(np.argmax(sc))]
        m['score'] = float(np.mean(sc))
        m['windows'] = len(sc)
    return out


def recording_files(paths):
    """A file is taken as it is; a directory is globbed the way the dataset loader globs (`.flac` with NAFP_INGEST_FLAC=1)."""
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


def fingerprint_recordings(cfg, checkpoint_name, checkpoint_index, files):
    """Fingerprints of `files` in memory: (rows (n, d) float32, rec_first (n_files + 1,)), through the path `generate` uses."""
    from ..model.generate import StreamedEmbedder, build_fp, load_checkpoint, write_fingerprints
    from ..model.utils.audio_utils import SegmentSource
    m_pre, m_fp = build_fp(cfg)
    load_checkpoint(cfg['DIR']['LOG_ROOT_DIR'] + 'checkpoint/', checkpoint_name, checkpoint_index, m_fp)
    bsz = int(cfg['BSZ']['TS_BATCH_SZ'])
    src = SegmentSource(files, bsz, cfg['MODEL']['DUR'], cfg['MODEL']['HOP'], cfg['MODEL']['FS'])
    rows = np.empty((src.n_samples, int(cfg['MODEL']['EMB_SZ'])), np.float32)
    write_fingerprints(src, StreamedEmbedder(m_pre, m_fp), rows, bsz)
    return rows, np.asarray(src.file_first, np.int64)


def match_windows(flat, index, rows, rec_first, track_first, window, window_hop, k_probe, min_overlap, min_votes, n_short):
    """Top-k search of every recording row on `index`, then one nafp_search_identify launch over all windows on `flat` (the
    resident fp32 rows).  Returns the window plan and the best result per window as numpy arrays."""
    import torch
    rec, s0, ln = plan_windows(np.diff(rec_first), window, window_hop)
    dev = flat.device
    q = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(dev)
    _, ids = index.search_device(q, int(k_probe))
    ids = ids.to(torch.int32).contiguous()
    q0 = torch.from_numpy((rec_first[rec] + s0).astype(np.int32)).to(dev)
    tl = torch.from_numpy(ln.astype(np.int32)).to(dev)
    track, align, score, votes, overlap, n_cand = flat.identify(q, ids, q0, tl, track_first, n_out=1, n_short=int(n_short),
                                                                min_overlap=int(min_overlap), min_votes=int(min_votes),
                                                                max_len=int(window))
    host = lambda t: t.cpu().numpy()
    return rec, s0, ln, host(track)[:, 0], host(align)[:, 0], host(score)[:, 0], host(votes)[:, 0], host(overlap)[:, 0], host(n_cand)


def identify(cfg, checkpoint_name, checkpoint_index, paths, index_type='l2', window=20, window_hop=10, k_probe=20,
             min_overlap=4, min_votes=2, n_short=32, min_score=None, align_tol=1, output=None, emb_dir=None):
    """`run.py identify`.  Returns the dict written to identify.json."""
    from .eval_faiss import FlatL2Index, get_index, load_memmap_data
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

    rows, rec_first = fingerprint_recordings(cfg, checkpoint_name, checkpoint_index, files)
    rec, s0, ln, track, align, score, votes, overlap, n_cand = match_windows(
        flat, index, rows, rec_first, track_first, window, window_hop, k_probe, min_overlap, min_votes, n_short)
    matches = merge_windows(rec, s0, ln, track, align, score, votes, min_score, align_tol)

    result_matches = []
    print(f'{"recording":<32s} {"from":>8s} {"to":>8s}  {"track":<32s} {"at":>9s} {"score":>7s} {"votes":>5s} {"win":>4s}')
    for m in matches:
        tr = m['track']
        row = {'recording': files[m['rec']],
               'recording_span_s': [m['seg0'] * hop_s, (m['seg1'] - 1) * hop_s + dur_s],
               'track': track_files[tr], 'track_index': tr,
               'track_position_s': (m['a_rec'] - int(track_first[tr])) * hop_s,
               'score': m['score'], 'min_votes': m['votes'], 'windows': m['windows']}
        result_matches.append(row)
        print(f'{os.path.basename(row["recording"])[-32:]:<32s} {row["recording_span_s"][0]:8.1f} {row["recording_span_s"][1]:8.1f}  '
              f'{os.path.basename(row["track"])[-32:]:<32s} {row["track_position_s"]:9.1f} {row["score"]:7.4f} {row["min_votes"]:5d} '
              f'{row["windows"]:4d}')
    matched = {m['rec'] for m in matches}
    for r, f in enumerate(files):
        if r not in matched:
            print(f'{os.path.basename(f)[-32:]:<32s} no match')
    requested = getattr(index, 'requested_type', index_type)
    used = index.index_description if hasattr(index, 'index_description') else 'L2 (exact, HIP FlatL2Index)'
    result = {'index_type_requested': requested, 'index_type_used': used, 'k_probe': int(k_probe), 'window': int(window),
              'window_hop': int(window_hop), 'min_overlap': int(min_overlap), 'min_votes': int(min_votes), 'n_short': int(n_short),
              'min_score': None if min_score is None else float(min_score), 'align_tol': int(align_tol), 'hop_s': hop_s,
              'duration_s': dur_s, 'recordings': files, 'n_windows': int(len(rec)), 'matches': result_matches}
    out_path = output or f'{emb_dir}identify.json'
    with open(out_path, 'w') as f:
        json.dump(result, f, indent=1)
    print(f'Saved {len(result_matches)} matches to {out_path}.')
    return result
