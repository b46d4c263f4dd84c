"""Duplicates: which tracks does the library hold more than once.

`run.py duplicates NAME INDEX` reads the library's fingerprints ({dummy_db, db}.mm or custom_source.mm) and the row -> file tables
that `generate` writes under NAFP_TRACK_TABLE=1, exactly as `identify` does, and needs nothing else: no model, no checkpoint, no
audio.  The queries are the library's own rows, resident in HBM already (a slice of the index's device array, never a second
copy).  Searching a library with its own rows fills every row's top-k with its own track -- the row itself, its half-overlapping
neighbours, the repeats of a chorus -- so the search is `FlatL2Index.search_device_excl` (nafp_search_topk_l2_excl, include/nafp.h):
row r never takes a row of its own track [first[tr], first[tr + 1]), and that happens inside the selection, where the k survivors
are still to be had.  Only the exact index can exclude, so there is no `-i`.  Everything downstream is `identify`'s, unchanged:
`plan_windows` over the tracks, one `FlatL2Index.identify` launch per chunk (nafp_search_identify), `merge_windows`.

The library is worked in chunks of whole tracks of at most `--chunk_rows` rows (a longer track is a chunk of its own); a query's
result does not depend on what shares its launch, a window's neither, and the windows of all chunks are merged at once, so the
output does not depend on `--chunk_rows`.

A DIRECTED match X -> Y covers segments [seg0, seg1) of track X and says that X's segment s is Y's segment s + pos.  In CANONICAL
form, lo = min(X, Y), hi = max(X, Y): offset = pos if X is lo, else -pos (hi's segment = lo's segment + offset), and the span is
given in lo's segments, clipped to the segments lo has and to those whose partner hi has.  Two directed matches FOLD into one pair
when (lo, hi) are equal, the offsets differ by at most `--align_tol` and the spans overlap by more than half of the shorter one
(the rule of `select_across_speeds`).  `groups` are the connected components over the pairs with coverage >= `--min_coverage`.
`--min_coverage` and `--min_score` are the user's thresholds, as in `identify`: nobody has measured one on trained weights.
All of this is pure host code (`canonical`, `fold_matches`, `group_pairs`, `plan_chunks`)."""
import json
import os
import sys

import numpy as np

from .identify import MAX_SHORT, MAX_SLOTS, library_keys, load_track_tables, merge_windows, plan_windows


def plan_chunks(track_first, chunk_rows):
    """[(t0, t1)]: consecutive runs of whole tracks [t0, t1) of at most chunk_rows rows each; a longer track is a run of its own."""
    first = np.asarray(track_first, np.int64)
    chunk_rows = int(chunk_rows)
    if chunk_rows < 1:
        raise ValueError('plan_chunks: chunk_rows >= 1')
    out, t0 = [], 0
    n_tracks = len(first) - 1
    while t0 < n_tracks:
        t1 = t0 + 1
        while t1 < n_tracks and first[t1 + 1] - first[t0] <= chunk_rows:
            t1 += 1
        out.append((t0, t1))
        t0 = t1
    return out


def canonical(x, y, seg0, seg1, pos, n_seg):
    """The directed match x -> y over segments [seg0, seg1) of x with y's segment = x's segment + pos, in canonical form:
    (lo, hi, offset, s0, s1, direction) with the span [s0, s1) in lo's segments, clipped to lo's segments and to those whose
    partner lo's segment + offset is a segment of hi; direction 0: x is lo, 1: x is hi.  n_seg: the segments of each track.
    s1 <= s0 means that nothing is left."""
    x, y, pos = int(x), int(y), int(pos)
    if x == y:
        raise ValueError('canonical: a track is no duplicate of itself')
    if x < y:
        lo, hi, offset, s0, s1, direction = x, y, pos, int(seg0), int(seg1), 0
    else:
        lo, hi, offset, s0, s1, direction = y, x, -pos, int(seg0) + pos, int(seg1) + pos, 1
    s0 = max(s0, 0, -offset)
    s1 = min(s1, int(n_seg[lo]), int(n_seg[hi]) - offset)
    return lo, hi, offset, s0, s1, direction


def fold_matches(directed, n_seg, align_tol=1):
    """directed: dicts with rec (X), track (Y), seg0, seg1, pos, score, votes, windows -> the folded pairs, ordered by
    (lo, hi, span start): dicts with lo, hi, offset, s0, s1, score (the higher), votes (the lower), windows (summed),
    directions (1 or 2), coverage (span segments over the segments of the shorter track).  The offset of a folded pair is that
    of its best-scoring member."""
    canon = []
    for m in directed:
        lo, hi, offset, s0, s1, direction = canonical(m['rec'], m['track'], m['seg0'], m['seg1'], m['pos'], n_seg)
        if s1 > s0:
            canon.append({'lo': lo, 'hi': hi, 'offset': offset, 's0': s0, 's1': s1, 'score': float(m['score']), 'votes': int(m['votes']),
                          'windows': int(m['windows']), '_dirs': {direction}})
    canon.sort(key=lambda c: (c['lo'], c['hi'], c['s0'], c['s1'], c['offset'], min(c['_dirs'])))
    pairs = []
    for c in canon:
        for p in pairs:
            if (p['lo'], p['hi']) != (c['lo'], c['hi']) or abs(p['offset'] - c['offset']) > int(align_tol):
                continue
            if min(p['s1'], c['s1']) - max(p['s0'], c['s0']) > 0.5 * min(p['s1'] - p['s0'], c['s1'] - c['s0']):
                if c['score'] > p['score']:
                    p['offset'], p['score'] = c['offset'], c['score']
                p['s0'], p['s1'] = min(p['s0'], c['s0']), max(p['s1'], c['s1'])
                p['votes'] = min(p['votes'], c['votes'])
                p['windows'] += c['windows']
                p['_dirs'] |= c['_dirs']
                break
        else:
            pairs.append(dict(c, _dirs=set(c['_dirs'])))
    for p in pairs:
        p['directions'] = len(p.pop('_dirs'))
        p['coverage'] = (p['s1'] - p['s0']) / float(min(int(n_seg[p['lo']]), int(n_seg[p['hi']])))
    return sorted(pairs, key=lambda p: (p['lo'], p['hi'], p['s0']))


def group_pairs(pairs, min_coverage=0.0):
    """The connected components (union-find) over the pairs with coverage >= min_coverage: sorted lists of track indices,
    singletons omitted, ordered by their first member."""
    parent = {}

    def find(a):
        parent.setdefault(a, a)
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for p in pairs:
        if p['coverage'] >= float(min_coverage):
            a, b = find(p['lo']), find(p['hi'])
            if a != b:
                parent[max(a, b)] = min(a, b)
    groups = {}
    for a in parent:
        groups.setdefault(find(a), []).append(a)
    return sorted(sorted(g) for g in groups.values() if len(g) > 1)


def match_library(flat, track_first, window=20, window_hop=10, k_probe=20, min_overlap=4, min_votes=2, n_short=32, chunk_rows=1 << 20):
    """The self-join: per chunk one masked search of the chunk's rows (own track excluded) and one nafp_search_identify launch over
    the chunk's windows.  Returns (rec, s0, length, track, align, score, votes) numpy arrays over the windows of ALL tracks, tracks
    in order: `rec` is the track a window belongs to, the rest as `merge_windows` takes them."""
    import torch
    first = np.asarray(track_first, np.int32)
    out = [[] for _ in range(7)]
    for t0, t1 in plan_chunks(first, chunk_rows):
        r0, r1 = int(first[t0]), int(first[t1])
        q = flat._x[r0:r1]                                          # the resident rows themselves: a view, no second copy
        own = np.repeat(np.stack([first[t0:t1], first[t0 + 1:t1 + 1]], 1), np.diff(first[t0:t1 + 1]), axis=0)
        excl = torch.from_numpy(np.ascontiguousarray(own, dtype=np.int32)).to(flat.device)
        _, ids = flat.search_device_excl(q, int(k_probe), excl)
        rec, s0, ln = plan_windows(np.diff(first[t0:t1 + 1]), window, window_hop)
        q0 = torch.from_numpy((first[t0 + rec] - r0 + s0).astype(np.int32)).to(flat.device)
        tl = torch.from_numpy(ln.astype(np.int32)).to(flat.device)
        track, align, score, votes, _, _ = flat.identify(q, ids, q0, tl, first, n_out=1, n_short=int(n_short), min_overlap=int(min_overlap),
                                                         min_votes=int(min_votes), max_len=int(window))
        for dst, v in zip(out, (rec + t0, s0, ln, track[:, 0].cpu().numpy(), align[:, 0].cpu().numpy(), score[:, 0].cpu().numpy(),
                                votes[:, 0].cpu().numpy())):
            dst.append(v)
    return tuple(np.concatenate(v) for v in out)


def pairs_from_windows(rec, s0, length, track, align, score, votes, track_first, min_score=None, align_tol=1):
    """Per-window results of `match_library` -> (directed matches, folded pairs).  A window's alignment is a row of the library;
    merge_windows' a_rec is the library row that segment 0 of track X falls on, so pos = a_rec - first[Y]."""
    first = np.asarray(track_first, np.int64)
    directed = []
    for m in merge_windows(rec, s0, length, track, align, score, votes, min_score, align_tol):
        directed.append({'rec': m['rec'], 'track': m['track'], 'seg0': m['seg0'], 'seg1': m['seg1'], 'pos': m['a_rec'] - int(first[m['track']]),
                         'score': m['score'], 'votes': m['votes'], 'windows': m['windows']})
    return directed, fold_matches(directed, np.diff(first), align_tol)


def check_arguments(window, window_hop, k_probe, min_overlap, min_votes, n_short, align_tol, min_coverage, chunk_rows):
    """The refusals that need no file, each by name; before any GPU call."""
    if not 1 <= int(k_probe) <= 32:
        sys.exit(f'duplicates: --k_probe {k_probe} is outside 1..32, the results the search keeps per row')
    if int(window) < 1 or int(window_hop) < 1:
        sys.exit('duplicates: --window and --window_hop >= 1')
    if int(window) * int(k_probe) > MAX_SLOTS:
        sys.exit(f'duplicates: --window {window} x --k_probe {k_probe} = {int(window) * int(k_probe)} slots per window; the matcher '
                 f'(nafp_search_identify) takes at most {MAX_SLOTS}')
    if not 1 <= int(n_short) <= MAX_SHORT:
        sys.exit(f'duplicates: --n_short {n_short} is outside 1..{MAX_SHORT}')
    if int(min_overlap) < 1 or int(min_votes) < 1 or int(align_tol) < 0:
        sys.exit('duplicates: --min_overlap and --min_votes >= 1, --align_tol >= 0')
    if int(chunk_rows) < 1:
        sys.exit('duplicates: --chunk_rows >= 1')
    if not float(min_coverage) >= 0:
        sys.exit('duplicates: --min_coverage >= 0')


def duplicates(cfg, checkpoint_name, checkpoint_index, window=20, window_hop=10, k_probe=20, min_overlap=4, min_votes=2, n_short=32,
               min_score=None, align_tol=1, min_coverage=0.0, chunk_rows=1 << 20, output=None, emb_dir=None):
    """`run.py duplicates`.  Returns the dict written to duplicates.json."""
    check_arguments(window, window_hop, k_probe, min_overlap, min_votes, n_short, align_tol, min_coverage, chunk_rows)
    from .eval_faiss import FlatL2Index, load_memmap_data
    if emb_dir is None:
        emb_dir = f"{cfg['DIR']['OUTPUT_ROOT_DIR']}{checkpoint_name}/{checkpoint_index}/"
    keys = library_keys(emb_dir)
    for key in keys:
        if not os.path.exists(f'{emb_dir}{key}.mm') or not os.path.exists(f'{emb_dir}{key}_shape.npy'):
            sys.exit(f'duplicates: {emb_dir}{key}.mm is missing; run `generate` first')
        if not os.path.exists(f'{emb_dir}{key}_tracks.json'):
            sys.exit(f'duplicates: {emb_dir}{key}_tracks.json is missing.  The track table maps fingerprint rows to files; write it by '
                     'running `generate` with NAFP_TRACK_TABLE=1 in the environment.')
    shapes = [load_memmap_data(emb_dir, key, shape_only=True) for key in keys]
    track_files, track_first, hop_s, dur_s = load_track_tables(emb_dir, keys, shapes)
    n_tracks = len(track_files)
    if n_tracks < 2:
        sys.exit(f'duplicates: the library holds {n_tracks} track; two are needed for a duplicate')

    parts = [load_memmap_data(emb_dir, key)[0] for key in keys]     # the first GPU call is below this line
    flat = FlatL2Index(int(parts[0].shape[1]))
    for p in parts:
        flat.add(p)
    print(f'duplicates: {flat.ntotal} library rows in {n_tracks} tracks')
    win = match_library(flat, track_first, window, window_hop, k_probe, min_overlap, min_votes, n_short, chunk_rows)
    _, folded = pairs_from_windows(*win, track_first, min_score, align_tol)

    n_seg = np.diff(track_first.astype(np.int64))
    span_s = lambda a, b: [a * hop_s, (b - 1) * hop_s + dur_s]
    pairs = []
    for p in folded:
        lo, hi, off = p['lo'], p['hi'], p['offset']
        b0, b1 = max(p['s0'] + off, 0), min(p['s1'] + off, int(n_seg[hi]))
        pairs.append({'a': track_files[lo], 'a_index': lo, 'b': track_files[hi], 'b_index': hi, 'a_span_s': span_s(p['s0'], p['s1']),
                      'b_span_s': span_s(b0, b1), 'offset_s': off * hop_s, 'score': p['score'], 'min_votes': p['votes'],
                      'windows': p['windows'], 'directions': p['directions'], 'coverage': p['coverage']})
    groups = [{'tracks': g, 'files': [track_files[t] for t in g]} for g in group_pairs(folded, min_coverage)]

    print(f'{"a":<30s} {"from":>8s} {"to":>8s}  {"b":<30s} {"from":>8s} {"to":>8s} {"offset":>8s} {"score":>8s} {"votes":>5s} {"win":>4s} {"dir":>3s} {"cover":>6s}')
    for row in pairs:
        print(f'{os.path.basename(row["a"])[-30:]:<30s} {row["a_span_s"][0]:8.1f} {row["a_span_s"][1]:8.1f}  '
              f'{os.path.basename(row["b"])[-30:]:<30s} {row["b_span_s"][0]:8.1f} {row["b_span_s"][1]:8.1f} {row["offset_s"]:8.1f} '
              f'{row["score"]:8.4f} {row["min_votes"]:5d} {row["windows"]:4d} {row["directions"]:3d} {row["coverage"]:6.3f}')
    for n, g in enumerate(groups):
        print(f'group {n}: ' + ', '.join(os.path.basename(f) for f in g['files']))
    result = {'index_type_used': 'L2 (exact, HIP FlatL2Index, own track excluded)', 'k_probe': int(k_probe), 'window': int(window),
              'window_hop': int(window_hop), 'min_overlap': int(min_overlap), 'min_votes': int(min_votes), 'n_short': int(n_short),
              'min_score': None if min_score is None else float(min_score), 'align_tol': int(align_tol),
              'min_coverage': float(min_coverage), 'hop_s': hop_s, 'duration_s': dur_s, 'n_rows': int(flat.ntotal), 'n_tracks': n_tracks,
              'n_windows': int(len(win[0])), 'pairs': pairs, 'groups': groups}
    out_path = output or f'{emb_dir}duplicates.json'
    with open(out_path, 'w') as f:
        json.dump(result, f, indent=1)
    print(f'Saved {len(pairs)} pairs in {len(groups)} groups to {out_path}.')
    return result
