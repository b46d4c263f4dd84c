"""TEST INFRASTRUCTURE: the contract of nafp_search_identify (include/nafp.h), steps 1 to 6, restated in numpy.

  1. candidates  slot (i < len_t, j < k) with id = topk_ids[q0 + i, j] in [0, n_index): tr = the track with first[tr] <= id <
                 first[tr + 1], a = id - i (any sign); a candidate is a distinct pair (tr, a);
  2. votes       v(tr, a) = the number of slots that gave the pair;
  3. overlap     i0 = max(0, first[tr] - a), i1 = min(len_t, first[tr + 1] - a), n_ov = i1 - i0; dropped if n_ov < min(min_overlap,
                 len_t) or v < min_votes;
  4. shortlist   the n_short best by votes descending, track ascending, a ascending; n_cand counts the survivors of 3 before the cut;
  5. score       one float32 per shortlisted candidate, from the CALLBACK `score_fn(q_start, n_ov, cand)` (three int arrays over all
                 tasks' shortlists at once -> float32 array): mean_{i < n_ov} query[q_start + i] . index[cand + i] with q_start =
                 q0 + i0, cand = a + i0.  The restatement ranks by exactly the values it is given, so a test can hand it the bits of
                 nafp_search_seq_scores (the yardstick on the GPU) or `score_f64` below; NaN and -inf drop the candidate;
  6. rank        score descending, track ascending, a ascending; the n_out best; padding track -1, align 0, score -inf, votes 0,
                 overlap 0.
len_t = min(task_len[t], max_len, n_query - q0); a task with q0 outside [0, n_query) or len_t <= 0 has no candidates."""
import numpy as np


def effective_len(task_q0, task_len, max_len, n_query):
    q0 = int(task_q0)
    if q0 < 0 or q0 >= n_query:
        return 0
    return max(0, min(int(task_len), int(max_len), n_query - q0))


def shortlist(topk_ids, q0, length, n_index, first, min_overlap, min_votes, n_short):
    """Steps 1 to 4 of one task: (rows (m, 5) int64 = [track, a, votes, i0, n_ov] in shortlist order, n_cand)."""
    empty = np.zeros((0, 5), np.int64)
    if length <= 0:
        return empty, 0
    first = np.asarray(first, np.int64)
    I = np.asarray(topk_ids[q0:q0 + length], dtype=np.int64)
    i = np.broadcast_to(np.arange(length)[:, None], I.shape)
    present = (I >= 0) & (I < n_index)
    ids, seg = I[present], i[present]
    if not len(ids):
        return empty, 0
    tr = np.searchsorted(first, ids, side='right') - 1
    pairs, votes = np.unique(np.stack([tr, ids - seg], 1), axis=0, return_counts=True)
    tr, a = pairs[:, 0], pairs[:, 1]
    i0 = np.maximum(0, first[tr] - a)
    n_ov = np.minimum(length, first[tr + 1] - a) - i0
    keep = (n_ov >= min(min_overlap, length)) & (votes >= min_votes)
    rows = np.stack([tr, a, votes, i0, n_ov], 1)[keep]
    order = np.lexsort((rows[:, 1], rows[:, 0], -rows[:, 2]))
    return rows[order][:n_short], int(keep.sum())


def score_f64(query, index):
    """A `score_fn`: the float64 mean, rounded to float32 once."""
    query, index = np.asarray(query, np.float64), np.asarray(index, np.float64)

    def fn(q_start, n_ov, cand):
        out = np.empty(len(cand), np.float32)
        with np.errstate(invalid='ignore', over='ignore'):
            for n, (q, l, c) in enumerate(zip(q_start, n_ov, cand)):
                out[n] = np.float32((query[q:q + l] * index[c:c + l]).sum() / l)
        return out
    return fn


def identify(topk_ids, task_q0, task_len, max_len, n_query, n_index, first, score_fn, min_overlap=4, min_votes=2, n_short=32, n_out=1):
    """dict of track, align, score, votes, overlap (T, n_out) and n_cand (T,); plus `scored`: per task the (rows, scores) of its
    shortlist as they were scored (what a test needs to compare the scores with another arithmetic)."""
    T = len(task_q0)
    lists, n_cand = [], np.zeros(T, np.int32)
    for t in range(T):
        length = effective_len(task_q0[t], task_len[t], max_len, n_query)
        rows, n_cand[t] = shortlist(topk_ids, int(task_q0[t]), length, n_index, first, min_overlap, min_votes, n_short)
        lists.append(rows)
    sizes = [len(r) for r in lists]
    allr = np.concatenate(lists) if sum(sizes) else np.zeros((0, 5), np.int64)
    q0_of = np.repeat(np.asarray(task_q0, np.int64), sizes)
    scores = np.asarray(score_fn(q0_of + allr[:, 3], allr[:, 4], allr[:, 1] + allr[:, 3]), np.float32) if len(allr) else np.zeros(0, np.float32)
    out = {'track': -np.ones((T, n_out), np.int32), 'align': np.zeros((T, n_out), np.int32),
           'score': np.full((T, n_out), -np.inf, np.float32), 'votes': np.zeros((T, n_out), np.int32),
           'overlap': np.zeros((T, n_out), np.int32), 'n_cand': n_cand, 'scored': []}
    at = 0
    for t in range(T):
        rows, s = lists[t], scores[at:at + sizes[t]]
        at += sizes[t]
        out['scored'].append((rows, s))
        keep = ~(np.isnan(s) | (s == -np.inf))
        rows, s = rows[keep], s[keep]
        order = np.lexsort((rows[:, 1], rows[:, 0], -s.astype(np.float64)))[:n_out]
        m = len(order)
        out['track'][t, :m], out['align'][t, :m], out['score'][t, :m] = rows[order, 0], rows[order, 1], s[order]
        out['votes'][t, :m], out['overlap'][t, :m] = rows[order, 2], rows[order, 4]
    return out
