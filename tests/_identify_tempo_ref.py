"""TEST INFRASTRUCTURE: the contract of nafp_search_identify_tempo (include/nafp.h) restated in numpy.

  hypotheses  rho[r], 16.16 fixed point: the library rows advanced per query segment; off_r(i) = (i * rho[r] + 32768) >> 16;
  candidates  slot (i < len_t, j < k) with id = topk_ids[q0 + i, j] in [0, n_index) gives, for EVERY r, the triple (tr, r, a):
              tr the track of id, a = id - off_r(i) (any sign); a candidate is a distinct triple, counted with a dictionary;
  overlap     by brute force over i: i0 = the smallest i with a + off_r(i) >= first[tr], i1 the smallest with a + off_r(i) >=
              first[tr + 1], len_t where there is none, the track clipped to [0, n_index); n_ov = i1 - i0; dropped if n_ov <
              min(min_overlap, len_t), n_ov == 0 or votes < min_votes;
  shortlist   the n_short best by votes descending, then tr, r, a ascending; n_cand counts the survivors before the cut;
  score       one float32 per shortlisted candidate from the CALLBACK `score_fn(q_start, n_ov, rows)`: q_start and n_ov int arrays
              over all tasks' shortlists, rows a list of int arrays, rows[n] = a + off_r(i) for i0 <= i < i1: the mean of
              query[q_start + m] . index[rows[n][m]].  The restatement ranks by exactly the values it is given (the bits of
              nafp_search_seq_scores on the gathered rows on the GPU, `score_f64` below on the host); NaN and -inf drop the candidate;
  rank        score descending, then tr, r, a ascending; the n_out best; padding track -1, align 0, rho -1, score -inf, votes 0,
              overlap 0.
len_t is that of tests/_identify_ref.py."""
import numpy as np

from _identify_ref import effective_len

ONE = 1 << 16


def off(i, rho):
    return (np.asarray(i, np.int64) * int(rho) + 32768) >> 16


def overlap(a, rho, length, lo, hi):
    """(i0, i1) of alignment a under rho against the rows [lo, hi), by brute force over i."""
    rows = a + off(np.arange(length), rho)
    at = lambda bound: int(np.argmax(rows >= bound)) if (rows >= bound).any() else length
    i0 = at(lo)
    return i0, max(i0, at(hi))


def shortlist(topk_ids, q0, length, n_index, first, rhos, min_overlap, min_votes, n_short):
    """One task up to the shortlist: (rows (m, 6) int64 = [track, r, a, votes, i0, n_ov] in shortlist order, n_cand)."""
    empty = np.zeros((0, 6), np.int64)
    if length <= 0:
        return empty, 0
    first = [int(v) for v in first]
    votes = {}
    for i in range(length):
        offs = [int(off(i, rho)) for rho in rhos]
        for idx in topk_ids[q0 + i]:
            idx = int(idx)
            if 0 <= idx < n_index:
                tr = int(np.searchsorted(first, idx, side='right')) - 1
                for r, o in enumerate(offs):
                    votes[(tr, r, idx - o)] = votes.get((tr, r, idx - o), 0) + 1
    rows = []
    for (tr, r, a), v in votes.items():
        i0, i1 = overlap(a, rhos[r], length, max(first[tr], 0), min(first[tr + 1], n_index))
        n_ov = i1 - i0
        if n_ov >= min(min_overlap, length) and n_ov > 0 and v >= min_votes:
            rows.append((tr, r, a, v, i0, n_ov))
    rows.sort(key=lambda c: (-c[3], c[0], c[1], c[2]))
    return np.asarray(rows[:n_short], np.int64).reshape(-1, 6), len(rows)


def score_f64(query, index):
    """A `score_fn`: the float64 mean, rounded to float32 once."""
    query, index = np.asarray(query, np.float64), np.asarray(index, np.float64)

    def fn(q_start, n_ov, rows):
        out = np.empty(len(rows), np.float32)
        with np.errstate(invalid='ignore', over='ignore'):
            for n, (q, l, rw) in enumerate(zip(q_start, n_ov, rows)):
                out[n] = np.float32((query[q:q + l] * index[rw]).sum() / l)
        return out
    return fn


def identify(topk_ids, task_q0, task_len, max_len, n_query, n_index, first, rhos, score_fn, min_overlap=4, min_votes=2, n_short=32,
             n_out=1):
    """dict of track, align, rho, score, votes, overlap (T, n_out) and n_cand (T,); plus `scored`: per task the (rows, scores) of
    its shortlist as they were scored."""
    T = len(task_q0)
    rhos = [int(v) for v in rhos]
    lists, n_cand = [], np.zeros(T, np.int32)
    for t in range(T):
        length = effective_len(task_q0[t], task_len[t], max_len, n_query)
        rows, n_cand[t] = shortlist(topk_ids, int(task_q0[t]), length, n_index, first, rhos, min_overlap, min_votes, n_short)
        lists.append(rows)
    sizes = [len(r) for r in lists]
    allr = np.concatenate(lists) if sum(sizes) else np.zeros((0, 6), np.int64)
    q0_of = np.repeat(np.asarray(task_q0, np.int64), sizes)
    gathered = [c[2] + off(np.arange(c[4], c[4] + c[5]), rhos[c[1]]) for c in allr]
    scores = np.asarray(score_fn(q0_of + allr[:, 4], allr[:, 5], gathered), np.float32) if len(allr) else np.zeros(0, np.float32)
    out = {'track': -np.ones((T, n_out), np.int32), 'align': np.zeros((T, n_out), np.int32), 'rho': -np.ones((T, n_out), np.int32),
           'score': np.full((T, n_out), -np.inf, np.float32), 'votes': np.zeros((T, n_out), np.int32),
           'overlap': np.zeros((T, n_out), np.int32), 'n_cand': n_cand, 'scored': []}
    at = 0
    for t in range(T):
        rows, s = lists[t], scores[at:at + sizes[t]]
        at += sizes[t]
        out['scored'].append((rows, s))
        keep = ~(np.isnan(s) | (s == -np.inf))
        rows, s = rows[keep], s[keep]
        order = np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0], -s.astype(np.float64)))[:n_out]
        m = len(order)
        out['track'][t, :m], out['rho'][t, :m], out['align'][t, :m], out['score'][t, :m] = rows[order, 0], rows[order, 1], rows[order, 2], s[order]
        out['votes'][t, :m], out['overlap'][t, :m] = rows[order, 3], rows[order, 5]
    return out
