"""TEST INFRASTRUCTURE: the contract of nafp_search_seq_match (include/nafp.h) restated in numpy, one task at a time.

  * effective length len_t = min(task_len[t], max_len, n_query - task_q0[t]); a task whose task_q0[t] is outside [0, n_query) or
    whose len_t <= 0 has no candidates;
  * candidates: the distinct c = topk_ids[task_q0[t] + i, j] - i over i < len_t, j < k with 0 <= topk_ids[..] < n_index and c >= 0
    (entries outside [0, n_index) are absent);
  * score(c) = mean over i < min(len_t, n_index - c) of query[task_q0[t] + i] . index[c + i];
  * a candidate whose score is NaN or -inf is dropped;
  * output: the n_out best by score descending, smaller id first among equal scores; padding id -1, score -inf; n_cand = the number
    of distinct candidates not dropped.

Arithmetic: the sum is formed in float64 and rounded to float32, then divided by float32(len) in float32 -- the kernel's last two
steps.  Where every product and partial sum is an integer below 2^24 (the lattice data of the tests) the float32 chain of the kernel
is exact, so this restatement gives the kernel's bits; on other data it is the kernel's value to within float32 summation error and
the tests compare with nafp_search_seq_scores instead.  `oracle.search` (the float64 evaluation loop of the reference) is the
yardstick this file is pinned to in tests/test_seq_match_host.py."""
import numpy as np

from oracle import search as S  # noqa: F401  (the pinned yardstick; `evaluate_with` below mirrors S.evaluate's bookkeeping)


def effective_len(task_q0, task_len, max_len, n_query):
    q0 = int(task_q0)
    if q0 < 0 or q0 >= n_query:
        return 0
    return max(0, min(int(task_len), int(max_len), n_query - q0))


def candidates(topk_ids, q0, length, n_index):
    """Sorted distinct compensated ids of one task."""
    if length <= 0:
        return np.zeros(0, np.int64)
    I = np.asarray(topk_ids[q0:q0 + length], dtype=np.int64)
    present = (I >= 0) & (I < n_index)
    c = I - np.arange(length)[:, None]
    return np.unique(c[present & (c >= 0)])


def score(query, index, q0, length, c):
    n = min(length, len(index) - c)
    q = np.asarray(query[q0:q0 + n], dtype=np.float64)
    x = np.asarray(index[c:c + n], dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        s = np.float32((q * x).sum())
        return np.float32(s / np.float32(n))


def seq_match(query, index, topk_ids, task_q0, task_len, max_len, n_out=10, n_index=None):
    """(ids (T, n_out) int32, scores (T, n_out) float32, n_cand (T,) int32)."""
    query, index = np.asarray(query), np.asarray(index)
    n_index = len(index) if n_index is None else int(n_index)
    index = index[:n_index]
    T = len(task_q0)
    ids = -np.ones((T, n_out), np.int32)
    scores = np.full((T, n_out), -np.inf, np.float32)
    n_cand = np.zeros(T, np.int32)
    for t in range(T):
        length = effective_len(task_q0[t], task_len[t], max_len, len(query))
        q0 = int(task_q0[t])
        c = candidates(topk_ids, q0, length, n_index)
        s = np.array([score(query, index, q0, length, int(ci)) for ci in c], np.float32)
        keep = ~(np.isnan(s) | (s == -np.inf))
        c, s = c[keep], s[keep]
        n_cand[t] = len(c)
        order = np.lexsort((c, -s.astype(np.float64)))[:n_out]        # score descending, then the smaller id
        ids[t, :len(order)] = c[order]
        scores[t, :len(order)] = s[order]
    return ids, scores, n_cand


def evaluate_with(query, index, topk_of_rows, test_ids, test_seq_len, k_probe, n_dummy):
    """oracle.search.evaluate's bookkeeping around `seq_match`: `topk_of_rows(q_rows)` -> (n, k) ids of the segment search.
    Returns the same 5-tuple."""
    n_test, n_len = len(test_ids), len(test_seq_len)
    out = [np.zeros((n_test, n_len), int) for _ in range(4)]
    preds = -np.ones((n_test, n_len, 10), np.int64)
    I = topk_of_rows(query)
    for si, sl in enumerate(test_seq_len):
        p, _, _ = seq_match(query, index, I, np.asarray(test_ids), np.full(n_test, sl), sl, 10)
        p = p.astype(np.int64)
        gt = (np.asarray(test_ids) + n_dummy)[:, None]
        preds[:, si] = p
        out[0][:, si] = (p[:, :1] == gt).any(1)
        out[1][:, si] = (np.abs(p[:, :1] - gt) <= 1).any(1) & (p[:, 0] >= 0)
        out[2][:, si] = (p[:, :3] == gt).any(1)
        out[3][:, si] = (p[:, :10] == gt).any(1)
    return out[0], out[1], out[2], out[3], preds
