"""float64 numpy restatement of the HNSW contract (include/nafp.h "HNSW", neural-audio-fp_amd/eval/hnsw.py, csrc/hnsw.hip):
the level draws, the round bounds, the bounded-pool layer search, the neighbour selection, one round, the whole build and the
search.  Every ordering is by the pair (squared L2 distance, id) ascending.  Link lists are kept for every row on every level
(`links[level]` is (n, M_level) int64, -1 padded): the compact upper-level storage of the device index is a layout, not part of
the contract."""
import numpy as np

M = 16
MAX_LEVEL = 7
STREAM_HNSW_LEVEL = 7
ROUND_CAP = 16384


def degree(level, m=M):
    return 2 * m if level == 0 else m


def default_max_expansions(ef):
    return 4 * int(ef) + 256


def draw_levels(seed, n0, n1, m=M):
    """Levels of rows n0 .. n1 - 1: row i gets min(MAX_LEVEL, floor(-ln(u_i) / ln(M))), u_i the i-th draw of the stream."""
    u = np.random.default_rng([int(seed), STREAM_HNSW_LEVEL]).random(int(n1))[int(n0):]
    with np.errstate(divide='ignore'):
        lv = np.floor(-np.log(u) / np.log(float(m)))
    return np.minimum(lv, MAX_LEVEL).astype(np.int32)


def round_bounds(n_inserted, ntotal):
    """[(s, e)] of the rounds that take the graph from n_inserted to ntotal rows."""
    out, s = [], int(n_inserted)
    while s < ntotal:
        e = min(int(ntotal), s + min(max(1, s // 8), ROUND_CAP))
        out.append((s, e))
        s = e
    return out


def entry_point(levels, n):
    """(ep, L): the row of highest level among the first n, the smallest id among equals; (-1, -1) for n = 0."""
    if n == 0:
        return -1, -1
    ep = int(np.argmax(levels[:n]))                 # argmax keeps the first
    return ep, int(levels[ep])


def search_layer(x, links, q, entry, ef, max_expansions=None):
    """[(distance, id)] in order, at most ef of them.  links: (n, deg), -1 padded."""
    if entry < 0:
        return []
    cap = default_max_expansions(ef) if max_expansions is None else int(max_expansions)
    q = np.asarray(q, np.float64)
    pool = [(float(((x[entry] - q) ** 2).sum()), int(entry))]
    inpool, expanded = {int(entry)}, set()
    for _ in range(cap):
        c = next((p for p in pool if p[1] not in expanded), None)
        if c is None:
            break
        expanded.add(c[1])
        nb = [int(j) for j in dict.fromkeys(links[c[1]].tolist()) if j >= 0 and j not in inpool]
        if nb:
            dist = ((x[nb] - q) ** 2).sum(1)
            pool = sorted(pool + list(zip(dist.tolist(), nb)))[:ef]
            inpool = {p[1] for p in pool}
    return pool


def select(x, owner, cands, m):
    """cands: [(distance to owner, id)] in order.  Accept c unless an accepted a is nearer to c than the owner is."""
    acc, seen = [], set()
    for dist, c in cands:
        if c == owner or c in seen:
            continue
        seen.add(c)
        if acc and (((x[acc] - x[c]) ** 2).sum(1) < dist).any():
            continue
        acc.append(c)
        if len(acc) == m:
            break
    return acc


def _row(ids, deg):
    out = np.full(deg, -1, np.int64)
    out[:len(ids)] = ids
    return out


class Graph:
    def __init__(self, x, levels, ef_construction=40, m=M):
        self.x = np.asarray(x, np.float64)
        self.levels = np.asarray(levels, np.int32)
        self.m, self.efc = m, int(ef_construction)
        n = len(self.x)
        self.links = [np.full((n, degree(l, m)), -1, np.int64) for l in range(MAX_LEVEL + 1)]
        self.n = 0                                   # rows inserted
        self.history = []

    @property
    def entry(self):
        return entry_point(self.levels, self.n)

    def insert_round(self, s, e):
        x, links = self.x, self.links
        ep, L = entry_point(self.levels, s)
        new = {}                                     # (row, level) -> list, applied after the round's searches: frozen graph
        for i in range(s, e):
            if ep < 0:
                break
            li, cur = int(self.levels[i]), ep
            for level in range(L, li, -1):
                cur = search_layer(x, links[level], x[i], cur, 1)[0][1]
            for level in range(min(li, L), -1, -1):
                W = search_layer(x, links[level], x[i], cur, self.efc)
                new[(i, level)] = select(x, i, W, degree(level, self.m))
                cur = W[0][1]
        incoming = {}
        for (i, level), lst in new.items():
            links[level][i] = _row(lst, degree(level, self.m))
            for j in lst:
                incoming.setdefault((j, level), []).append(i)
        self.last_round = {}                         # (old row, level) -> (new rows that chose it, size of the union)
        for (j, level), rows in incoming.items():
            deg = degree(level, self.m)
            U = [int(t) for t in links[level][j] if t >= 0] + rows
            self.last_round[(j, level)] = (len(rows), len(U))
            U = sorted(zip(((x[U] - x[j]) ** 2).sum(1).tolist(), U))
            links[level][j] = _row([c for _, c in U] if len(U) <= deg else select(x, j, U, deg), deg)
        self.n = e
        self.history.append((s, e))

    def build(self, ntotal=None):
        for s, e in round_bounds(self.n, len(self.x) if ntotal is None else ntotal):
            self.insert_round(s, e)
        return self

    def search(self, q, k, ef_search=16):
        """(D (nq, k) float64, I (nq, k) int64), padded with +inf / -1."""
        q = np.atleast_2d(np.asarray(q, np.float64))
        D = np.full((len(q), k), np.inf)
        I = np.full((len(q), k), -1, np.int64)
        ep, L = self.entry
        for r, qq in enumerate(q):
            cur = ep
            for level in range(L, 0, -1):
                cur = search_layer(self.x, self.links[level], qq, cur, 1)[0][1]
            W = search_layer(self.x, self.links[0], qq, cur, max(int(ef_search), k))[:k]
            D[r, :len(W)] = [w[0] for w in W]
            I[r, :len(W)] = [w[1] for w in W]
        return D, I

    def level_rows(self, level):
        return np.nonzero(self.levels[:self.n] >= level)[0]


def build(x, seed, ef_construction=40, levels=None):
    levels = draw_levels(seed, 0, len(x)) if levels is None else levels
    return Graph(x, levels, ef_construction).build()


def check_invariants(levels, links_of_level, n):
    """Degree bounds, lists ordered, no self or duplicate links, every target exists on that level.  links_of_level(l) ->
    (rows (n_l,), links (n_l, deg)) and dist(i, js) is not needed: order is checked by the caller where distances are known."""
    for level in range(MAX_LEVEL + 1):
        rows, lk = links_of_level(level)
        assert np.array_equal(rows, np.nonzero(levels[:n] >= level)[0])
        assert lk.shape == (len(rows), degree(level))
        for r, row in zip(rows.tolist(), lk.tolist()):
            ids = [t for t in row if t >= 0]
            assert row[:len(ids)] == ids, 'padding inside a list'
            assert r not in ids and len(set(ids)) == len(ids)
            assert all(0 <= t < n and levels[t] >= level for t in ids)


def lattice(n, d, seed, n_dup=6):
    """Integer lattice rows, coordinates uniform in {-2 .. 2}, plus n_dup exact duplicates of earlier rows (float32)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, size=(n, d)).astype(np.float32)
    for t in rng.choice(np.arange(n // 2, n), size=min(n_dup, n // 2), replace=False):
        x[t] = x[rng.integers(0, n // 2)]
    return x
