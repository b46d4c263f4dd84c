"""HNSW graph index on the device: faiss.IndexHNSWFlat as the reference builds it for evaluation (eval/utils/get_index_faiss.py:88-96:
M = 16, efConstruction = 80, efSearch = 16, search_bounded_queue), backed by libnafp's HNSW kernels (include/nafp.h "HNSW",
csrc/hnsw.hip).  Opt-in from `get_index` (NAFP_HNSW=1 next to NAFP_APPROX_INDEX=1, eval_faiss.py).  The reference builds this
index on the CPU only (faiss has no GPU HNSW); this project builds and searches it on the GPU only.

The build is DETERMINISTIC AND ROUND BASED (the contract is in include/nafp.h; tests/_hnsw_ref.py restates it in float64): levels are
drawn on the host from the index's own generator (a row's level depends on its id alone), and the graph is built lazily at the first
search after an `add`, as the IVF indexes build their lists.  Rows enter in id order in rounds [s, e), e = min(ntotal, s +
min(max(1, s // 8), 16384)) from s = the rows already inserted; a round's rows search the graph frozen at s, choose their lists, and
are then linked back from the rows they chose.  The graph therefore depends on (rows, seed, parameters) and on the row counts at which
builds happened -- `add` in pieces without a search in between equals one `add`.

faiss-shaped surface: `train` (a no-op), `is_trained`, `add`, `ntotal`, settable `efConstruction` / `efSearch` (1 .. 128), `search(q, k)`
-> (D, I) numpy, `search_device`, `device`, `reconstruct_n` / `sequence_scores` (an inner FlatL2Index keeps the fp32 rows),
`index_description`.  For tests and re-use: `levels()`, `entry_point` / `max_level`, `neighbors(level)`, `set_graph(...)`, `build()`,
`insert_round_device(...)`, `search_layer_device(...)`; and, importable without a GPU, `draw_levels`, `round_bounds`,
`default_max_expansions`.  torch only allocates, initialises and copies here.
"""
import numpy as np
import torch

from .. import _lib
from .ivf import DEFAULT_SEED, STREAM_HNSW_LEVEL, rng_for

M_LINKS = 16
MAX_LEVEL = 7
MAX_EF = 128
MAX_K = 32
ROUND_GROWTH = 8                         # a round inserts at most s // 8 rows into a graph of s rows ...
ROUND_CAP = 16384                        # ... and at most this many


def _levels_of(u, M=M_LINKS):
    with np.errstate(divide='ignore'):
        lv = np.floor(-np.log(u) / np.log(float(M)))
    return np.minimum(lv, MAX_LEVEL).astype(np.int32)


def draw_levels(seed, n0, n1, M=M_LINKS):
    """Levels of rows n0 .. n1 - 1: min(MAX_LEVEL, floor(-ln(u_i) / ln(M))), u_i the i-th draw of the seed's level stream."""
    return _levels_of(rng_for(seed, STREAM_HNSW_LEVEL).random(int(n1))[int(n0):], M)


def round_bounds(n_inserted, ntotal):
    """[(s, e)]: the rounds that take a graph of n_inserted rows to ntotal rows."""
    out, s = [], int(n_inserted)
    while s < ntotal:
        e = min(int(ntotal), s + min(max(1, s // ROUND_GROWTH), ROUND_CAP))
        out.append((s, e))
        s = e
    return out


def default_max_expansions(ef):
    """The static bound of a layer search: 4 ef + 256 expansions."""
    return 4 * int(ef) + 256


def _entry(levels, n):
    if n == 0:
        return -1, -1
    ep = int(np.argmax(levels[:n]))      # the highest level, the smallest id among equals
    return ep, int(levels[ep])


class HNSWIndex:
    """faiss.IndexHNSWFlat(d, M) with the round-based build of the module docstring.  efConstruction defaults to 40 (faiss's);
    `get_index` sets 80 as the reference does."""

    def __init__(self, d, M=M_LINKS, seed=DEFAULT_SEED, device=None):
        from .eval_faiss import FlatL2Index
        if d not in (64, 128, 256):
            raise NotImplementedError(f'fingerprint dimension {d}')
        if M != M_LINKS:
            raise NotImplementedError(f'HNSW with M = {M} (this build: M = {M_LINKS})')
        self.d, self.M, self.seed = int(d), int(M), int(seed)
        self._flat = FlatL2Index(d, device=device)              # the fp32 rows in insertion order
        self.device = self._flat.device
        self._lib = _lib.load()
        self._rng = rng_for(self.seed, STREAM_HNSW_LEVEL)       # lives in the index: a row's level depends on its id only
        self._efc, self._efs = 40, 16
        self._levels = np.zeros((0,), np.int32)                 # host copy: the entry point is found here
        self._levels_dev = self._empty((0,), torch.int32)
        self._slot = self._empty((0,), torch.int32)             # row -> its slot in _upper (-1: a row of level 0)
        self._links0 = self._empty((0, 2 * self.M), torch.int32)
        self._upper = self._empty((0, MAX_LEVEL, self.M), torch.int32)
        self._n_slots = 0
        self._n_inserted = 0

    def _empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    # ---- parameters
    @property
    def efConstruction(self):
        return self._efc

    @efConstruction.setter
    def efConstruction(self, v):
        if int(v) != v or not 1 <= int(v) <= MAX_EF:
            raise NotImplementedError(f'efConstruction = {v} (the HIP layer search keeps 1 .. {MAX_EF} pool entries)')
        self._efc = int(v)

    @property
    def efSearch(self):
        return self._efs

    @efSearch.setter
    def efSearch(self, v):
        if int(v) != v or not 1 <= int(v) <= MAX_EF:
            raise NotImplementedError(f'efSearch = {v} (the HIP layer search keeps 1 .. {MAX_EF} pool entries)')
        self._efs = int(v)

    @property
    def is_trained(self):
        return True

    def train(self, x=None):
        """Nothing to train."""

    @property
    def ntotal(self):
        return self._flat.ntotal

    @property
    def index_description(self):
        return f'HNSW (HIP; M {self.M}, efConstruction {self._efc}, efSearch {self._efs})'

    # ---- storage
    def _grow(self, t, rows, fill=None):
        """t with room for `rows` rows (doubling, as FlatL2Index._x), the old rows copied, the new ones holding `fill`."""
        if rows <= t.shape[0]:
            return t
        shape = (max(rows, 2 * t.shape[0]),) + tuple(t.shape[1:])
        grown = self._empty(shape, t.dtype) if fill is None else torch.full(shape, fill, dtype=t.dtype, device=self.device)
        grown[:t.shape[0]] = t
        return grown

    def _set_levels(self, n0, levels):
        """Rows n0 .. get these levels: host copy, device copy, and a slot each for the rows of level >= 1, in id order."""
        levels = np.asarray(levels, np.int32)
        n1 = n0 + len(levels)
        self._levels = np.concatenate([self._levels[:n0], levels])
        slot = np.full(len(levels), -1, np.int32)
        up = levels >= 1
        slot[up] = self._n_slots + np.arange(int(up.sum()), dtype=np.int32)
        self._n_slots += int(up.sum())
        self._levels_dev = self._grow(self._levels_dev, n1)
        self._slot = self._grow(self._slot, n1)
        self._links0 = self._grow(self._links0, n1, -1)
        self._upper = self._grow(self._upper, self._n_slots, -1)
        if len(levels):
            self._levels_dev[n0:n1].copy_(torch.from_numpy(levels))
            self._slot[n0:n1].copy_(torch.from_numpy(slot))

    def add(self, x):
        n0 = self.ntotal
        self._flat.add(x)
        n = self.ntotal - n0
        if n:
            self._set_levels(n0, _levels_of(self._rng.random(n), self.M))

    def levels(self):
        """(ntotal,) int32 numpy: the level of every row."""
        return self._levels.copy()

    @property
    def entry_point(self):
        """The entry row of the graph built so far (-1: none)."""
        return _entry(self._levels, self._n_inserted)[0]

    @property
    def max_level(self):
        return _entry(self._levels, self._n_inserted)[1]

    @property
    def n_inserted(self):
        return self._n_inserted

    def neighbors(self, level):
        """(ids of the inserted rows of level >= `level`, their (n_level, M_level) int32 lists on it), numpy."""
        n = self._n_inserted
        if level == 0:
            return np.arange(n), self._links0[:n].cpu().numpy()
        rows = np.nonzero(self._levels[:n] >= level)[0]
        slots = self._slot[:n].cpu().numpy()[rows]
        return rows, self._upper[:, level - 1].cpu().numpy()[slots].reshape(len(rows), self.M)

    def set_graph(self, levels, links_per_level, n_inserted=None):
        """Upload a graph built elsewhere over the rows added so far: levels (ntotal,), links_per_level[l] (ntotal, M_l) for
        l = 0 .. (rows below level l: ignored).  Every row counts as inserted, or the first n_inserted of them (the others keep
        the levels given here and enter with the next build)."""
        n = self.ntotal
        levels = np.asarray(levels, np.int32)
        if levels.shape != (n,) or levels.min(initial=0) < 0 or levels.max(initial=0) > MAX_LEVEL:
            raise ValueError(f'levels: ({n},) values 0 .. {MAX_LEVEL}')
        self._n_slots = 0
        self._links0 = self._empty((0, 2 * self.M), torch.int32)
        self._upper = self._empty((0, MAX_LEVEL, self.M), torch.int32)
        self._set_levels(0, levels)
        slots = np.cumsum(levels >= 1) - 1
        upper = np.full((max(self._n_slots, 1), MAX_LEVEL, self.M), -1, np.int32)
        for l, lk in enumerate(links_per_level):
            lk = np.asarray(lk, np.int32)
            if lk.shape != (n, 2 * self.M if l == 0 else self.M):
                raise ValueError(f'links of level {l}: ({n}, {2 * self.M if l == 0 else self.M})')
            if l == 0:
                if n:
                    self._links0[:n].copy_(torch.from_numpy(np.ascontiguousarray(lk)))
            else:
                rows = np.nonzero(levels >= l)[0]
                upper[slots[rows], l - 1] = lk[rows]
        if self._n_slots:
            self._upper[:self._n_slots].copy_(torch.from_numpy(upper[:self._n_slots]))
        self._n_inserted = n if n_inserted is None else int(n_inserted)
        if not 0 <= self._n_inserted <= n:
            raise ValueError(f'n_inserted = {n_inserted} of {n} rows')

    # ---- the kernels
    def _level_args(self, level):
        """(links pointer, slot pointer, n_link_rows, link_stride) of one level (include/nafp.h)."""
        if level == 0:
            return _lib.ptr(self._links0), None, self._links0.shape[0], 2 * self.M
        if self._upper.shape[0] == 0:
            raise ValueError(f'no row of level {level}')
        return (_lib.c_void_p(self._upper.data_ptr() + (level - 1) * self.M * 4), _lib.ptr(self._slot), self._upper.shape[0],
                MAX_LEVEL * self.M)

    def _search_layer(self, q, nq, entries, q_levels, ef, level, max_expansions, n_rows, D, I, n_out):
        links, slot, n_link_rows, stride = self._level_args(level)
        _lib.check(self._lib.nafp_hnsw_search_layer(_lib.ptr(self._flat._x), n_rows, self.d, links, slot, n_link_rows, stride, self.M,
                                                    level, q, nq, _lib.ptr(entries), _lib.ptr(q_levels), ef, max_expansions, n_out,
                                                    _lib.ptr(D), _lib.ptr(I), _lib.current_stream()), 'hnsw_search_layer')

    def search_layer_device(self, q, entries, ef, level, max_expansions=None):
        """The layer search of `level` over the graph as it stands: q (nq, d) CUDA, entries (nq,) row ids -> (D, I) (nq, ef) CUDA,
        in order, padded with +inf / -1."""
        q = _lib.require_cuda(q, 'q').float().contiguous()
        if not 1 <= int(ef) <= MAX_EF or not 0 <= int(level) <= MAX_LEVEL:
            raise NotImplementedError(f'ef = {ef}, level = {level} (1 .. {MAX_EF}, 0 .. {MAX_LEVEL})')
        ent = torch.as_tensor(np.asarray(entries) if not torch.is_tensor(entries) else entries).to(device=self.device, dtype=torch.int32).contiguous()
        nq = q.shape[0]
        if ent.shape != (nq,):
            raise ValueError('one entry per query')
        cap = default_max_expansions(ef) if max_expansions is None else int(max_expansions)
        D, I = self._empty((nq, int(ef)), torch.float32), self._empty((nq, int(ef)), torch.int32)
        with torch.cuda.device(self.device):
            self._search_layer(_lib.ptr(q), nq, ent, None, int(ef), int(level), cap, self._n_inserted, D, I, int(ef))
        return D, I

    def insert_round_device(self, s=None, e=None):
        """One round: rows [s, e) into the graph of the rows < s (s = the rows inserted so far; e defaults to the round's bound)."""
        s = self._n_inserted if s is None else int(s)
        if s != self._n_inserted:
            raise ValueError(f'a round starts at the {self._n_inserted} rows already inserted')
        e = round_bounds(s, self.ntotal)[0][1] if e is None else int(e)
        if not s < e <= self.ntotal:
            raise ValueError(f'round [{s}, {e}) of {self.ntotal} rows')
        ep, L = _entry(self._levels, s)
        n_new, lib, x = e - s, self._lib, self._flat._x
        if ep >= 0:
            top_new = int(self._levels[s:e].max())
            new_levels = self._levels_dev[s:e]
            q = _lib.c_void_p(x.data_ptr() + s * self.d * 4)
            with torch.cuda.device(self.device):
                cur = torch.from_numpy(np.full(n_new, ep, np.int32)).to(self.device)
                Wd, Wi = self._empty((n_new * self._efc,), torch.float32), self._empty((n_new * self._efc,), torch.int32)
                for level in range(L, -1, -1):
                    ef = self._efc if level <= top_new else 1          # above every new row's level: the descent only
                    D, I = Wd[:n_new * ef].view(n_new, ef), Wi[:n_new * ef].view(n_new, ef)
                    self._search_layer(q, n_new, cur, new_levels, ef, level, default_max_expansions(ef), s, D, I, ef)
                    if level <= top_new:
                        links, slot, n_link_rows, stride = self._level_args(level)
                        _lib.check(lib.nafp_hnsw_select_forward(_lib.ptr(x), e, self.d, s, n_new, _lib.ptr(new_levels), level, self.M,
                                                                _lib.ptr(D), _lib.ptr(I), ef, links, slot, n_link_rows, stride,
                                                                _lib.current_stream()), 'hnsw_select_forward')
                    cur = I[:, 0].clone()                                  # its own buffer: the next level's output overwrites Wi while blocks still read their entries
                for level in range(min(top_new, L), -1, -1):
                    need = int(lib.nafp_hnsw_reverse_workspace_bytes(s, n_new, self.M, level))
                    if need < 0:
                        raise NotImplementedError(f'a round of {n_new} rows into {s}')
                    ws = self._empty((need,), torch.uint8)
                    links, slot, n_link_rows, stride = self._level_args(level)
                    _lib.check(lib.nafp_hnsw_reverse_links(_lib.ptr(x), e, self.d, s, n_new, _lib.ptr(new_levels), level, self.M, links,
                                                           slot, n_link_rows, stride, _lib.ptr(ws), need, _lib.current_stream()),
                               'hnsw_reverse_links')
        self._n_inserted = e

    def build(self):
        """Insert the rows added since the last build (lazily called by the searches)."""
        for s, e in round_bounds(self._n_inserted, self.ntotal):
            self.insert_round_device(s, e)
        return self

    def search_device(self, q, k):
        """q: (nq, d) CUDA float32 -> (D, I) CUDA tensors (float32, int32)."""
        q = _lib.require_cuda(q, 'q').float().contiguous()
        if k > MAX_K or k < 1:
            raise NotImplementedError(f'k = {k} (the HIP search keeps k <= {MAX_K} results per query)')
        if self.ntotal == 0:
            raise ValueError('empty index')
        self.build()
        ep, L = _entry(self._levels, self._n_inserted)
        nq, lib = q.shape[0], self._lib
        D, I = self._empty((nq, k), torch.float32), self._empty((nq, k), torch.int32)
        need = int(lib.nafp_hnsw_search_workspace_bytes(nq, self._efs, int(k)))
        ws = self._empty((need,), torch.uint8)
        with torch.cuda.device(self.device):
            _lib.check(lib.nafp_hnsw_search(_lib.ptr(self._flat._x), self._n_inserted, self.d, _lib.ptr(self._links0),
                                            _lib.ptr(self._upper) if self._n_slots else None, _lib.ptr(self._slot), self._upper.shape[0],
                                            self.M, ep, L, _lib.ptr(q), nq, self._efs, int(k), _lib.ptr(D), _lib.ptr(I), _lib.ptr(ws),
                                            need, _lib.current_stream()), 'hnsw_search')
        return D, I

    def search(self, q, k):
        """faiss signature: numpy in, (D float32, I int64) numpy out."""
        qd = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(self.device)
        D, I = self.search_device(qd, k)
        return D.cpu().numpy(), I.cpu().numpy().astype(np.int64)

    def reconstruct_n(self, i0, n):
        return self._flat.reconstruct_n(i0, n)

    def sequence_scores(self, q, task_q0, task_len, cand):
        """Scores from the original fp32 rows in insertion order (FlatL2Index.sequence_scores)."""
        return self._flat.sequence_scores(q, task_q0, task_len, cand)

    def sequence_match(self, q, topk_ids, task_q0, task_len, n_out=10, max_len=None):
        """Ranked sequence candidates from the original fp32 rows in insertion order (FlatL2Index.sequence_match)."""
        return self._flat.sequence_match(q, topk_ids, task_q0, task_len, n_out=n_out, max_len=max_len)
