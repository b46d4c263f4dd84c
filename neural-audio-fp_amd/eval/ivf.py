"""IVF-Flat and IVF-PQ indexes on the device: faiss.IndexIVFFlat / faiss.IndexIVFPQ as the reference builds them for
evaluation (eval/utils/get_index_faiss.py:64-80, nprobe = 40 at :120), backed by libnafp's IVF kernels (include/nafp.h
"Approximate indexes", csrc/ivf.hip).  Opt-in from `get_index` (NAFP_APPROX_INDEX=1, eval_faiss.py).

faiss-shaped surface: `train(x)`, `is_trained`, `add(x)` (repeatedly), `ntotal`, a settable `nprobe`, `search(q, k)` ->
(D, I) numpy, `search_device`; plus what the evaluation needs (`device`, `sequence_scores`, `reconstruct_n`: the original fp32
rows in insertion order, kept in a FlatL2Index -- the reference's `fake_recon_index`) and, for tests and re-use, `centroids`,
`pq_centroids`, `probe_device(q)` and `set_params(...)` / explicit k-means initialisations in `train`.  IVF-PQ has a settable
`lut` ('f32', the default, or 'f16': the ADC tables rounded to binary16 as the reference's GPU index keeps them) and
`adc_tables(q, pair_query, pair_list)`, the tables themselves.  `IVFPQRIndex` (faiss.IndexIVFPQR, 'ivfpq-rr' with NAFP_IVFPQ_RR=1)
adds refine codes and a re-ranking of k * k_factor first-stage candidates: `refine_centroids`, `refine_codes()`, `k_factor`,
`search_stages(q, k)`.

Training is modelled on faiss's CPU defaults (documentation and source as publicly known; faiss is not a dependency, so this is
the project's contract rather than a checked copy).  Every constant of it is below.  torch only allocates and copies here; the
k-means empty-cluster split is tiny and sequential and runs on the host (numpy).
"""
import numpy as np
import torch

from .. import _lib

DEFAULT_SEED = 1234
MAX_POINTS_PER_CENTROID = 256            # k-means training points per centroid (seeded subset beyond)
COARSE_ITERS = 10
PQ_ITERS = 25
PQ_MAX_TRAIN = 1024 * 256                # training points of the PQ stage (seeded subset beyond)
PQ_KS = 256                              # nbits = 8
SPLIT_EPS = 1.0 / 1024                   # empty-cluster split: the two copies are scaled by 1 +- SPLIT_EPS
MAX_NPROBE = 128
MAX_K = 32
MAX_NLIST = 16384
REFINE_M = 4                             # IVFPQ-RR: refine sub-quantizers ...
REFINE_KS = 16                           # ... of 2^4 codewords each
MAX_K_FACTOR = 4                         # first-stage candidates per result (k * k_factor <= 128)
LUT_CODES = {'f32': 0, 'f16': 1}         # NAFP_IVF_LUT_F32 / NAFP_IVF_LUT_F16 (include/nafp.h)
ASSIGN_CHUNK = 1 << 20                   # rows per coarse-assignment launch (the exact kernel's workspace grows with them)

# independent random streams of one seed
STREAM_TRAIN_SUBSET, STREAM_COARSE, STREAM_COARSE_SPLIT, STREAM_PQ, STREAM_PQ_SPLIT = range(5)
STREAM_REFINE, STREAM_REFINE_SPLIT = 5, 6   # IVFPQ-RR: the refine quantizer's initial pick and its splits
STREAM_HNSW_LEVEL = 7                       # HNSW (eval/hnsw.py): the level draws, one per row in id order


def rng_for(seed, stream):
    return np.random.default_rng([int(seed), int(stream)])


def subset_indices(n, n_max, rng):
    """Sorted indices of a seeded random subset of n_max of n rows (all rows if n <= n_max)."""
    if n <= n_max:
        return None
    return np.sort(rng.permutation(n)[:int(n_max)])


def training_subset(x, n_max, seed=DEFAULT_SEED):
    """get_index's training set: x, or a seeded random subset of int(n_max) of its rows (the reference draws it unseeded)."""
    idx = subset_indices(len(x), int(n_max), rng_for(seed, STREAM_TRAIN_SUBSET))
    return x if idx is None else _take(x, idx)


def _take(x, idx):
    if torch.is_tensor(x):
        return x[torch.from_numpy(idx).to(x.device)]
    return np.asarray(x[idx], dtype=np.float32)


def split_empty_clusters(cent, counts, rng):
    """faiss's split of empty clusters, in place on cent (k, dsub) / counts (k,): for each empty cluster in order, a donor is
    drawn with probability proportional to (size - 1) (one uniform draw against the cumulative weights), its centroid copied
    into the empty one, the two scaled by 1 +- SPLIT_EPS with the sign alternating per dimension, and its count halved."""
    k, dsub = cent.shape
    sign = np.where(np.arange(dsub) % 2 == 0, 1.0, -1.0)
    up = (1.0 + sign * SPLIT_EPS).astype(cent.dtype)
    down = (1.0 - sign * SPLIT_EPS).astype(cent.dtype)
    for ci in range(k):
        if counts[ci] != 0:
            continue
        w = np.maximum(counts.astype(np.float64) - 1.0, 0.0)
        cum = np.cumsum(w)
        cj = min(int(np.searchsorted(cum, rng.random() * cum[-1], side='right')), k - 1)
        cent[ci] = cent[cj] * up
        cent[cj] = cent[cj] * down
        counts[ci] = counts[cj] // 2
        counts[cj] -= counts[ci]
    return cent, counts


class _Dev:
    """Thin wrappers of the C ABI on one device."""

    def __init__(self, device):
        self.device = device
        self.lib = _lib.load()

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def bucket(self, keys, key_bytes, n, nb, batch=1):
        lib = self.lib
        offsets = self.empty((batch, nb + 1), torch.int32)
        ids = self.empty((batch, max(n, 1)), torch.int32)
        need = int(lib.nafp_ivf_bucket_workspace_bytes(n, nb, batch))
        ws = self.empty((need,), torch.uint8)
        _lib.check(lib.nafp_ivf_bucket(_lib.ptr(keys), key_bytes, n, nb, batch, _lib.ptr(offsets), _lib.ptr(ids), _lib.ptr(ws), need,
                                       _lib.current_stream()), 'ivf_bucket')
        return offsets, ids

    def assign(self, x, cent, out=None):
        """Nearest centroid per row (the exact search with k = 1 against the centroid table), in chunks."""
        lib = self.lib
        n, d = x.shape
        nlist = cent.shape[0]
        aux = self.empty((int(lib.nafp_search_index_aux_floats(nlist)),), torch.float32)
        _lib.check(lib.nafp_search_index_prepare(_lib.ptr(cent), nlist, d, _lib.ptr(aux), _lib.current_stream()), 'search_index_prepare')
        out = self.empty((n,), torch.int32) if out is None else out
        dist = self.empty((min(n, ASSIGN_CHUNK),), torch.float32)
        ws = None
        for a in range(0, n, ASSIGN_CHUNK):
            b = min(n, a + ASSIGN_CHUNK)
            need = int(lib.nafp_search_workspace_bytes(b - a, nlist, 1))
            if ws is None or ws.numel() < need:
                ws = self.empty((need,), torch.uint8)
            _lib.check(lib.nafp_search_topk_l2(_lib.ptr(x[a:b]), b - a, _lib.ptr(cent), _lib.ptr(aux), nlist, d, 1, _lib.ptr(dist),
                                               _lib.ptr(out[a:b]), _lib.ptr(ws), ws.numel(), _lib.current_stream()), 'search_topk_l2')
        return out

    def pq_encode(self, x, cent_assign, coarse, pq, out=None):
        n, d = x.shape
        out = self.empty((n, pq.shape[0]), torch.uint8) if out is None else out
        _lib.check(self.lib.nafp_ivf_pq_encode(_lib.ptr(x), n, d, _lib.ptr(cent_assign), _lib.ptr(coarse), _lib.ptr(pq), pq.shape[0],
                                               _lib.ptr(out), _lib.current_stream()), 'ivf_pq_encode')
        return out

    def pq_residuals(self, r, pq, codes):
        """r - decode(codes): the second-level residuals."""
        out = torch.empty_like(r)
        _lib.check(self.lib.nafp_ivf_pq_residuals(_lib.ptr(r), r.shape[0], r.shape[1], _lib.ptr(pq), pq.shape[0], _lib.ptr(codes),
                                                  _lib.ptr(out), _lib.current_stream()), 'ivf_pq_residuals')
        return out

    def refine_encode(self, r2, refine, packed):
        """Refine codes of the rows r2: (n, 2) nibble-packed, or (n, 4) one code per byte."""
        n, d = r2.shape
        out = self.empty((n, 2 if packed else REFINE_M), torch.uint8)
        _lib.check(self.lib.nafp_ivf_refine_encode(_lib.ptr(r2), n, d, _lib.ptr(refine), REFINE_M, 4, int(bool(packed)), _lib.ptr(out),
                                                   _lib.current_stream()), 'ivf_refine_encode')
        return out

    def residuals(self, x, assign, cent):
        out = torch.empty_like(x)
        _lib.check(self.lib.nafp_ivf_residuals(_lib.ptr(x), x.shape[0], x.shape[1], _lib.ptr(assign), _lib.ptr(cent), _lib.ptr(out),
                                               _lib.current_stream()), 'ivf_residuals')
        return out

    def kmeans(self, x, cent, nb, batch, niter, rng, assign_fn):
        """Lloyd iterations on the device from the initial centroids `cent` (batch, nb, dsub), updated in place: assign (ties:
        smaller id), bucket, mean in id order, host split of empty clusters.  Returns the final cluster sizes (batch, nb)."""
        n, dim = x.shape
        dsub = dim // batch
        counts = self.empty((batch, nb), torch.int32)
        c = None
        for _ in range(niter):
            keys, key_bytes = assign_fn(cent)
            offsets, ids = self.bucket(keys, key_bytes, n, nb, batch)
            _lib.check(self.lib.nafp_ivf_kmeans_update(_lib.ptr(x), n, dim, batch, _lib.ptr(offsets), _lib.ptr(ids), nb, _lib.ptr(cent),
                                                       _lib.ptr(counts), _lib.current_stream()), 'ivf_kmeans_update')
            c = counts.cpu().numpy().astype(np.int64)
            if (c == 0).any():
                h = cent.cpu().numpy().reshape(batch, nb, dsub)
                for b in range(batch):
                    split_empty_clusters(h[b], c[b], rng)
                cent.copy_(torch.from_numpy(h).reshape(cent.shape))
        return c


def _as_device(x, device):
    if torch.is_tensor(x):
        return _lib.require_cuda(x, 'x').to(device=device, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.array(x, dtype=np.float32)).to(device)


def _codebook(c, shape, device):
    """Explicit codewords (numpy or tensor, any shape of the right size) as a float32 tensor of `shape` of their own on the device."""
    return _as_device(c.reshape(shape) if torch.is_tensor(c) else np.asarray(c, dtype=np.float32).reshape(shape), device).clone()


def kmeans(x, init, niter=COARSE_ITERS, seed=DEFAULT_SEED, device=None):
    """k-means on the device from an explicit initialisation init (k, d): the coarse quantizer's training loop.
    Returns (centroids (k, d) float32 numpy, final cluster sizes (k,))."""
    dev = _Dev(torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device()))
    xd = _as_device(x, dev.device)
    cent = _as_device(init, dev.device).clone()
    k = cent.shape[0]
    counts = dev.kmeans(xd, cent, k, 1, niter, rng_for(seed, STREAM_COARSE_SPLIT), lambda c: (dev.assign(xd, c), 4))
    return cent.cpu().numpy(), counts[0]


class _IVFBase:
    kind = None

    def __init__(self, d, nlist, seed=DEFAULT_SEED, device=None):
        from .eval_faiss import FlatL2Index
        if d not in (64, 128, 256):
            raise NotImplementedError(f'fingerprint dimension {d}')
        if not 1 <= int(nlist) <= MAX_NLIST:
            raise NotImplementedError(f'nlist = {nlist} (1 .. {MAX_NLIST})')
        self.d, self.nlist, self.seed = int(d), int(nlist), int(seed)
        self._flat = FlatL2Index(d, device=device)             # the fp32 rows in insertion order
        self.device = self._flat.device
        self._dev = _Dev(self.device)
        self._nprobe = 1
        self.centroids = None                                  # (nlist, d) float32 on the device
        self._assign = self._dev.empty((0,), torch.int32)
        self._lists = None

    @property
    def nprobe(self):
        return self._nprobe

    @nprobe.setter
    def nprobe(self, v):
        if not 1 <= int(v) <= MAX_NPROBE:
            raise NotImplementedError(f'nprobe = {v} (the HIP IVF search keeps 1 .. {MAX_NPROBE} probes)')
        self._nprobe = int(v)

    @property
    def is_trained(self):
        return self.centroids is not None

    @property
    def ntotal(self):
        return self._flat.ntotal

    def _train_coarse(self, x, init):
        n = len(x)
        if n < self.nlist:
            raise ValueError(f'{n} training points for nlist = {self.nlist} centroids (faiss refuses this too)')
        rng = rng_for(self.seed, STREAM_COARSE)
        idx = subset_indices(n, self.nlist * MAX_POINTS_PER_CENTROID, rng)
        xt = _as_device(x if idx is None else _take(x, idx), self.device)
        if init is None:
            pick = rng.permutation(xt.shape[0])[:self.nlist]
            cent = xt[torch.from_numpy(pick).to(self.device)].contiguous()
        else:
            cent = _as_device(init, self.device).clone()
        dev = self._dev
        dev.kmeans(xt, cent, self.nlist, 1, COARSE_ITERS, rng_for(self.seed, STREAM_COARSE_SPLIT), lambda c: (dev.assign(xt, c), 4))
        self.centroids = cent

    def probe_device(self, q):
        """(nq, min(nprobe, nlist)) int32 CUDA: the probed lists per query, nearest first (ties: smaller list id)."""
        q = _lib.require_cuda(q, 'q').float().contiguous()
        npr = min(self._nprobe, self.nlist)
        out = self._dev.empty((q.shape[0], npr), torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self._dev.lib.nafp_ivf_probe(_lib.ptr(q), q.shape[0], _lib.ptr(self.centroids), self.nlist, self.d, npr, _lib.ptr(out),
                                                    _lib.current_stream()), 'ivf_probe')
        return out

    def add(self, x):
        if not self.is_trained:
            raise RuntimeError('the index is not trained')
        n0 = self.ntotal
        self._flat.add(x)
        n = self.ntotal - n0
        if n == 0:
            return
        xd = self._flat._x[n0:n0 + n]
        with torch.cuda.device(self.device):
            a = self._dev.assign(xd, self.centroids)
            self._add_encoded(xd, a)
            self._assign = torch.cat([self._assign, a])
        self._lists = None

    def _add_encoded(self, xd, a):
        pass

    def _prepare(self):
        if self._lists is None:
            with torch.cuda.device(self.device):
                offsets, ids = self._dev.bucket(self._assign, 4, self.ntotal, self.nlist, 1)
                self._lists = self._build_lists(offsets.reshape(-1), ids.reshape(-1))
        return self._lists

    def _search_inputs(self, q, k):
        """What every search starts with: the queries as contiguous float32 on the device, k and the index checked, the lists."""
        q = _lib.require_cuda(q, 'q').float().contiguous()
        if k > MAX_K or k < 1:
            raise NotImplementedError(f'k = {k} (the HIP search keeps k <= {MAX_K} results per query)')
        if self.ntotal == 0:
            raise ValueError('empty index')
        return q, self._prepare()

    def _search_numpy(self, search_device, q, k):
        """numpy in, numpy out of a device search: distances float32, ids int64."""
        qd = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(self.device)
        return tuple(t.cpu().numpy() if t.is_floating_point() else t.cpu().numpy().astype(np.int64) for t in search_device(qd, k))

    def search_device(self, q, k):
        """q: (nq, d) CUDA float32 -> (D, I) CUDA tensors (float32, int32)."""
        q, lists = self._search_inputs(q, k)
        nq = q.shape[0]
        D = self._dev.empty((nq, k), torch.float32)
        I = self._dev.empty((nq, k), torch.int32)
        need = int(self._dev.lib.nafp_ivf_search_workspace_bytes(nq, self.nlist, self._nprobe, k, self.kind))
        if need < 0:
            raise NotImplementedError(f'k = {k}, nprobe = {self._nprobe}')
        ws = self._dev.empty((need,), torch.uint8)
        with torch.cuda.device(self.device):
            self._search(q, k, lists, D, I, ws, need)
        return D, I

    def search(self, q, k):
        """faiss signature: numpy in, (D float32, I int64) numpy out."""
        return self._search_numpy(self.search_device, q, k)

    def reconstruct_n(self, i0, n):
        return self._flat.reconstruct_n(i0, n)

    def sequence_scores(self, q, task_q0, task_len, cand):
        """Scores from the original fp32 rows in insertion order (FlatL2Index.sequence_scores)."""
        return self._flat.sequence_scores(q, task_q0, task_len, cand)

    def sequence_match(self, q, topk_ids, task_q0, task_len, n_out=10, max_len=None):
        """Ranked sequence candidates from the original fp32 rows in insertion order (FlatL2Index.sequence_match)."""
        return self._flat.sequence_match(q, topk_ids, task_q0, task_len, n_out=n_out, max_len=max_len)

    def list_assignments(self):
        """(ntotal,) int32 CUDA: the list of every row, in insertion order."""
        return self._assign

    def lists(self):
        """(offsets (nlist + 1,), ids (ntotal,)) int32 CUDA: the inverted lists, ascending ids inside each."""
        L = self._prepare()
        return L['offsets'], L['ids'][:self.ntotal]


class IVFFlatIndex(_IVFBase):
    """faiss.IndexIVFFlat(quantizer, d, nlist): rows stored as fp32 in their lists; exact squared L2 distances."""
    kind = 0

    def train(self, x, init=None):
        """x: (n, d) numpy / memmap / CUDA tensor.  init: an explicit (nlist, d) k-means initialisation."""
        self._train_coarse(x, init)

    def set_params(self, centroids):
        self.centroids = _as_device(centroids, self.device).clone()
        self._lists = None

    @property
    def index_description(self):
        return f'IVF-Flat (HIP; nlist {self.nlist}, nprobe {self._nprobe})'

    def _build_lists(self, offsets, ids):
        lib, n = self._dev.lib, self.ntotal
        bound = int(lib.nafp_ivf_flat_rows_bound(n, self.nlist))
        row_off = self._dev.empty((self.nlist + 1,), torch.int32)
        rows = self._dev.empty((bound, self.d), torch.float32)
        hn = self._dev.empty((bound,), torch.float32)
        row_ids = self._dev.empty((bound,), torch.int32)
        _lib.check(lib.nafp_ivf_flat_lists(_lib.ptr(self._flat._x), n, self.d, _lib.ptr(offsets), _lib.ptr(ids), self.nlist, _lib.ptr(row_off),
                                           _lib.ptr(rows), _lib.ptr(hn), _lib.ptr(row_ids), _lib.current_stream()), 'ivf_flat_lists')
        return dict(offsets=offsets, ids=ids, row_off=row_off, rows=rows, hn=hn, row_ids=row_ids)

    def _search(self, q, k, L, D, I, ws, need):
        _lib.check(self._dev.lib.nafp_ivf_flat_search(_lib.ptr(q), q.shape[0], _lib.ptr(self.centroids), self.nlist, self.d, self._nprobe,
                                                      _lib.ptr(L['rows']), _lib.ptr(L['hn']), _lib.ptr(L['row_off']), _lib.ptr(L['row_ids']),
                                                      int(k), _lib.ptr(D), _lib.ptr(I), _lib.ptr(ws), need, _lib.current_stream()),
                   'ivf_flat_search')


class IVFPQIndex(_IVFBase):
    """faiss.IndexIVFPQ(quantizer, d, nlist, M, nbits) with by_residual: M = 64 sub-quantizers of 2^nbits = 256 codewords of
    the residual to the coarse centroid.  `lut`: the precision of the ADC tables of a search, 'f32' (default) or 'f16' (the
    reference's GPU index, useFloat16; contract in include/nafp.h).  It can be changed at any time: centroids, codes
    and lists do not depend on it."""
    kind = 1

    def __init__(self, d, nlist, M=64, nbits=8, seed=DEFAULT_SEED, device=None, lut='f32'):
        if M != 64 or nbits != 8 or d % M or d // M not in (1, 2, 4):
            raise NotImplementedError(f'IVF-PQ with M = {M}, nbits = {nbits} (this build: M = 64, nbits = 8)')
        self.lut = lut
        super().__init__(d, nlist, seed, device)
        self.M, self.nbits, self.dsub = int(M), int(nbits), d // M
        self.pq_centroids = None                               # (M, 256, dsub) float32 on the device
        self._codes = self._dev.empty((0, self.M), torch.uint8)

    @property
    def is_trained(self):
        return self.centroids is not None and self.pq_centroids is not None

    @property
    def lut(self):
        return self._lut

    @lut.setter
    def lut(self, v):
        if v not in LUT_CODES:
            raise ValueError(f'lut = {v!r} (the ADC tables are {" or ".join(map(repr, LUT_CODES))})')
        self._lut = v

    @property
    def index_description(self):
        tables = ', fp16 tables' if self._lut == 'f16' else ''
        return f'IVFPQ (HIP; nlist {self.nlist}, M {self.M}, nbits {self.nbits}, nprobe {self._nprobe}{tables})'

    def set_params(self, centroids, pq_centroids):
        self.centroids = _as_device(centroids, self.device).clone()
        self.pq_centroids = _codebook(pq_centroids, (self.M, PQ_KS, self.dsub), self.device)
        self._lists = None

    def train(self, x, init=None, pq_init=None):
        """x: (n, d).  init: explicit (nlist, d) coarse initialisation; pq_init: explicit (M, 256, dsub) PQ initialisation."""
        self._train_coarse(x, init)
        self._train_pq(x, pq_init)

    def _train_pq(self, x, pq_init):
        """Trains the PQ stage; returns its training residuals (after the subsets), on the device."""
        rng = rng_for(self.seed, STREAM_PQ)
        idx = subset_indices(len(x), PQ_MAX_TRAIN, rng)
        xp = _as_device(x if idx is None else _take(x, idx), self.device)
        dev = self._dev
        with torch.cuda.device(self.device):
            r = dev.residuals(xp, dev.assign(xp, self.centroids), self.centroids)
            idx = subset_indices(r.shape[0], PQ_KS * MAX_POINTS_PER_CENTROID, rng)
            if idx is not None:
                r = r[torch.from_numpy(idx).to(self.device)].contiguous()
            if pq_init is None:
                if r.shape[0] < PQ_KS:
                    raise ValueError(f'{r.shape[0]} training points for {PQ_KS} PQ centroids')
                pick = torch.from_numpy(rng.permutation(r.shape[0])[:PQ_KS]).to(self.device)
                pq = r[pick].reshape(PQ_KS, self.M, self.dsub).transpose(0, 1).contiguous()
            else:
                pq = _codebook(pq_init, (self.M, PQ_KS, self.dsub), self.device)
            dev.kmeans(r, pq, PQ_KS, self.M, PQ_ITERS, rng_for(self.seed, STREAM_PQ_SPLIT), lambda c: (dev.pq_encode(r, None, None, c), 1))
        self.pq_centroids = pq
        return r

    def _add_encoded(self, xd, a):
        self._codes = torch.cat([self._codes, self._dev.pq_encode(xd, a, self.centroids, self.pq_centroids)])

    def codes(self):
        """(ntotal, M) uint8 CUDA: the PQ codes in insertion order."""
        return self._codes

    def _build_lists(self, offsets, ids):
        codes_sorted = self._dev.empty((self.ntotal, self.M), torch.uint8)
        _lib.check(self._dev.lib.nafp_ivf_pq_lists(_lib.ptr(self._codes), self.ntotal, self.M, _lib.ptr(ids), _lib.ptr(codes_sorted),
                                                   _lib.current_stream()), 'ivf_pq_lists')
        return dict(offsets=offsets, ids=ids, codes=codes_sorted)

    def _search(self, q, k, L, D, I, ws, need):
        _lib.check(self._dev.lib.nafp_ivf_pq_search_ex(_lib.ptr(q), q.shape[0], _lib.ptr(self.centroids), self.nlist, self.d, self._nprobe,
                                                       _lib.ptr(self.pq_centroids), self.M, _lib.ptr(L['codes']), _lib.ptr(L['offsets']),
                                                       _lib.ptr(L['ids']), int(k), _lib.ptr(D), _lib.ptr(I), LUT_CODES[self._lut],
                                                       _lib.ptr(ws), need, _lib.current_stream()), 'ivf_pq_search_ex')

    def adc_tables(self, q, pair_query, pair_list):
        """The ADC tables the search builds for the pairs (query row pair_query[p] of q, list pair_list[p]): (n_pairs, M, 256) CUDA,
        float32 or float16 by `lut`."""
        q = _lib.require_cuda(q, 'q').float().contiguous()
        pq_, pl_ = (torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).to(device=self.device, dtype=torch.int32).contiguous()
                    for t in (pair_query, pair_list))
        if pq_.shape != pl_.shape or pq_.dim() != 1:
            raise ValueError('pair_query and pair_list are two 1-D arrays of one length')
        out = self._dev.empty((pq_.shape[0], self.M, PQ_KS), torch.float16 if self._lut == 'f16' else torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self._dev.lib.nafp_ivf_pq_adc_tables(_lib.ptr(q), q.shape[0], _lib.ptr(pq_), _lib.ptr(pl_), pq_.shape[0],
                                                            _lib.ptr(self.centroids), self.nlist, self.d, _lib.ptr(self.pq_centroids),
                                                            self.M, LUT_CODES[self._lut], _lib.ptr(out), _lib.current_stream()),
                       'ivf_pq_adc_tables')
        return out


class IVFPQRIndex(IVFPQIndex):
    """faiss.IndexIVFPQR(quantizer, d, nlist, M, nbits, M_refine, nbits_refine): an IVFPQIndex plus a refine product quantizer
    (M_refine = 4 sub-spaces of 2^4 codewords) of what the PQ stage leaves, x - centroid[list] - pq_decode(code), 2 bytes per row.
    `search(q, k)`: the IVF-PQ ADC search of this index for k * k_factor candidates (`lut` applies), then those re-ranked by the
    fp32 distance to their refined reconstruction (include/nafp.h "IVFPQ-RR").  faiss's CPU class is the model."""

    def __init__(self, d, nlist, M=64, nbits=8, M_refine=4, nbits_refine=4, seed=DEFAULT_SEED, device=None, lut='f32', k_factor=4):
        if M_refine != REFINE_M or nbits_refine != 4:
            raise NotImplementedError(f'IVFPQ-RR with M_refine = {M_refine}, nbits_refine = {nbits_refine} (this build: 4 x 4 bits)')
        super().__init__(d, nlist, M, nbits, seed, device, lut)
        self.M_refine, self.nbits_refine, self.dsub_refine = REFINE_M, 4, d // REFINE_M
        self.k_factor = k_factor
        self.refine_centroids = None                           # (4, 16, d / 4) float32 on the device
        self._rcodes = self._dev.empty((0, 2), torch.uint8)

    @property
    def is_trained(self):
        return super().is_trained and self.refine_centroids is not None

    @property
    def k_factor(self):
        return self._k_factor

    @k_factor.setter
    def k_factor(self, v):
        if int(v) != v or not 1 <= int(v) <= MAX_K_FACTOR:
            raise NotImplementedError(f'k_factor = {v} (an integer 1 .. {MAX_K_FACTOR})')
        self._k_factor = int(v)

    @property
    def index_description(self):
        tables = ', fp16 tables' if self._lut == 'f16' else ''
        return (f'IVFPQR (HIP; nlist {self.nlist}, M {self.M}, nbits {self.nbits}, refine {self.M_refine} x {self.nbits_refine} bits, '
                f'k_factor {self._k_factor}, nprobe {self._nprobe}{tables})')

    def set_params(self, centroids, pq_centroids, refine_centroids):
        super().set_params(centroids, pq_centroids)
        self.refine_centroids = _codebook(refine_centroids, (REFINE_M, REFINE_KS, self.dsub_refine), self.device)

    def train(self, x, init=None, pq_init=None, refine_init=None):
        """As IVFPQIndex.train, then the refine quantizer on the PQ stage's own training residuals r: k-means (16 codewords in each
        of 4 sub-spaces, PQ_ITERS iterations) of r - decode(encode(r)).  refine_init: an explicit (4, 16, d / 4) initialisation."""
        self._train_coarse(x, init)
        r = self._train_pq(x, pq_init)
        dev = self._dev
        with torch.cuda.device(self.device):
            r2 = dev.pq_residuals(r, self.pq_centroids, dev.pq_encode(r, None, None, self.pq_centroids))
            if refine_init is None:
                if r2.shape[0] < REFINE_KS:
                    raise ValueError(f'{r2.shape[0]} training points for {REFINE_KS} refine centroids')
                pick = torch.from_numpy(rng_for(self.seed, STREAM_REFINE).permutation(r2.shape[0])[:REFINE_KS]).to(self.device)
                rf = r2[pick].reshape(REFINE_KS, REFINE_M, self.dsub_refine).transpose(0, 1).contiguous()
            else:
                rf = _codebook(refine_init, (REFINE_M, REFINE_KS, self.dsub_refine), self.device)
            dev.kmeans(r2, rf, REFINE_KS, REFINE_M, PQ_ITERS, rng_for(self.seed, STREAM_REFINE_SPLIT),
                       lambda c: (dev.refine_encode(r2, c, False), 1))
        self.refine_centroids = rf

    def _add_encoded(self, xd, a):
        dev = self._dev
        codes = dev.pq_encode(xd, a, self.centroids, self.pq_centroids)
        rcodes = dev.empty((xd.shape[0], 2), torch.uint8)
        for i0 in range(0, xd.shape[0], ASSIGN_CHUNK):            # the two residual arrays are temporaries: a chunk at a time
            i1 = min(xd.shape[0], i0 + ASSIGN_CHUNK)
            r2 = dev.pq_residuals(dev.residuals(xd[i0:i1], a[i0:i1], self.centroids), self.pq_centroids, codes[i0:i1])
            rcodes[i0:i1] = dev.refine_encode(r2, self.refine_centroids, True)
        self._codes = torch.cat([self._codes, codes])
        self._rcodes = torch.cat([self._rcodes, rcodes])

    def refine_codes(self):
        """(ntotal, 2) uint8 CUDA: the refine codes in insertion order, byte0 = c0 | c1 << 4, byte1 = c2 | c3 << 4."""
        return self._rcodes

    def search_stages_device(self, q, k):
        """q: (nq, d) CUDA -> (D1, I1, D, I) CUDA: the first stage's k * k_factor candidates and the k re-ranked results."""
        q, L = self._search_inputs(q, k)
        nq, k1, lib = q.shape[0], int(k) * self._k_factor, self._dev.lib
        D, I = self._dev.empty((nq, k), torch.float32), self._dev.empty((nq, k), torch.int32)
        D1, I1 = self._dev.empty((nq, k1), torch.float32), self._dev.empty((nq, k1), torch.int32)
        need = int(lib.nafp_ivf_pq_wide_workspace_bytes(nq, self.nlist, self._nprobe, k1))
        if need < 0:
            raise NotImplementedError(f'k = {k}, k_factor = {self._k_factor}, nprobe = {self._nprobe}')
        ws = self._dev.empty((need,), torch.uint8)
        with torch.cuda.device(self.device):
            _lib.check(lib.nafp_ivf_pqr_search(_lib.ptr(q), nq, _lib.ptr(self.centroids), self.nlist, self.d, self._nprobe,
                                               _lib.ptr(self.pq_centroids), self.M, _lib.ptr(L['codes']), _lib.ptr(L['offsets']),
                                               _lib.ptr(L['ids']), _lib.ptr(self._assign), _lib.ptr(self._codes),
                                               _lib.ptr(self.refine_centroids), self.M_refine, self.nbits_refine, _lib.ptr(self._rcodes),
                                               self.ntotal, int(k), self._k_factor, _lib.ptr(D), _lib.ptr(I), _lib.ptr(D1), _lib.ptr(I1),
                                               LUT_CODES[self._lut], _lib.ptr(ws), need, _lib.current_stream()), 'ivf_pqr_search')
        return D1, I1, D, I

    def search_device(self, q, k):
        return self.search_stages_device(q, k)[2:]

    def search_stages(self, q, k):
        """numpy in, (D1, I1, D, I) numpy out (ids int64): `search` plus the first stage it re-ranked."""
        return self._search_numpy(self.search_stages_device, q, k)
