"""Segment/sequence-wise audio search experiment and evaluation on the HIP exact index.

Host mirror of the reference's eval/eval_faiss.py (`load_memmap_data` :18-62, `eval_faiss` :93-275)
and of `get_index` (eval/utils/get_index_faiss.py:10-121) for index_type 'L2' -- the exact
faiss.IndexFlatL2 -- backed by libnafp's search kernels (include/nafp.h "Search / evaluation").
With NAFP_APPROX_INDEX=1 in the environment, 'ivf' and 'ivfpq' build real IVF-Flat / IVF-PQ indexes on the device (eval/ivf.py,
opt-in; `index_used.json` then names the index and its parameters; NAFP_IVFPQ_LUT=f16 gives 'ivfpq' the reference's fp16 lookup
tables; NAFP_IVFPQ_RR=1 next to it makes 'ivfpq-rr' the IVFPQ-RR index, IVF-PQ with refine codes and an exact re-ranking of
4 x k candidates; NAFP_HNSW=1 next to it makes 'hnsw' the HNSW graph index of eval/hnsw.py, M 16, efConstruction 80, efSearch 16:
the reference builds that one on the CPU only, this project on the GPU only).  Otherwise, and always for IVFPQ-ONDISK,
the approximate index types are not built: a request for one of them
(the reference's default is `-i ivfpq`) is SERVED BY THE EXACT SEARCH, with a notice on stderr and the substitution
recorded in `index_used.json` next to `raw_score.npy` -- on an MI355X the whole [dummy_db ; db] table stays resident
in HBM (51 GB for 100 M fingerprints out of 288 GB), and the exact index is the accuracy ceiling of the approximate ones.
Fingerprint dimensions 64 / 128 / 256 (EMB_SZ).

Same inputs ({query, db, dummy_db}.mm + *_shape.npy written by `generate`), same outputs
(`raw_score.npy` = [top1_exact | top1_near | top3_exact | top10_exact] per test id and sequence
length, `test_ids.npy`), same metrics.  Differences in mechanism, not in result:
  * all test ids x sequence lengths are evaluated in ONE batched search over the distinct query
    rows, one batched sequence-score launch, and a vectorised ranking -- not a Python loop with an
    index.search call per (id, length); the ranking runs on the host (numpy) unless NAFP_SEQ_MATCH=1 is set: then one kernel
    per sequence length goes from the top-k ids to the ten ranked predictions on the device (`sequence_match`; same results,
    `index_used.json` then says "sequence_rank": "device");
  * `dummy_db.mm` is NOT extended on disk (the reference appends `db` to it as its
    "fake_recon_index", eval_faiss.py:158-167): the concatenated table lives on the device;
  * equal scores/distances rank the smaller id first (faiss/argsort leave ties unspecified);
  * a plain printed table instead of curses.
"""
import glob
import os
import time

import numpy as np
import torch

from .. import _lib


def load_memmap_data(source_dir, fname, append_extra_length=None, shape_only=False, display=True):
    """eval_faiss.py:18-62."""
    path_shape = source_dir + fname + '_shape.npy'
    path_data = source_dir + fname + '.mm'
    data_shape = np.load(path_shape)
    if shape_only:
        return data_shape
    if append_extra_length:
        data_shape[0] += append_extra_length
        data = np.memmap(path_data, dtype='float32', mode='r+', shape=(data_shape[0], data_shape[1]))
    else:
        data = np.memmap(path_data, dtype='float32', mode='r', shape=(data_shape[0], data_shape[1]))
    if display:
        print(f'Load {data_shape[0]:,} items from \033[32m{path_data}\033[0m.')
    return data, data_shape


class FlatL2Index:
    """faiss.IndexFlatL2 as the reference uses it: `.add(x)` (repeatedly), `.ntotal`, `.search(q, k)`
    -> (D, I) with squared L2 distances, nearest first; plus `.reconstruct_n` and the batched
    `.sequence_scores` the evaluation needs.  The vectors live in ONE device array."""

    def __init__(self, d, capacity=0, device=None):
        if d not in (64, 128, 256):
            raise NotImplementedError(f'fingerprint dimension {d}')
        self.d = int(d)
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self._lib = _lib.load()
        self._x = torch.empty((int(capacity), self.d), dtype=torch.float32, device=self.device)
        self.ntotal = 0
        self._aux = None

    def add(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32) if not torch.is_tensor(x) else x
        n = x.shape[0]
        if x.shape[1] != self.d:
            raise ValueError(f'expected (n, {self.d}) vectors')
        if self.ntotal + n > self._x.shape[0]:
            grown = torch.empty((max(self.ntotal + n, 2 * self._x.shape[0]), self.d), dtype=torch.float32, device=self.device)
            grown[:self.ntotal] = self._x[:self.ntotal]
            self._x = grown
        step = 1 << 20                                        # upload in 512 MB pieces (memmap friendly)
        for a in range(0, n, step):
            b = min(n, a + step)
            piece = x[a:b] if torch.is_tensor(x) else torch.from_numpy(np.array(x[a:b], dtype=np.float32))
            self._x[self.ntotal + a:self.ntotal + b].copy_(piece)
        self.ntotal += n
        self._aux = None

    def _prepare(self):
        if self._aux is None:
            n_aux = int(self._lib.nafp_search_index_aux_floats(self.ntotal))
            self._aux = torch.empty((n_aux,), dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(self._lib.nafp_search_index_prepare(_lib.ptr(self._x), self.ntotal, self.d, _lib.ptr(self._aux),
                                                               _lib.current_stream()), 'search_index_prepare')
        return self._aux

    def search_device(self, q, k):
        """q: (nq, d) CUDA float32 -> (D, I) CUDA tensors (float32, int32)."""
        q = _lib.require_cuda(q, 'q').float().contiguous()
        if self.ntotal == 0:
            raise ValueError('empty index')
        aux = self._prepare()
        nq = q.shape[0]
        D = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        I = torch.empty((nq, k), dtype=torch.int32, device=self.device)
        need = int(self._lib.nafp_search_workspace_bytes(nq, self.ntotal, k))
        if need < 0:
            raise NotImplementedError(f'k = {k} (the HIP search keeps k <= 32 results per query)')
        ws = torch.empty((need,), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nafp_search_topk_l2(_lib.ptr(q), nq, _lib.ptr(self._x), _lib.ptr(aux), self.ntotal, self.d,
                                                     int(k), _lib.ptr(D), _lib.ptr(I), _lib.ptr(ws), need,
                                                     _lib.current_stream()), 'search_topk_l2')
        return D, I

    def search_device_excl(self, q, k, excl):
        """`search_device` with a row range left out per query (nafp_search_topk_l2_excl, include/nafp.h): excl (nq, 2) CUDA
        int32, query r gets the k nearest rows outside [excl[r, 0], excl[r, 1]).  Any pair is legal; lo >= hi excludes nothing."""
        q = _lib.require_cuda(q, 'q').float().contiguous()
        excl = _lib.require_cuda(excl, 'excl')
        if self.ntotal == 0:
            raise ValueError('empty index')
        nq = q.shape[0]
        if excl.dtype != torch.int32 or excl.dim() != 2 or tuple(excl.shape) != (nq, 2):
            raise TypeError('search_device_excl: excl (nq, 2) int32')
        excl = excl.contiguous()
        aux = self._prepare()
        D = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        I = torch.empty((nq, k), dtype=torch.int32, device=self.device)
        need = int(self._lib.nafp_search_workspace_bytes(nq, self.ntotal, k))
        if need < 0:
            raise NotImplementedError(f'k = {k} (the HIP search keeps k <= 32 results per query)')
        ws = torch.empty((need,), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nafp_search_topk_l2_excl(_lib.ptr(q), nq, _lib.ptr(self._x), _lib.ptr(aux), self.ntotal, self.d,
                                                          int(k), _lib.ptr(excl), _lib.ptr(D), _lib.ptr(I), _lib.ptr(ws), need,
                                                          _lib.current_stream()), 'search_topk_l2_excl')
        return D, I

    def search(self, q, k):
        """faiss signature: numpy in, (D float32, I int64) numpy out."""
        qd = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(self.device)
        D, I = self.search_device(qd, k)
        return D.cpu().numpy(), I.cpu().numpy().astype(np.int64)

    def reconstruct_n(self, i0, n):
        return self._x[i0:i0 + n].cpu().numpy()

    def sequence_scores(self, q, task_q0, task_len, cand):
        """scores[t, s] = mean_i q[task_q0[t] + i] . index[cand[t, s] + i] (eval_faiss.py:224-230);
        q (nq, d) CUDA, task_q0 / task_len (T,) int32 CUDA, cand (T, S) int32 CUDA (-1 = none)."""
        T, S = cand.shape
        out = torch.empty((T, S), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nafp_search_seq_scores(_lib.ptr(q), _lib.ptr(self._x), self.ntotal, self.d, _lib.ptr(task_q0),
                                                        _lib.ptr(task_len), T, _lib.ptr(cand), S, _lib.ptr(out),
                                                        _lib.current_stream()), 'search_seq_scores')
        return out

    def sequence_match(self, q, topk_ids, task_q0, task_len, n_out=10, max_len=None):
        """The whole sequence match of eval_faiss.py:213-232 in one launch (nafp_search_seq_match, include/nafp.h): per task the
        distinct offset-compensated candidates of topk_ids (nq, k) int32 (-1 = none), each scored once like `sequence_scores`, and
        the n_out best (score descending, smaller id first).  q (nq, d) CUDA float32, task_q0 / task_len (T,) int32 CUDA;
        `max_len` defaults to the maximum of task_len.  Returns (ids (T, n_out) int32, scores (T, n_out) float32, n_cand (T,)
        int32) on the device; padding is id -1, score -inf."""
        q = _lib.require_cuda(q, 'q')
        T = int(task_q0.shape[0])
        if max_len is None:
            max_len = max(int(task_len.max()), 1) if T else 1
        ids = torch.empty((T, int(n_out)), dtype=torch.int32, device=self.device)
        scores = torch.empty((T, int(n_out)), dtype=torch.float32, device=self.device)
        n_cand = torch.empty((T,), dtype=torch.int32, device=self.device)
        if q.dtype != torch.float32 or topk_ids.dtype != torch.int32 or task_q0.dtype != torch.int32 or task_len.dtype != torch.int32:
            raise TypeError('sequence_match: q float32, topk_ids / task_q0 / task_len int32')
        if q.dim() != 2 or q.shape[1] != self.d or topk_ids.dim() != 2 or topk_ids.shape[0] != q.shape[0] or task_len.shape[0] != T:
            raise ValueError('sequence_match: q (nq, d), topk_ids (nq, k), task_q0 and task_len (T,)')
        q, topk_ids, task_q0, task_len = q.contiguous(), topk_ids.contiguous(), task_q0.contiguous(), task_len.contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nafp_search_seq_match(_lib.ptr(q), q.shape[0], _lib.ptr(self._x), self.ntotal, self.d, _lib.ptr(topk_ids),
                                                       int(topk_ids.shape[1]), _lib.ptr(task_q0), _lib.ptr(task_len), T, int(max_len),
                                                       int(n_out), _lib.ptr(ids), _lib.ptr(scores), _lib.ptr(n_cand),
                                                       _lib.current_stream()), 'search_seq_match')
        return ids, scores, n_cand

    def identify(self, q, topk_ids, task_q0, task_len, track_first, n_out=1, n_short=32, min_overlap=4, min_votes=2, max_len=None):
        """The track-aware sequence match in one launch (nafp_search_identify, include/nafp.h): per task (one analysis window of a
        recording) the distinct (track, alignment) pairs of topk_ids (nq, k) int32 with their votes, the n_short best by votes scored
        over their overlap with the track only, and the n_out best by score.  q (nq, d) CUDA float32, task_q0 / task_len (T,) int32
        CUDA, track_first (n_tracks + 1,) int32 on the host (numpy or CPU tensor): the first row of each track, checked here
        (nafp_search_identify_check_tracks_host) before anything runs; `max_len` defaults to the maximum of task_len.  Returns
        (track, align, score, votes, overlap) (T, n_out) and n_cand (T,) on the device; padding is track -1, align 0, score -inf,
        votes 0, overlap 0."""
        q = _lib.require_cuda(q, 'q')
        first = np.ascontiguousarray(track_first.numpy() if torch.is_tensor(track_first) else track_first)
        if first.dtype != np.int32 or first.ndim != 1 or first.shape[0] < 2:
            raise TypeError('identify: track_first (n_tracks + 1,) int32 on the host')
        n_tracks = int(first.shape[0]) - 1
        _lib.check(self._lib.nafp_search_identify_check_tracks_host(first.ctypes.data, n_tracks, self.ntotal), 'search_identify (track_first)')
        T = int(task_q0.shape[0])
        if q.dtype != torch.float32 or topk_ids.dtype != torch.int32 or task_q0.dtype != torch.int32 or task_len.dtype != torch.int32:
            raise TypeError('identify: q float32, topk_ids / task_q0 / task_len int32')
        if q.dim() != 2 or q.shape[1] != self.d or topk_ids.dim() != 2 or topk_ids.shape[0] != q.shape[0] or task_len.shape[0] != T:
            raise ValueError('identify: q (nq, d), topk_ids (nq, k), task_q0 and task_len (T,)')
        if max_len is None:
            max_len = max(int(task_len.max()), 1) if T else 1
        n_out = int(n_out)
        track, align, votes, overlap = (torch.empty((T, n_out), dtype=torch.int32, device=self.device) for _ in range(4))
        score = torch.empty((T, n_out), dtype=torch.float32, device=self.device)
        n_cand = torch.empty((T,), dtype=torch.int32, device=self.device)
        q, topk_ids, task_q0, task_len = q.contiguous(), topk_ids.contiguous(), task_q0.contiguous(), task_len.contiguous()
        first_dev = torch.from_numpy(first).to(self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nafp_search_identify(_lib.ptr(q), q.shape[0], _lib.ptr(self._x), self.ntotal, self.d, _lib.ptr(topk_ids),
                                                      int(topk_ids.shape[1]), _lib.ptr(task_q0), _lib.ptr(task_len), T, int(max_len),
                                                      _lib.ptr(first_dev), n_tracks, int(min_overlap), int(min_votes), int(n_short), n_out,
                                                      _lib.ptr(track), _lib.ptr(align), _lib.ptr(score), _lib.ptr(votes), _lib.ptr(overlap),
                                                      _lib.ptr(n_cand), _lib.current_stream()), 'search_identify')
        return track, align, score, votes, overlap, n_cand

    def identify_tempo(self, q, topk_ids, task_q0, task_len, track_first, rhos, n_out=1, n_short=32, min_overlap=4, min_votes=2,
                       max_len=None):
        """`identify` under tempo hypotheses, all in one launch (nafp_search_identify_tempo, include/nafp.h): `rhos` (1 .. 16 ints
        on the host, 16.16 fixed point within 52429 .. 81920) are the library rows advanced per query segment; segment i of a window
        at alignment a falls on row a + ((i * rho + 32768) >> 16).  The other arguments are those of `identify`.  Returns `identify`'s
        tuple with one more member: (track, align, score, votes, overlap) (T, n_out), n_cand (T,) and rho (T, n_out), the place in
        `rhos` of each result's hypothesis (padding -1)."""
        q = _lib.require_cuda(q, 'q')
        first = np.ascontiguousarray(track_first.numpy() if torch.is_tensor(track_first) else track_first)
        if first.dtype != np.int32 or first.ndim != 1 or first.shape[0] < 2:
            raise TypeError('identify_tempo: track_first (n_tracks + 1,) int32 on the host')
        rho = np.ascontiguousarray(np.asarray(rhos, dtype=np.int64).reshape(-1).astype(np.int32))
        n_tracks = int(first.shape[0]) - 1
        _lib.check(self._lib.nafp_search_identify_check_tracks_host(first.ctypes.data, n_tracks, self.ntotal), 'search_identify_tempo (track_first)')
        T = int(task_q0.shape[0])
        if q.dtype != torch.float32 or topk_ids.dtype != torch.int32 or task_q0.dtype != torch.int32 or task_len.dtype != torch.int32:
            raise TypeError('identify_tempo: q float32, topk_ids / task_q0 / task_len int32')
        if q.dim() != 2 or q.shape[1] != self.d or topk_ids.dim() != 2 or topk_ids.shape[0] != q.shape[0] or task_len.shape[0] != T:
            raise ValueError('identify_tempo: q (nq, d), topk_ids (nq, k), task_q0 and task_len (T,)')
        if max_len is None:
            max_len = max(int(task_len.max()), 1) if T else 1
        n_out = int(n_out)
        track, align, votes, overlap, rho_out = (torch.empty((T, n_out), dtype=torch.int32, device=self.device) for _ in range(5))
        score = torch.empty((T, n_out), dtype=torch.float32, device=self.device)
        n_cand = torch.empty((T,), dtype=torch.int32, device=self.device)
        q, topk_ids, task_q0, task_len = q.contiguous(), topk_ids.contiguous(), task_q0.contiguous(), task_len.contiguous()
        first_dev = torch.from_numpy(first).to(self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nafp_search_identify_tempo(_lib.ptr(q), q.shape[0], _lib.ptr(self._x), self.ntotal, self.d, _lib.ptr(topk_ids),
                                                            int(topk_ids.shape[1]), _lib.ptr(task_q0), _lib.ptr(task_len), T, int(max_len),
                                                            _lib.ptr(first_dev), n_tracks, rho.ctypes.data, int(rho.shape[0]),
                                                            int(min_overlap), int(min_votes), int(n_short), n_out, _lib.ptr(track),
                                                            _lib.ptr(align), _lib.ptr(score), _lib.ptr(votes), _lib.ptr(overlap),
                                                            _lib.ptr(n_cand), _lib.ptr(rho_out), _lib.current_stream()), 'search_identify_tempo')
        return track, align, score, votes, overlap, n_cand, rho_out


def seq_match_enabled():
    """NAFP_SEQ_MATCH=1: the evaluation ranks the sequence candidates on the device (`FlatL2Index.sequence_match`) instead of on
    the host.  Opt-in; the results are the same."""
    return os.environ.get('NAFP_SEQ_MATCH', '') == '1'


def seq_match_supported(index, k_probe, max_sl):
    """Whether `index` and the shape fit nafp_search_seq_match: k 1..32, k * max_sl <= 2048 slots, d 64 / 128 / 256."""
    return (hasattr(index, 'sequence_match') and 1 <= int(k_probe) <= 32 and int(max_sl) >= 1 and int(k_probe) * int(max_sl) <= 2048
            and getattr(index, 'd', None) in (64, 128, 256))


# NAFP_APPROX_INDEX=1: 'ivf' and 'ivfpq' build real approximate indexes (eval/ivf.py) with the reference's parameters
# (get_index_faiss.py:64-74, nprobe = 40 at :120) instead of being served by the exact search.
APPROX_INDEX_PARAMS = {'ivf': dict(nlist=400, nprobe=40), 'ivfpq': dict(nlist=256, M=64, nbits=8, nprobe=40)}


def approx_index_enabled():
    return os.environ.get('NAFP_APPROX_INDEX', '') == '1'


def ivfpq_rr_enabled():
    """NAFP_IVFPQ_RR=1 next to NAFP_APPROX_INDEX=1: 'ivfpq-rr' builds the IVFPQ-RR index (get_index_faiss.py's IndexIVFPQR:
    nlist 256, M 64 x 8 bits, refine 4 x 4 bits; k_factor 4, faiss's CPU default) instead of being served by the exact search."""
    return approx_index_enabled() and os.environ.get('NAFP_IVFPQ_RR', '') == '1'


def hnsw_enabled():
    """NAFP_HNSW=1 next to NAFP_APPROX_INDEX=1: 'hnsw' builds the HNSW index (get_index_faiss.py:88-96: IndexHNSWFlat, M 16,
    efConstruction 80, efSearch 16, search_bounded_queue) instead of being served by the exact search."""
    return approx_index_enabled() and os.environ.get('NAFP_HNSW', '') == '1'


def ivfpq_lut():
    """NAFP_IVFPQ_LUT: the ADC table precision of the opted-in 'ivfpq' index, 'f32' (default) or 'f16' (the reference's
    useFloat16 lookup tables)."""
    lut = os.environ.get('NAFP_IVFPQ_LUT', '') or 'f32'
    if lut not in ('f32', 'f16'):
        raise ValueError(f"NAFP_IVFPQ_LUT = {lut!r} ('f32' or 'f16')")
    return lut


def get_index(index_type, train_data, train_data_shape, use_gpu=True, max_nitem_train=2e7):
    """get_index_faiss.py:10-121 for the exact index (and, opted in, IVF / IVFPQ / IVFPQ-RR / HNSW).  The reference builds HNSW on
    the CPU only (faiss has no GPU HNSW); this build has it on the GPU only, so `use_gpu=False` raises for it as for every type."""
    mode = index_type.lower()
    if mode == 'l2':
        if not use_gpu:
            raise NotImplementedError('--nogpu: this build has no CPU search path')
        return FlatL2Index(int(train_data_shape[1]))
    if mode == 'hnsw' and hnsw_enabled():
        if not use_gpu:
            raise NotImplementedError('--nogpu: this build has no CPU search path')
        from .hnsw import HNSWIndex
        index = HNSWIndex(int(train_data_shape[1]), 16)          # nothing to train: max_nitem_train is unused, as in the reference
        index.efConstruction = 80
        index.efSearch = 16
        index.requested_type = index_type
        return index
    if (mode in APPROX_INDEX_PARAMS and approx_index_enabled()) or (mode == 'ivfpq-rr' and ivfpq_rr_enabled()):
        if not use_gpu:
            raise NotImplementedError('--nogpu: this build has no CPU search path')
        from .ivf import IVFFlatIndex, IVFPQIndex, IVFPQRIndex, training_subset
        p = APPROX_INDEX_PARAMS['ivfpq' if mode == 'ivfpq-rr' else mode]
        d = int(train_data_shape[1])
        if mode == 'ivf':
            index = IVFFlatIndex(d, p['nlist'])
        elif mode == 'ivfpq':
            index = IVFPQIndex(d, p['nlist'], p['M'], p['nbits'], lut=ivfpq_lut())
        else:
            index = IVFPQRIndex(d, p['nlist'], p['M'], p['nbits'], 4, 4, lut=ivfpq_lut())
        index.nprobe = p['nprobe']
        start_time = time.time()
        index.train(training_subset(train_data, max_nitem_train, index.seed))
        print(f'Trained {index.index_description} in {time.time() - start_time:.2f} sec.')
        index.requested_type = index_type
        return index
    if mode in ('ivf', 'ivfpq', 'ivfpq-rr', 'ivfpq-ondisk', 'hnsw'):
        # get_index_faiss.py:64-121 builds an approximate faiss index here (run.py:118 default 'ivfpq').  None of them is
        # built; the exact search over the HBM-resident table is the accuracy ceiling of every one of them, so the request
        # is served by it, with a notice (hit rates can only be >= what the approximate index would report).
        if not use_gpu:
            raise NotImplementedError('--nogpu: this build has no CPU search path')
        import sys
        print(f"eval: index_type '{index_type}' (approximate faiss index) is not built here; using the exact "
              "search 'L2' over the table resident in HBM instead.  Hit rates are an UPPER BOUND of what that index "
              "would report (max_nitem_train is ignored); the substitution is recorded in index_used.json.", file=sys.stderr)
        index = FlatL2Index(int(train_data_shape[1]))
        index.requested_type = index_type
        return index
    raise ValueError(mode.lower())


def resolve_test_ids(test_ids, n_query, test_seq_len):
    """eval_faiss.py:170-181."""
    if isinstance(test_ids, np.ndarray):
        return test_ids
    if test_ids.lower() == 'all':
        return np.arange(0, n_query - max(test_seq_len), 1)
    if test_ids.lower() == 'icassp':
        return np.load(glob.glob('./**/test_ids_icassp2021.npy', recursive=True)[0])
    if test_ids.isnumeric():
        return np.random.permutation(n_query - max(test_seq_len))[:int(test_ids)]
    return np.load(test_ids)


def search_and_score(index, query, test_ids, test_seq_len, k_probe, n_dummy, chunk_tasks=1 << 16, device_rank=False):
    """The batched form of the loop at eval_faiss.py:199-246.
    Returns (top1_exact, top1_near, top3_exact, top10_exact, pred_ids (n_test, n_len, 10)).
    device_rank: candidates, de-duplication, scores and ranking in one `index.sequence_match` launch per length and chunk; only
    the (T, 10) predicted ids come back to the host.  Same returns; NotImplementedError where `seq_match_supported` is false."""
    test_ids = np.asarray(test_ids, dtype=np.int64)
    test_seq_len = np.asarray(test_seq_len, dtype=np.int64)
    n_test, n_len = len(test_ids), len(test_seq_len)
    max_sl = int(test_seq_len.max())
    if device_rank and not seq_match_supported(index, k_probe, max_sl):
        raise NotImplementedError(f'device_rank: {type(index).__name__} with k_probe {k_probe} x sequence length {max_sl} is outside '
                                  'nafp_search_seq_match (k <= 32, k * length <= 2048 slots)')
    n_query = len(query)
    assert np.all(test_ids <= n_query)
    # distinct query rows any task touches (python slicing clips at the end of `query`)
    rows = (test_ids[:, None] + np.arange(max_sl)[None, :]).reshape(-1)
    rows = np.unique(rows[rows < n_query])
    pos = -np.ones(n_query + max_sl + 1, np.int64)
    pos[rows] = np.arange(len(rows))
    dev = index.device
    q_dev = torch.from_numpy(np.ascontiguousarray(query[rows], dtype=np.float32)).to(dev)
    _, I = index.search_device(q_dev, k_probe)                      # (n_rows, k) int32
    out = [np.zeros((n_test, n_len), int) for _ in range(4)]
    preds = -np.ones((n_test, n_len, 10), np.int64)

    def fill(a, b, si, p):
        gt = (test_ids[a:b] + n_dummy)[:, None]
        preds[a:b, si, :p.shape[1]] = p
        out[0][a:b, si] = (p[:, :1] == gt).any(1)
        out[1][a:b, si] = (np.abs(p[:, :1] - gt) <= 1).any(1) & (p[:, 0] >= 0)
        out[2][a:b, si] = (p[:, :3] == gt).any(1)
        out[3][a:b, si] = (p[:, :10] == gt).any(1)

    if device_rank:
        I = I.to(torch.int32).contiguous()
        for si, sl in enumerate(test_seq_len.tolist()):
            sl_eff = np.minimum(sl, n_query - test_ids)              # q = query[t : t+sl] clips at the end
            for a in range(0, n_test, chunk_tasks):
                b = min(n_test, a + chunk_tasks)
                q0 = torch.from_numpy(pos[test_ids[a:b]].astype(np.int32)).to(dev)      # rows of a task are consecutive in q_dev
                ln = torch.from_numpy(sl_eff[a:b].astype(np.int32)).to(dev)
                ids, _, _ = index.sequence_match(q_dev, I, q0, ln, n_out=10, max_len=max(int(sl), 1))
                fill(a, b, si, ids.cpu().numpy().astype(np.int64))
        return out[0], out[1], out[2], out[3], preds
    I = I.to(torch.int64)
    S = max_sl * k_probe
    offs = torch.arange(max_sl, device=dev)
    for si, sl in enumerate(test_seq_len.tolist()):
        sl_eff = np.minimum(sl, n_query - test_ids)                  # q = query[t : t+sl] clips at the end
        for a in range(0, n_test, chunk_tasks):
            b = min(n_test, a + chunk_tasks)
            t_ids = test_ids[a:b]
            T = b - a
            row_idx = pos[np.minimum(t_ids[:, None] + np.arange(max_sl)[None, :], n_query + max_sl)]   # (T, max_sl)
            valid = (np.arange(max_sl)[None, :] < sl_eff[a:b, None]) & (row_idx >= 0)
            ri = torch.from_numpy(np.where(valid, row_idx, 0)).to(dev)
            cand = I[ri] - offs[None, :, None]                       # offset compensation (eval_faiss.py:213-215)
            ok = torch.from_numpy(valid).to(dev)[:, :, None] & (I[ri] >= 0) & (cand >= 0)
            cand = torch.where(ok, cand, torch.full_like(cand, -1)).reshape(T, S).to(torch.int32).contiguous()
            q0 = torch.from_numpy(pos[t_ids].astype(np.int32)).to(dev)
            ln = torch.from_numpy(sl_eff[a:b].astype(np.int32)).to(dev)
            scores = index.sequence_scores(q_dev, q0, ln, cand)      # rows of a task are consecutive in q_dev
            c = cand.cpu().numpy().astype(np.int64)
            s = scores.cpu().numpy().astype(np.float64)
            # unique candidates (np.unique, eval_faiss.py:218), then score descending / id ascending
            order = np.argsort(c, axis=1, kind='stable')
            c = np.take_along_axis(c, order, 1); s = np.take_along_axis(s, order, 1)
            dup = np.zeros_like(c, dtype=bool)
            dup[:, 1:] = c[:, 1:] == c[:, :-1]
            s[dup | (c < 0)] = -np.inf
            rank = np.lexsort((c, -s), axis=1)[:, :10]
            p = np.take_along_axis(c, rank, 1)
            p[np.take_along_axis(s, rank, 1) == -np.inf] = -1
            fill(a, b, si, p)
    return out[0], out[1], out[2], out[3], preds


def eval_faiss(emb_dir, emb_dummy_dir=None, index_type='l2', nogpu=False, max_train=1e7, test_ids='icassp',
               test_seq_len='1 3 5 9 11 19', k_probe=20, display_interval=5):
    """eval_faiss.py:93-275."""
    if isinstance(test_seq_len, str):
        test_seq_len = np.asarray(list(map(int, test_seq_len.split())))
    query, query_shape = load_memmap_data(emb_dir, 'query')
    db, db_shape = load_memmap_data(emb_dir, 'db')
    if emb_dummy_dir is None:
        emb_dummy_dir = emb_dir
    dummy_db, dummy_db_shape = load_memmap_data(emb_dummy_dir, 'dummy_db')
    index = get_index(index_type, dummy_db, dummy_db.shape, (not nogpu), max_train)
    start_time = time.time()
    index.add(dummy_db); print(f'{len(dummy_db)} items from dummy DB')
    index.add(db); print(f'{len(db)} items from reference DB')
    print(f'Added total {index.ntotal} items to DB. {time.time() - start_time:>4.2f} sec.')
    print(f'test_id: \033[93m{test_ids}\033[0m,  ', end='')
    test_ids = resolve_test_ids(test_ids, len(query), test_seq_len)
    n_test = len(test_ids)
    print(f'n_test: \033[93m{n_test:n}\033[0m')
    start_time = time.time()
    device_rank = False
    if seq_match_enabled():
        device_rank = seq_match_supported(index, k_probe, int(np.max(test_seq_len)))
        if not device_rank:
            import sys
            print(f'eval: NAFP_SEQ_MATCH=1, but k_probe {k_probe} x sequence length {int(np.max(test_seq_len))} is outside the device '
                  'ranking (k <= 32, k * length <= 2048 slots); ranking on the host instead.', file=sys.stderr)
    top1_exact, top1_near, top3_exact, top10_exact, _ = search_and_score(index, query, test_ids, test_seq_len, k_probe,
                                                                        int(dummy_db_shape[0]), device_rank=device_rank)
    torch.cuda.synchronize()
    dt = time.time() - start_time
    rates = [100. * np.mean(m, axis=0) for m in (top1_exact, top1_near, top3_exact, top10_exact)]
    print(f'{n_test} test ids x {len(test_seq_len)} lengths in {dt:.2f} s ({dt / max(n_test * len(test_seq_len), 1) * 1e3:.3f} ms per query sequence)')
    print('segments      ' + ''.join(f'{int(s):>8d}' for s in test_seq_len))
    for name, r in zip(['Top1 exact', 'Top1 near', 'Top3 exact', 'Top10 exact'], rates):
        print(f'{name:<14s}' + ''.join(f'{v:8.2f}' for v in r))
    np.save(f'{emb_dir}/raw_score.npy', np.concatenate((top1_exact, top1_near, top3_exact, top10_exact), axis=1))
    np.save(f'{emb_dir}/test_ids.npy', test_ids)
    # the reference's result files carry no index type; when the requested (approximate) type was served by the exact
    # search the numbers are not comparable with the reference's IVF-PQ figures: say so NEXT TO them
    import json
    requested = getattr(index, 'requested_type', index_type)
    rank_note = {'sequence_rank': 'device'} if device_rank else {}      # only when NAFP_SEQ_MATCH=1 served the run
    if hasattr(index, 'index_description'):                     # an approximate index really served the run (opted in)
        with open(f'{emb_dir}/index_used.json', 'w') as f:
            json.dump({'index_type_requested': requested, 'index_type_used': index.index_description, 'substituted': False,
                       'k_probe': int(k_probe), 'note': 'hit rates in raw_score.npy are those of the approximate index '
                                                        '(NAFP_APPROX_INDEX=1)', **rank_note}, f, indent=1)
        print(f'Saved test_ids and raw score to {emb_dir}.')
        return rates
    with open(f'{emb_dir}/index_used.json', 'w') as f:
        json.dump({'index_type_requested': requested, 'index_type_used': 'L2 (exact, HIP FlatL2Index)',
                   'substituted': requested.lower() != 'l2', 'k_probe': int(k_probe),
                   'note': 'approximate faiss index types are served by the exact search: hit rates in raw_score.npy are an '
                           'upper bound of what the requested index would give' if requested.lower() != 'l2' else 'exact search as requested',
                   **rank_note}, f, indent=1)
    print(f'Saved test_ids and raw score to {emb_dir}.')
    return rates
