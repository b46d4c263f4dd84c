"""Training / validation batches: (anchors, augmented replicas) assembled ON THE DEVICE.

Host mirror of the reference's `genUnbalSequence` (model/utils/dataloader_keras.py:11-482) for its
training and validation use (model/dataset.py:118-186): same constructor arguments, same
enumeration (`fns_event_seg_list` = [file, seg_idx, offset_min, offset_max], audio_utils.py:140-218),
same batch composition (n_anchor anchors + n_pos_per_anchor replicas each, replicas in anchor order),
same selection of background / speech / impulse-response items per batch index
(dataloader_keras.py:223-311), same distributions of the random draws (anchor / replica offsets
within +-offset_margin, background offset, SNR uniform in snr_range, amplitude ratio log-uniform in
(0.1, 1)).  `__getitem__` returns float32 CUDA tensors (n_anchor, 1, T), (n_pos, 1, T).

What is different, on purpose:
  * every WAV of every list is read ONCE into one int16 arena resident in HBM (`PcmStore`; the whole
    10k x 30 s training set is 4.8 GB of 288 GB).  A batch is then only a table of windows
    (`nafp_aug_row`, 64 B per row) and ONE kernel launch (`nafp_augment_rows`): no file I/O, no
    np.vstack, no host FFT per step;
  * random draws come from numpy Generators (the reference's global `np.random` stream cannot be
    matched, and it re-seeds that global stream with the sample index for every anchor,
    dataloader_keras.py:327-331, which makes the anchor offsets a function of the index; here every
    batch draws from Generator([seed, epoch, batch index]), vectorised over the batch);
  * `randint(low, high)` with low >= high (single-segment files) raises in the reference; here it
    yields `low`;
  * `speed_mix_parameter=[True, (lo, hi), n]` (no argument of the reference's): every replica is played at a speed drawn
    uniformly from a grid of n speeds over [lo, hi], tempo and pitch together, inside the same launch (`plan_speed`, a table of
    `nafp_aug_speed` next to the row table, and `nafp_augment_rows_speed`).  Without it every call and every byte is as before.
Unsupported (NotImplementedError): experimental_mode, amp_mode other than 'normal', seg_mode other than 'all'.
"""
import numpy as np
import torch

from ... import _lib
from . import ingest as ig
from .audio_utils import FileCatalog, n_segments

MAX_IR_LENGTH = 600          # dataloader_keras.py:8


def segment_table(n_frames, fs, duration, hop, mode='all'):
    """(seg_idx, offset_min, offset_max) rows of one file (audio_utils.py:151-218)."""
    n_seg_frames, n_hop_frames = fs * duration, fs * hop
    n_segs = n_segments(n_frames, fs, duration, hop)
    residual = int(max(0, n_frames - ((n_segs - 1) * n_hop_frames + n_seg_frames)))
    if mode == 'first':
        return [(0, 0, 0)]
    if mode != 'all':
        raise NotImplementedError(f'seg_mode={mode}')
    out = []
    for s in range(n_segs):
        lo, hi = int(-1 * n_hop_frames), int(n_hop_frames)
        if s == 0:
            lo = 0
        if s == n_segs - 1:
            hi = residual
        out.append((s, lo, hi))
    return out


class PcmStore(FileCatalog):
    """All samples of a list of WAV files in ONE int16 array at the model rate: the catalog of the files (audio_utils.FileCatalog,
    with `n_frames` as an int64 array) plus their placement, `start[f]` (first sample of file f, 8-sample aligned) from `base` to
    `end`.  `.host()` materialises it in numpy (tests, small sets), `.device()` uploads it once through a pinned staging buffer.
    A file the device converts (`resampled[f]`, under the opt-in layers) is converted into its place by `.device()`; `.host()`
    raises for it (there is no CPU path)."""

    def __init__(self, fns, fs, base=0):
        super().__init__(fns, fs)
        self.n_frames = np.asarray(self.n_frames, np.int64)
        sizes = (self.n_frames + 7) // 8 * 8
        self.start = int(base) + np.cumsum(sizes) - sizes
        self.base, self.end = int(base), int(base) + int(sizes.sum())

    def read_into(self, dst, f0=0, f1=None, leave_converted=False):
        """dst: int16 numpy view (zero-initialised by the caller) of the places of the files [f0, f1) (default: all, [base, end)).
        leave_converted: a file the device converts stays zero instead of raising."""
        f1 = len(self.fns) if f1 is None else f1
        for f in range(f0, f1):
            e = self.files[f]
            if e.resampled and leave_converted:
                continue
            if e.resampled and self.ingest:
                raise NotImplementedError(f'{e.fn}: {e.rate} Hz x {e.channels} x {e.format} is decoded and resampled '
                                          'on the device only (PcmArena.device); there is no CPU path')
            if e.resampled:
                raise NotImplementedError(f'{e.fn}: {e.rate} Hz x {e.channels} is resampled on the device only '
                                          '(PcmArena.device); there is no CPU resampler')
            if e.n_frames:
                with open(e.fn, 'rb', buffering=0) as fh:
                    fh.seek(e.data_offset)
                    a = int(self.start[f] - self.start[f0])
                    got = fh.readinto(memoryview(dst[a:a + e.n_frames]).cast('B'))
                    if got != 2 * e.n_frames:
                        raise IOError(f'{e.fn}: short read')


class PcmArena:
    """Several PcmStores back to back in one arena (event | bg | speech | ir)."""

    def __init__(self, stores):
        self.stores = stores
        self.total = max([s.end for s in stores] + [8])

    def host(self):
        a = np.zeros(self.total, np.int16)
        for s in self.stores:
            s.read_into(a[s.base:s.end])
        return a

    def device(self, device=None, piece=1 << 25):
        device = device or torch.device('cuda', torch.cuda.current_device())
        d = torch.zeros((self.total,), dtype=torch.int16, device=device)
        n_stage = min(piece, self.total)
        if any(any(s.resampled) for s in self.stores):     # raw frames of a file to resample: several per output sample
            n_stage = max(n_stage, min(piece, 1 << 22))
        stage = torch.zeros((n_stage,), dtype=torch.int16).pin_memory()
        for s in self.stores:                      # per store, in pieces of whole files
            f = 0
            while f < len(s.fns):
                g, a0 = f, int(s.start[f])
                while g < len(s.fns) and int(s.start[g]) + (int(s.n_frames[g]) + 7) // 8 * 8 - a0 <= stage.shape[0]:
                    g += 1
                if g == f:
                    raise NotImplementedError(f'{s.fns[f]}: one file larger than the staging buffer')
                a1 = int(s.start[g - 1]) + (int(s.n_frames[g - 1]) + 7) // 8 * 8
                buf = stage.numpy()[:a1 - a0]
                buf[:] = 0
                s.read_into(buf, f, g, leave_converted=True)     # files to convert leave their place zero here and are filled below
                d[a0:a1].copy_(stage[:a1 - a0], non_blocking=False)
                f = g
            for f in range(len(s.fns)):
                if s.resampled[f]:
                    self._convert_file(s, f, d, stage)
        if any(any(s.resampled) for s in self.stores):
            torch.cuda.current_stream(device).synchronize()
        return d

    @staticmethod
    def _convert_file(s, f, d, stage):
        """File f of store s -> d[start[f] : start[f] + n_frames[f]] at the model rate: its bytes go through the staging buffer in
        runs of outputs (ingest.file_runs: each run uploads the one byte range its outputs need -- frames, whole codec blocks or
        whole FLAC frames) and every run is a launch of one piece.  FLAC frames that fail their checks are zeros; each is counted
        once, on the device, in s.flac_failed."""
        stage_bytes = stage.numpy().view(np.uint8)
        with open(s.fns[f], 'rb', buffering=0) as fh:
            for n0, n1, run in ig.file_runs(s.files[f], s.fs, int(s.start[f]), len(stage_bytes), s.flac_failed):
                (fn, file_off, n_bytes, _), = run.reads
                if n_bytes:
                    fh.seek(file_off)
                    if fh.readinto(memoryview(stage_bytes[:n_bytes])) != n_bytes:
                        raise IOError(f'{fn}: short read')
                raw = stage[:max((n_bytes + 1) // 2, 1)].to(d.device, non_blocking=False)
                run.work(d.numel()).run(raw, out=d)

    def flac_failed_frames(self):
        """Frames of the stores' FLAC files that failed their checks in `.device()` (one read of the device flags per store)."""
        return sum(s.flac_failed.count() for s in self.stores if s.flac_failed is not None)


def _randint(rng, low, high, size=None):
    """np.random.randint(low, high) (exclusive high); low >= high -> low (see module docstring)."""
    if high <= low:
        return low if size is None else np.full(size, low, dtype=np.int64)
    return rng.integers(low, high, size=size)


SPEED_ONE = 1 << 24          # the Q24 step of "no speed change"
SPEED_MIN, SPEED_MAX = 0.8, 1.25
SPEED_MAX_STEPS = 32         # nafp_aug_speedset_create


def speed_grid(speed_mix_parameter):
    """`[True, (lo, hi), n]` -> (speeds, steps): s_k = lo + k (hi - lo) / (n - 1), k < n (n = 1: lo must equal hi);
    step_k = round(2^24 s_k), duplicates removed (the speed kept for a step is the first that gave it).  `[False, ...]` -> ([], []).
    ValueError, before anything touches the GPU: n < 1, lo > hi, n = 1 with lo != hi, a speed outside 0.8 .. 1.25, more than 32
    distinct steps."""
    if not speed_mix_parameter[0]:
        return [], []
    if len(speed_mix_parameter) != 3 or len(speed_mix_parameter[1]) != 2:
        raise ValueError(f'speed_mix_parameter={speed_mix_parameter!r}: expected [True, (lo, hi), n]')
    (lo, hi), n = speed_mix_parameter[1], speed_mix_parameter[2]
    lo, hi = float(lo), float(hi)
    if int(n) != n or n < 1:
        raise ValueError(f'speed_mix_parameter: n={n!r} must be an integer >= 1')
    if not lo <= hi:
        raise ValueError(f'speed_mix_parameter: lo={lo} > hi={hi}')
    if n == 1 and lo != hi:
        raise ValueError(f'speed_mix_parameter: n=1 needs lo == hi, got ({lo}, {hi})')
    if not (SPEED_MIN <= lo and hi <= SPEED_MAX):
        raise ValueError(f'speed_mix_parameter: speeds ({lo}, {hi}) outside the supported range {SPEED_MIN} .. {SPEED_MAX}')
    speeds, steps = [], []
    for k in range(int(n)):
        s = lo if n == 1 else lo + k * (hi - lo) / (n - 1)
        step = int(round(SPEED_ONE * s))
        if step not in steps:
            speeds.append(s); steps.append(step)
    if len(steps) > SPEED_MAX_STEPS:
        raise ValueError(f'speed_mix_parameter: {len(steps)} distinct steps, at most {SPEED_MAX_STEPS} are supported')
    return speeds, steps


def speed_out0(start, seg_len, step):
    """First output of a speed row, centre-aligned with the plain window [start, start + seg_len) of the same file: the output
    nearest the window's centre sample c (n step / 2^24 ~ c) sits at seg_len // 2, clamped at the start of the stream."""
    c = np.asarray(start, np.int64) + seg_len // 2
    step = np.asarray(step, np.int64)
    return np.maximum(0, (c * SPEED_ONE + step // 2) // step - seg_len // 2)


class genUnbalSequence:
    def __init__(self, fns_event_list, bsz=120, n_anchor=60, duration=1, hop=.5, fs=8000, shuffle=False,
                 seg_mode='all', amp_mode='normal', random_offset_anchor=False, offset_margin_hop_rate=0.4,
                 bg_mix_parameter=[False], ir_mix_parameter=[False], speech_mix_parameter=[False], reduce_items_p=0,
                 reduce_batch_first_half=False, experimental_mode=False, drop_the_last_non_full_batch=True,
                 seed=0, device=None, resident=True, shard=(0, 1), speed_mix_parameter=[False]):
        if experimental_mode:
            raise NotImplementedError('experimental_mode')
        # replicas played at a speed drawn from a grid (tempo and pitch together): the grid's steps; the slot of each grid entry in
        # the step set of the kernel (the unity step has none, -1: such replicas are plain rows)
        self.speed_mix = bool(speed_mix_parameter[0])
        self.speed_grid, self.speed_grid_steps = speed_grid(speed_mix_parameter)
        self.speed_steps = [s for s in self.speed_grid_steps if s != SPEED_ONE]
        self.speed_grid_slot = np.asarray([self.speed_steps.index(s) if s != SPEED_ONE else -1 for s in self.speed_grid_steps], np.int32)
        self._speedset = None
        self.reduce_batch_first_half = reduce_batch_first_half
        if amp_mode != 'normal':
            raise NotImplementedError(f'amp_mode={amp_mode}')
        if seg_mode != 'all':
            raise NotImplementedError('seg_mode={}'.format(seg_mode))
        self.bsz, self.n_anchor = bsz, n_anchor
        if bsz != n_anchor:
            self.n_pos_per_anchor = round((bsz - n_anchor) / n_anchor)
            self.n_pos_bsz = bsz - n_anchor
        else:
            self.n_pos_per_anchor = 0
            self.n_pos_bsz = 0
        self.duration, self.hop, self.fs, self.shuffle = duration, hop, fs, shuffle
        self.random_offset_anchor = random_offset_anchor
        self.offset_margin_frame = int(hop * offset_margin_hop_rate * fs)
        self.seg_len = int(duration * fs)
        self.bg_mix, self.ir_mix, self.speech_mix = bg_mix_parameter[0], ir_mix_parameter[0], speech_mix_parameter[0]
        self.rng = np.random.default_rng(seed)
        self.seed, self.epoch = int(seed), 0
        # ---- stores + segment tables -------------------------------------------------------
        stores, pos = [], 0

        def add_store(fns):
            nonlocal pos
            s = PcmStore(fns, fs, base=pos)
            pos = s.end
            stores.append(s)
            return s

        def seg_list(store, dur, hp, mode='all'):
            rows = []                                       # (file, seg_idx, offset_min, offset_max)
            for f in range(len(store.fns)):
                rows += [(f,) + t for t in segment_table(int(store.n_frames[f]), fs, dur, hp, mode)]
            return np.asarray(rows, np.int64).reshape(-1, 4)

        self.ev = add_store(fns_event_list)
        self.fns_event_seg_list = seg_list(self.ev, duration, hop)
        if drop_the_last_non_full_batch:
            self.n_samples = int((len(self.fns_event_seg_list) // n_anchor) * n_anchor)
        else:
            self.n_samples = len(self.fns_event_seg_list)
        self.index_event = self.rng.permutation(self.n_samples) if shuffle else np.arange(self.n_samples)
        if self.bg_mix:
            self.bg = add_store(bg_mix_parameter[1]); self.bg_snr_range = bg_mix_parameter[2]
            self.fns_bg_seg_list = seg_list(self.bg, duration, duration)
            self.n_bg_samples = len(self.fns_bg_seg_list)
            self.index_bg = self.rng.permutation(self.n_bg_samples) if shuffle else np.arange(self.n_bg_samples)
        if self.speech_mix:
            self.sp = add_store(speech_mix_parameter[1]); self.speech_snr_range = speech_mix_parameter[2]
            self.fns_speech_seg_list = seg_list(self.sp, duration, duration)
            self.n_speech_samples = len(self.fns_speech_seg_list)
            self.index_speech = self.rng.permutation(self.n_speech_samples) if shuffle else np.arange(self.n_speech_samples)
        if self.ir_mix:
            self.ir = add_store(ir_mix_parameter[1])
            self.fns_ir_seg_list = seg_list(self.ir, duration, duration, 'first')
            self.n_ir_samples = len(self.fns_ir_seg_list)
            self.index_ir = self.rng.permutation(self.n_ir_samples) if shuffle else np.arange(self.n_ir_samples)
        self.reduce_items_p = reduce_items_p
        assert reduce_items_p <= 100
        # data parallel: bsz / n_anchor are the GLOBAL batch, every rank builds the SAME permutation and the
        # same draws (same seed) and keeps rows [rank * n_anchor/world, (rank+1) * n_anchor/world) of each batch
        # with their replicas, so that len(ds), the epoch and the batches equal the single-process run
        self.rank, self.world = int(shard[0]), int(shard[1])
        if not 0 <= self.rank < self.world or n_anchor % self.world:
            raise ValueError(f'shard={shard}: n_anchor={n_anchor} must split evenly over the ranks')
        self.arena = PcmArena(stores)
        self.device = device
        self._pcm = None
        self._lib = None
        if not resident:
            raise NotImplementedError('streaming (non-resident) PCM arena')
        self.set_epoch(0)

    def __len__(self):
        """dataloader_keras.py:187-195."""
        if self.reduce_items_p != 0:
            return int(np.ceil(self.n_samples / float(self.n_anchor)) * (self.reduce_items_p / 100))
        return int(np.ceil(self.n_samples / float(self.n_anchor)))

    def on_epoch_end(self):
        """dataloader_keras.py:198-222."""
        self.set_epoch(self.epoch + 1)

    def set_epoch(self, epoch):
        """Permutations of epoch `epoch` (0-based): a function of (seed, epoch) only, so a restarted run that
        resumes at epoch e continues with the permutations and draws the uninterrupted run would have used."""
        self.epoch = int(epoch)
        if self.shuffle:
            rng = np.random.default_rng([self.seed, 0x5eed, self.epoch])
            self.index_event = rng.permutation(self.n_samples)
            if self.bg_mix:
                self.index_bg = rng.permutation(self.n_bg_samples)
            if self.ir_mix:
                self.index_ir = rng.permutation(self.n_ir_samples)
            if self.speech_mix:
                self.index_speech = rng.permutation(self.n_speech_samples)

    # ---- the batch as a table of windows (host only; unit-testable without a GPU) -----------
    def plan(self, idx):
        """nafp_aug_row table of batch `idx`: rows [0, n_anchor) anchors, then the replicas in anchor
        order (dataloader_keras.py:223-311, 316-398).  Vectorised over the batch.  The same bytes with and without
        `speed_mix_parameter`: a speed row keeps its plain ev_off / ev_valid, which the kernel ignores for it."""
        return self._plan(idx)[0]

    def plan_speed(self, idx):
        """nafp_aug_speed table of batch `idx`, parallel to `plan(idx)` (same order, same rank slice).  Anchors, replicas that
        drew the unity step and every row of a loader without `speed_mix_parameter` have slot -1 (and zeros otherwise).  One
        draw per replica, uniform over the grid, made after every draw of `plan`."""
        return self._plan(idx)[1]

    def _plan(self, idx):
        anchors = self.index_event[idx * self.n_anchor:(idx + 1) * self.n_anchor]
        nA, npa, T = len(anchors), self.n_pos_per_anchor, self.seg_len
        nP = nA * npa
        rows = np.zeros(nA + nP, dtype=_lib.AUG_ROW_DTYPE)
        rows['nz_off'] = -1; rows['nz2_off'] = -1; rows['ir_off'] = -1; rows['amp'] = 1.0
        rng = np.random.default_rng([self.seed, self.epoch, int(idx)])
        tab = self.fns_event_seg_list[anchors]                       # (nA, 4): file, seg, offset_min, offset_max
        f, seg, off_min, off_max = tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3]
        m = self.offset_margin_frame
        if self.random_offset_anchor:
            lo, hi = np.maximum(off_min, -m), np.minimum(off_max, m)
            a_off = np.where(hi > lo, rng.integers(lo, np.maximum(hi, lo + 1)), lo)     # randint(low, high), exclusive high
        else:
            a_off = np.zeros(nA, np.int64)
        start_of = lambda off: np.floor((seg[:, None] * self.hop + off / self.fs) * self.fs).astype(np.int64)
        starts = start_of(a_off[:, None])                            # (nA, 1)
        if npa > 0:
            p_min, p_max = np.maximum(a_off - m, off_min), np.minimum(a_off + m, off_max)
            draw = rng.integers(p_min[:, None], np.maximum(p_max, p_min + 1)[:, None], size=(nA, npa))
            p_off = np.where((p_max > p_min)[:, None], draw, p_min[:, None])
            # p_min == p_max == 0 (dataloader_keras.py:361-366) is the constant case of the line above
            starts = np.concatenate([starts, start_of(p_off)], axis=1)    # (nA, 1 + npa)
        n_fr, base = self.ev.n_frames[f], self.ev.start[f]
        ev_off = base[:, None] + starts
        ev_valid = np.clip(n_fr[:, None] - starts, 0, T)
        rows['ev_off'][:nA] = ev_off[:, 0]; rows['ev_valid'][:nA] = ev_valid[:, 0]
        if nP > 0:
            rows['ev_off'][nA:] = ev_off[:, 1:].reshape(-1); rows['ev_valid'][nA:] = ev_valid[:, 1:].reshape(-1)
            sel = np.arange(idx * self.n_pos_bsz, idx * self.n_pos_bsz + nP)
            rep = slice(nA, nA + nP)

            def noise_windows(store, seg_list, index, n_items):
                """__bg_batch_load / __speech_batch_load (dataloader_keras.py:400-452)."""
                t = seg_list[index[sel % n_items] % n_items]
                rnd = rng.integers(0, max(int(self.duration * self.fs / 2), 1), size=nP)
                offset_sec = np.minimum(rnd / self.fs, t[:, 3] / self.fs)
                st = np.floor((t[:, 1] * self.duration + offset_sec) * self.fs).astype(np.int64)
                return store.start[t[:, 0]] + st, np.clip(store.n_frames[t[:, 0]] - st, 0, T)

            snr_range = None
            if self.bg_mix:
                rows['nz_off'][rep], rows['nz_valid'][rep] = noise_windows(self.bg, self.fns_bg_seg_list, self.index_bg, self.n_bg_samples)
                snr_range = self.bg_snr_range
            if self.speech_mix:
                key = 'nz2' if self.bg_mix else 'nz'
                rows[key + '_off'][rep], rows[key + '_valid'][rep] = noise_windows(self.sp, self.fns_speech_seg_list, self.index_speech,
                                                                                 self.n_speech_samples)
                # both: noise = bg + speech mixed at speech_snr_range (:241-259); speech alone uses bg_snr_range (:291-294)
                snr_range = self.speech_snr_range if self.bg_mix else getattr(self, 'bg_snr_range', self.speech_snr_range)
            if snr_range is not None:
                lo, hi = float(np.min(snr_range)), float(np.max(snr_range))
                rows['snr_db'][rep] = rng.random(nP) * (hi - lo) + lo                               # audio_utils.py:92-95
                rows['amp'][rep] = np.power(10.0, rng.random(nP) * (np.log10(1.0) - np.log10(0.1)) + np.log10(0.1))   # :75-79
                rows['mix'][rep] = 1
            if self.ir_mix:
                fi = self.fns_ir_seg_list[self.index_ir[sel % self.n_ir_samples] % self.n_ir_samples][:, 0]
                rows['ir_off'][rep] = self.ir.start[fi]
                rows['ir_len'][rep] = np.minimum(np.minimum(self.ir.n_frames[fi], MAX_IR_LENGTH), T)
        speeds = np.zeros(nA + nP, dtype=_lib.AUG_SPEED_DTYPE)
        speeds['slot'] = -1
        if self.speed_mix and nP > 0:
            k = rng.integers(0, len(self.speed_grid_steps), size=nP)          # the last draw of the batch: no other draw moves
            slot = self.speed_grid_slot[k]
            on = slot >= 0
            fr = np.repeat(f, npa)
            sp = speeds[nA:]
            sp['slot'] = slot
            sp['file_off'] = np.where(on, self.ev.start[fr], 0)
            sp['n_in'] = np.where(on, self.ev.n_frames[fr], 0)
            sp['out0'] = np.where(on, speed_out0(starts[:, 1:].reshape(-1), T, np.asarray(self.speed_grid_steps, np.int64)[k]), 0)
        if self.world > 1:
            # this rank's anchors of the global batch and their replicas (a ragged last batch splits as evenly
            # as its anchors allow)
            a0, a1 = (nA * self.rank) // self.world, (nA * (self.rank + 1)) // self.world
            rows = np.concatenate([rows[a0:a1], rows[nA + a0 * npa:nA + a1 * npa]])
            speeds = np.concatenate([speeds[a0:a1], speeds[nA + a0 * npa:nA + a1 * npa]])
        return rows, speeds

    def n_local_anchors(self, idx):
        nA = min(self.n_anchor, self.n_samples - idx * self.n_anchor)
        return (nA * (self.rank + 1)) // self.world - (nA * self.rank) // self.world

    # ---- device ---------------------------------------------------------------------------
    def _resident(self):
        if self._pcm is None:
            self._pcm = self.arena.device(self.device)
            self._lib = _lib.load()
        return self._pcm

    def speedset(self):
        """The nafp_aug_speedset of the grid's steps (None without a step other than unity).  Host only until its first launch."""
        if self._speedset is None and self.speed_steps:
            import ctypes
            h = ctypes.c_void_p()
            steps = np.asarray(self.speed_steps, np.uint32)
            lib = _lib.load()
            _lib.check(lib.nafp_aug_speedset_create(ctypes.byref(h), steps.ctypes.data_as(ctypes.c_void_p), len(steps)), 'aug_speedset_create')
            self._speedset, self._speedset_destroy = h, lib.nafp_aug_speedset_destroy      # (kept: module globals are gone at exit)
        return self._speedset

    def __del__(self):
        if getattr(self, '_speedset', None):
            h, self._speedset = self._speedset, None
            self._speedset_destroy(h)

    def check_speed(self, rows, speeds):
        """The kernel's own per-row checks of a speed table, on the host (nafp_augment_speed_check_host)."""
        import ctypes
        rows = np.ascontiguousarray(rows, dtype=_lib.AUG_ROW_DTYPE)
        speeds = np.ascontiguousarray(speeds, dtype=_lib.AUG_SPEED_DTYPE)
        if len(rows) != len(speeds):
            raise ValueError(f'{len(speeds)} speed entries for {len(rows)} rows')
        _lib.check(_lib.load().nafp_augment_speed_check_host(self.speedset(), rows.ctypes.data_as(ctypes.c_void_p),
                                                            speeds.ctypes.data_as(ctypes.c_void_p), len(rows), self.arena.total,
                                                            self.seg_len), 'augment speed table')
        return speeds

    def run(self, rows, speeds=None):
        """(n_rows, 1, T) float32 CUDA batch of a row table, with its speed table if there is one."""
        pcm = self._resident()
        d_rows = torch.from_numpy(rows.view(np.uint8).reshape(-1)).to(pcm.device)
        out = torch.empty((len(rows), 1, self.seg_len), dtype=torch.float32, device=pcm.device)
        if speeds is not None and self.speedset() is not None and len(rows):
            speeds = self.check_speed(rows, speeds)
            d_speeds = torch.from_numpy(speeds.view(np.uint8).reshape(-1)).to(pcm.device)
            with torch.cuda.device(pcm.device):
                _lib.check(self._lib.nafp_augment_rows_speed(self.speedset(), _lib.ptr(pcm), pcm.numel(), _lib.ptr(d_rows),
                                                             _lib.ptr(d_speeds), len(rows), self.seg_len, _lib.ptr(out),
                                                             _lib.current_stream()), 'augment_rows_speed')
            return out
        with torch.cuda.device(pcm.device):
            _lib.check(self._lib.nafp_augment_rows(_lib.ptr(pcm), _lib.ptr(d_rows), len(rows), self.seg_len, _lib.ptr(out),
                                                   _lib.current_stream()), 'augment_rows')
        return out

    def __getitem__(self, idx):
        if idx < 0 or idx >= len(self):
            raise IndexError(idx)
        nA = self.n_local_anchors(idx)
        if self.speed_mix:
            rows, speeds = self._plan(idx)
            if self.reduce_batch_first_half:
                return self.run(rows[nA:], speeds[nA:]), []
            out = self.run(rows, speeds)
            return out[:nA], out[nA:]
        rows = self.plan(idx)
        if self.reduce_batch_first_half:           # synthesized queries only (dataloader_keras.py:308-309): the anchors are not built
            return self.run(rows[nA:]), []
        out = self.run(rows)
        return out[:nA], out[nA:]
