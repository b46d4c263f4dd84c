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
    yields `low`.
Unsupported (NotImplementedError): experimental_mode, amp_mode other than 'normal', seg_mode other than 'all'.
"""
import numpy as np
import torch

from ... import _lib
from .audio_utils import n_segments, riff_scan, riff_scan_ex, flac_scan, _resample_on, _ingest_on, _codecs_on, _flac_on, _taken_name

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


class PcmStore:
    """All samples of a list of 16-bit mono WAV files in ONE int16 array: `start[f]` (first sample of
    file f, 8-sample aligned), `n_frames[f]`.  `.host()` materialises it in numpy (tests, small sets),
    `.device()` uploads it once through a pinned staging buffer.  With NAFP_RESAMPLE=1 files at other rates / in stereo are
    taken too (utils/resample.py): `n_frames` / `start` then count samples at `fs`, `.device()` resamples such a file into its
    place on the device and `.host()` raises (there is no CPU resampler)."""

    def __init__(self, fns, fs, base=0):
        self.fns, self.fs = list(fns), fs
        self.n_frames, self.data_offset, self.start = [], [], []
        # NAFP_INGEST_ANY=1 (includes NAFP_RESAMPLE=1): any PCM / float format, 1 to 8 channels, rates in either direction
        # NAFP_INGEST_CODECS=1 (includes both): A-law, mu-law, IMA and MS ADPCM too; `spb` is the frames per block_align bytes
        # NAFP_INGEST_FLAC=1 (includes all three): `.flac` names too; `flac_index[f]` is the file's frame index (utils/flac.py) and
        # `flac_failed` counts, on the device, the frames that failed their checks while `.device()` decoded them
        self.flac = _flac_on()
        self.flac_index, self.flac_failed = {}, None
        self.codecs = _codecs_on()
        self.ingest = _ingest_on()
        self.resample = _resample_on() or self.ingest
        self.rate, self.channels, self.n_in, self.resampled = [], [], [], []
        self.format, self.block_align, self.spb = [], [], []
        pos = int(base)
        for fn in self.fns:
            if not _taken_name(fn, self.flac):
                raise NotImplementedError(fn[-3:])
            if self.ingest:
                from . import ingest as ig
                if fn[-3:] != 'wav':
                    info = flac_scan(fn, fs)
                    self.flac_index[len(self.n_frames)] = info['index']
                else:
                    info = riff_scan_ex(fn, fs, codecs=True) if self.codecs else riff_scan_ex(fn, fs)
                rate, ch, off, nfr = info['rate'], info['channels'], info['offset'], info['n_frames']
                native = ig.is_native(info, fs)
                n_model = nfr if native else ig.n_out(nfr, rate, fs)
                self.format.append(info['format']); self.block_align.append(info['block_align'])
                self.spb.append(info.get('samples_per_block', 1))
                self.n_frames.append(n_model); self.data_offset.append(off); self.start.append(pos)
                self.rate.append(rate); self.channels.append(ch); self.n_in.append(nfr); self.resampled.append(not native)
                pos += (n_model + 7) // 8 * 8
                continue
            rate, ch, width, off, nfr = riff_scan(fn)
            if self.resample:
                from . import resample as rs
                rs.check_file(fn, rate, ch, width, fs)
                native = rate == fs and ch == 1
                n_model = nfr if native else rs.n_out(nfr, rate, fs)
            else:
                if rate != fs:
                    raise ValueError('Sample rate should be {} but got {}'.format(str(fs), str(rate)))
                if width != 2 or ch != 1:
                    raise ValueError(f'{fn}: expected 16-bit mono PCM')
                native, n_model = True, nfr
            self.n_frames.append(n_model); self.data_offset.append(off); self.start.append(pos)
            self.rate.append(rate); self.channels.append(ch); self.n_in.append(nfr); self.resampled.append(not native)
            pos += (n_model + 7) // 8 * 8
        self.base, self.end = int(base), pos
        self.n_frames = np.asarray(self.n_frames, np.int64)
        self.start = np.asarray(self.start, np.int64)

    def read_into(self, dst):
        """dst: int16 numpy view of [base, end) (zero-initialised by the caller)."""
        for f, fn in enumerate(self.fns):
            n = int(self.n_frames[f])
            if self.resampled[f] and getattr(self, 'ingest', False):
                raise NotImplementedError(f'{fn}: {self.rate[f]} Hz x {self.channels[f]} x {self.format[f]} is decoded and resampled '
                                          'on the device only (PcmArena.device); there is no CPU path')
            if self.resampled[f]:
                raise NotImplementedError(f'{fn}: {self.rate[f]} Hz x {self.channels[f]} is resampled on the device only '
                                          '(PcmArena.device); there is no CPU resampler')
            if n:
                with open(fn, 'rb', buffering=0) as fh:
                    fh.seek(self.data_offset[f])
                    a = int(self.start[f] - self.base)
                    got = fh.readinto(memoryview(dst[a:a + n]).cast('B'))
                    if got != 2 * n:
                        raise IOError(f'{fn}: short read')


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
                sub = PcmStore.__new__(PcmStore)
                sub.fns, sub.n_frames, sub.data_offset, sub.start, sub.base = s.fns[f:g], s.n_frames[f:g], s.data_offset[f:g], s.start[f:g], a0
                # files to resample leave their place zero here and are filled below
                sub.resampled = [False] * (g - f)
                sub.n_frames = np.where(np.asarray(s.resampled[f:g], bool), 0, sub.n_frames)
                sub.read_into(buf)
                d[a0:a1].copy_(stage[:a1 - a0], non_blocking=False)
                f = g
            for f in range(len(s.fns)):
                if s.resampled[f]:
                    (self._ingest_file if s.ingest else self._resample_file)(s, f, d, stage)
        if any(any(s.resampled) for s in self.stores):
            torch.cuda.current_stream(device).synchronize()
        return d

    @staticmethod
    def _resample_file(s, f, d, stage):
        """File f of store s -> d[start[f] : start[f] + n_frames[f]] at the model rate: its raw frames go through the staging
        buffer in runs of outputs (each run uploads the frames it reads, nafp_resample_input_range) and one piece per run."""
        from . import resample as rs
        plan = rs.plan_for(s.rate[f], s.fs, d.device)
        ch, n_in, n_total, start = s.channels[f], int(s.n_in[f]), int(s.n_frames[f]), int(s.start[f])
        # outputs per run: their input span (n M / L frames + the filter's two half-widths) fits the staging buffer
        margin = 2 * (plan.half // plan.L + 2)
        room = stage.shape[0] // ch - margin
        if room * plan.L < plan.M:
            raise NotImplementedError(f'{s.fns[f]}: staging buffer too small to resample from {s.rate[f]} Hz')
        step = max(1, min(room * plan.L // plan.M, (1 << 31) - 1))
        with open(s.fns[f], 'rb', buffering=0) as fh:
            for n0 in range(0, n_total, step):
                n1 = min(n_total, n0 + step)
                first, last = rs.input_range(n0, n1, n_in, s.rate[f], s.fs)
                k = (last - first) * ch
                if k:
                    fh.seek(s.data_offset[f] + 2 * ch * first)
                    if fh.readinto(memoryview(stage.numpy()[:k]).cast('B')) != 2 * k:
                        raise IOError(f'{s.fns[f]}: short read')
                raw = stage[:max(k, 1)].to(d.device, non_blocking=False)
                piece = np.array([(0, first, last - first, n_in, n0, start + n0, n1 - n0, ch)], dtype=rs.PIECE_DTYPE)
                plan.run(raw, piece, d)

    @staticmethod
    def _ingest_file(s, f, d, stage):
        """`_resample_file` for NAFP_INGEST_ANY=1: the file's BYTES go through the staging buffer in runs of outputs (each run
        uploads the byte range nafp_ingest_input_range x block_align) and one nafp_ingest_piece per run."""
        from . import ingest as ig
        from . import codecs as cd
        if f in getattr(s, 'flac_index', {}):
            return PcmArena._flac_file(s, f, d, stage)
        plan = ig.plan_for(s.rate[f], s.fs, d.device)
        align, n_in, n_total, start = int(s.block_align[f]), int(s.n_in[f]), int(s.n_frames[f]), int(s.start[f])
        codec = cd.CODECS.get(s.format[f])          # a codec file: whole blocks are uploaded and decoded into a scratch tensor first
        spb = int(s.spb[f]) if codec else 1
        fmt = ig.FORMATS['s16' if codec else s.format[f]][0]
        stage_bytes = stage.numpy().view(np.uint8)
        # outputs per run: their input span (n M / L frames + the filter's two half-widths) fits the staging buffer (a codec
        # file's span is rounded out to whole blocks: two more)
        margin = 2 * (plan.half // plan.L + 2)
        room = (len(stage_bytes) // align - (2 if codec else 0)) * spb - margin
        if room * plan.L < plan.M:
            raise NotImplementedError(f'{s.fns[f]}: staging buffer too small to convert from {s.rate[f]} Hz')
        step = max(1, min(room * plan.L // plan.M, (1 << 31) - 1))
        with open(s.fns[f], 'rb', buffering=0) as fh:
            for n0 in range(0, n_total, step):
                n1 = min(n_total, n0 + step)
                first, last = ig.input_range(n0, n1, n_in, s.rate[f], s.fs)
                if codec:
                    first, last = cd.block_range(first, last, spb)
                k = (last - first) * align
                if k:
                    fh.seek(s.data_offset[f] + align * first)
                    if fh.readinto(memoryview(stage_bytes[:k])) != k:
                        raise IOError(f'{s.fns[f]}: short read')
                raw = stage[:max((k + 1) // 2, 1)].to(d.device, non_blocking=False).view(torch.uint8)
                n_frames = last - first
                if codec:
                    ch = s.channels[f]
                    pcm = torch.empty((max(n_frames * spb * ch, 1),), dtype=torch.int16, device=d.device)
                    cd.decode(raw, np.array([(0, n_frames, 0, codec, ch, align, spb)], dtype=cd.PIECE_DTYPE), pcm)
                    raw, first, n_frames = pcm.view(torch.uint8), first * spb, min(n_frames * spb, n_in - first * spb)
                piece = np.array([(0, first, n_frames, n_in, n0, start + n0, n1 - n0, s.channels[f], fmt, 0)], dtype=ig.PIECE_DTYPE)
                plan.run(raw, piece, d)


    @staticmethod
    def _flac_file(s, f, d, stage):
        """`_ingest_file` for a FLAC file (NAFP_INGEST_FLAC=1): each run uploads the WHOLE FRAMES that cover its input range, decodes
        them into a byte scratch tensor (utils/flac.py) and ingests that as 16- or 24-bit PCM.  Frames that fail their checks are
        zeros; each is counted once, on the device, in s.flac_failed."""
        from . import ingest as ig
        from . import flac as fl
        idx = s.flac_index[f]
        plan = ig.plan_for(s.rate[f], s.fs, d.device)
        n_in, n_total, start, ch = int(s.n_in[f]), int(s.n_frames[f]), int(s.start[f]), int(s.channels[f])
        fmt = ig.FORMATS['s16' if idx.bps <= 16 else 's24'][0]
        stage_bytes = stage.numpy().view(np.uint8)
        # outputs per run: the frames that cover their input span (two more than the span itself) fit the staging buffer at the
        # file's mean bytes per sample, the largest frame counted twice
        margin = 2 * (plan.half // plan.L + 2) + 2 * int(idx.block.max())
        per_sample = max(1., float(idx.n_bytes.sum()) / max(int(idx.start[-1]), 1))
        room = int((len(stage_bytes) - 2 * int(idx.n_bytes.max())) / (2 * per_sample)) - margin
        if room * plan.L < plan.M:
            raise NotImplementedError(f'{s.fns[f]}: staging buffer too small to convert FLAC from {s.rate[f]} Hz')
        step = max(1, min(room * plan.L // plan.M, (1 << 31) - 1))
        counted = 0
        with open(s.fns[f], 'rb', buffering=0) as fh:
            n0 = 0
            while n0 < n_total:
                n1 = min(n_total, n0 + step)
                first, last = ig.input_range(n0, n1, n_in, s.rate[f], s.fs)
                k0, k1 = fl.frame_range(idx, first, last)
                rows, n_raw, n_pcm = fl.records(idx, k0, k1, 0, 0)
                if n_raw > len(stage_bytes):             # denser than the file's mean: halve the run
                    if n1 - n0 <= 1:
                        raise NotImplementedError(f'{s.fns[f]}: staging buffer too small for its FLAC frames')
                    step = max(1, (n1 - n0) // 2)
                    continue
                if n_raw:
                    fh.seek(int(idx.offset[k0]))
                    if fh.readinto(memoryview(stage_bytes[:n_raw])) != n_raw:
                        raise IOError(f'{s.fns[f]}: short read')
                raw = stage[:max((n_raw + 1) // 2, 1)].to(d.device, non_blocking=False).view(torch.uint8)
                pcm = torch.empty((max(n_pcm, 1),), dtype=torch.uint8, device=d.device)
                status = torch.zeros((max(k1 - k0, 1),), dtype=torch.int32, device=d.device)
                fl.decode(raw, rows, pcm, status)
                if s.flac_failed is None:
                    s.flac_failed = torch.zeros((), dtype=torch.int64, device=d.device)
                s.flac_failed += (status[max(counted - k0, 0):k1 - k0] != 0).sum()
                counted = max(counted, k1)
                frame0 = int(idx.start[k0]) if k1 > k0 else 0
                covered = int(idx.start[k1] - idx.start[k0]) if k1 > k0 else 0
                piece = np.array([(0, frame0, max(0, min(covered, n_in - frame0)), n_in, n0, start + n0, n1 - n0, ch, fmt, 0)],
                                 dtype=ig.PIECE_DTYPE)
                plan.run(raw if n_pcm == 0 else pcm, piece, d)
                n0 = n1

    def flac_failed_frames(self):
        """Frames of the stores' FLAC files that failed their checks in `.device()` (one read of the device counters)."""
        return sum(int(s.flac_failed.item()) for s in self.stores if getattr(s, 'flac_failed', None) is not None)


def _randint(rng, low, high, size=None):
    """np.random.randint(low, high) (exclusive high); low >= high -> low (see module docstring)."""
    if high <= low:
        return low if size is None else np.full(size, low, dtype=np.int64)
    return rng.integers(low, high, size=size)


class genUnbalSequence:
    def __init__(self, fns_event_list, bsz=120, n_anchor=60, duration=1, hop=.5, fs=8000, shuffle=False,
                 seg_mode='all', amp_mode='normal', random_offset_anchor=False, offset_margin_hop_rate=0.4,
                 bg_mix_parameter=[False], ir_mix_parameter=[False], speech_mix_parameter=[False], reduce_items_p=0,
                 reduce_batch_first_half=False, experimental_mode=False, drop_the_last_non_full_batch=True,
                 seed=0, device=None, resident=True, shard=(0, 1)):
        if experimental_mode:
            raise NotImplementedError('experimental_mode')
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
        order (dataloader_keras.py:223-311, 316-398).  Vectorised over the batch."""
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
        if self.world > 1:
            # this rank's anchors of the global batch and their replicas (a ragged last batch splits as evenly
            # as its anchors allow)
            a0, a1 = (nA * self.rank) // self.world, (nA * (self.rank + 1)) // self.world
            rows = np.concatenate([rows[a0:a1], rows[nA + a0 * npa:nA + a1 * npa]])
        return rows

    def n_local_anchors(self, idx):
        nA = min(self.n_anchor, self.n_samples - idx * self.n_anchor)
        return (nA * (self.rank + 1)) // self.world - (nA * self.rank) // self.world

    # ---- device ---------------------------------------------------------------------------
    def _resident(self):
        if self._pcm is None:
            self._pcm = self.arena.device(self.device)
            self._lib = _lib.load()
        return self._pcm

    def run(self, rows):
        """(n_rows, 1, T) float32 CUDA batch of a row table."""
        pcm = self._resident()
        d_rows = torch.from_numpy(rows.view(np.uint8).reshape(-1)).to(pcm.device)
        out = torch.empty((len(rows), 1, self.seg_len), dtype=torch.float32, device=pcm.device)
        with torch.cuda.device(pcm.device):
            _lib.check(self._lib.nafp_augment_rows(_lib.ptr(pcm), _lib.ptr(d_rows), len(rows), self.seg_len, _lib.ptr(out),
                                                   _lib.current_stream()), 'augment_rows')
        return out

    def __getitem__(self, idx):
        if idx < 0 or idx >= len(self):
            raise IndexError(idx)
        rows = self.plan(idx)
        nA = self.n_local_anchors(idx)
        if self.reduce_batch_first_half:           # synthesized queries only (dataloader_keras.py:308-309): the anchors are not built
            return self.run(rows[nA:]), []
        out = self.run(rows)
        return out[:nA], out[nA:]
