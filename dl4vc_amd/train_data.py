"""Training-side batch assembly and example sampling (the training slice of row A2).

Restates what the reference's dataset adds for training on top of the six input planes
(``ContextDatasetFromNumpy._get_generator``, dl4vc/dataset.py:583-680) and its epoch sampler
(``AdjustableDataSampler``, dl4vc/dataset.py:683-749):

* targets per site: ``label`` (the record's field: 0 TP, 1 FN, 2 FP), ``var_type`` / ``is_snp`` / ``var_base_enum`` /
  ``var_ref_enum`` from the VCF line (``utils.parse_vcf``, utils.py:19-72 -- the truth genotype is the optional 11th
  column ``GT:a/b``), ``coverage`` = reads covering the centre column counted from the SELECTED reads when that count is
  positive, else the VCF's DP (dataset.py:603-620), ``allele_freq`` = the candidate's AF (``--aux-keep-candidate-af``, the
  published flag) or the counted variant fraction;
* the example weight ``(is_snp + (1 - is_snp) * non_snp_train_weight)`` (trainer.py:169-172);
* the easy-example sampler: every epoch keeps all examples that are neither "close" (well classified, trainer.py:258-264),
  black-listed nor held out, plus a random ``close_examples_sample_rate`` share of the close ones, in shuffled order.

* the loader workers: ``BatchPrefetcher`` assembles the batches of an epoch ahead of the GPU in ``--num-data-workers``
  processes, each with its own HDF5 handle (the reference: ``DataLoader(num_workers=args.num_data_workers)``, main.py:59-60,
  train_variant_caller.sh:115) -- at 64 sites per 45-ms step one process (≈60 ms per batch of shuffled records) would
  starve the GPU.

* dynamic read down-sampling (``--reads-dynamic-downsample-rate`` / ``-prob``; dataset.py:17-22,256-281,531): ``downsample_rate``
  and ``downsample_prob`` of ``assemble_training_batch`` and of the loaders' ``batches`` -- ``dataset.plan_rows`` on the host,
  ``site_assembly.plan_records`` (the native draw, the flag bit of a plan entry) for the device loaders.  Training batches only.

Not restated (off in the published scripts, rejected by the CLI when requested): read / reference noise augmentation
(dataset.py:24-80,292-336).
"""
from __future__ import annotations

import collections
from dataclasses import dataclass
from typing import Dict, Iterable, Iterator, List, Optional, Sequence

import numpy as np

from .alleles import parse_candidate, count_center_support, center_support_from_counts
from .dataset import assemble_site
from .synth import SiteBatch

TARGET_KEYS = ("label", "var_type", "allele_freq", "coverage", "var_base_enum", "var_ref_enum", "is_snp", "weight")


@dataclass
class TrainBatch:
    sites: SiteBatch
    targets: Dict[str, np.ndarray]
    index: np.ndarray              # absolute record indices (the loop writes close flags back by index, trainer.py:263)
    blacklist: np.ndarray
    names: List[str]
    sampled: Optional[np.ndarray] = None   # (n,) reads dynamic down-sampling kept per site (``sites.num_reads`` where it did not act)

    def planes(self):
        return self.sites.arrays()

    def downsampled(self):
        return downsampled_share(self.sites.num_reads, self.sampled)

    def __len__(self):
        return len(self.index)


def downsampled_share(num_reads, sampled):
    """-> (sites dynamic down-sampling dropped reads of, the sum of their kept fractions ``sampled / num_reads``)."""
    if sampled is None:
        return 0, 0.0
    n, k = np.asarray(num_reads, np.float64), np.asarray(sampled, np.float64)
    hit = k < n
    return int(hit.sum()), float((k[hit] / n[hit]).sum())


def site_targets(record, site, keep_candidate_af: bool = True) -> Dict[str, float]:
    """dataset.py:584-620 for one assembled site."""
    info = parse_candidate(site.vcfrec)
    coverage = info["coverage"]
    allele_freq = info["allele_freq"]
    cover, _agree, variant = count_center_support(np.ascontiguousarray(site.reads.T), site.ref, info["var_mode"])
    if cover > 0:                                               # dataset.py:614-620
        coverage = cover
        if not keep_candidate_af:
            allele_freq = variant / cover
    return {"label": int(np.asarray(record["label"]).reshape(-1)[0]), "var_type": int(info["var_type"]),
            "allele_freq": float(allele_freq), "coverage": float(coverage), "var_base_enum": int(info["var_base"]),
            "var_ref_enum": int(info["ref_base"]), "is_snp": int(bool(info["is_snp"]))}


def site_targets_from_counts(label: int, vcfrec: str, ref, counts, keep_candidate_af: bool = True) -> Dict[str, float]:
    """``site_targets`` of a site whose reads stayed on the device: the record's label and text, its reference row and the
    ``[2][16]`` centre-token counts of its selected rows (``cl_center_counts_device``).  Same arithmetic."""
    info = parse_candidate(vcfrec)
    coverage = info["coverage"]
    allele_freq = info["allele_freq"]
    cover, _agree, variant = center_support_from_counts(counts, ref, info["var_mode"])
    if cover > 0:                                               # dataset.py:614-620
        coverage = cover
        if not keep_candidate_af:
            allele_freq = variant / cover
    return {"label": int(label), "var_type": int(info["var_type"]), "allele_freq": float(allele_freq), "coverage": float(coverage),
            "var_base_enum": int(info["var_base"]), "var_ref_enum": int(info["ref_base"]), "is_snp": int(bool(info["is_snp"]))}


def target_arrays(tgs: Sequence[Dict[str, float]], non_snp_train_weight: float = 1.0, trust_weight=None) -> Dict[str, np.ndarray]:
    """The per-site dicts of ``site_targets`` -> the arrays of a batch, with the example weight (trainer.py:169-172)."""
    t = {"label": np.array([g["label"] for g in tgs], np.uint8), "var_type": np.array([g["var_type"] for g in tgs], np.uint8),
         "allele_freq": np.array([g["allele_freq"] for g in tgs], np.float32),
         "coverage": np.array([g["coverage"] for g in tgs], np.float32),
         "var_base_enum": np.array([g["var_base_enum"] for g in tgs], np.uint8),
         "var_ref_enum": np.array([g["var_ref_enum"] for g in tgs], np.uint8),
         "is_snp": np.array([g["is_snp"] for g in tgs], np.uint8)}
    s = t["is_snp"].astype(np.float32)
    w = s + (1.0 - s) * np.float32(non_snp_train_weight)         # trainer.py:169-172
    if trust_weight is not None:
        w = w * np.asarray(trust_weight, np.float32)
    t["weight"] = w.astype(np.float32)
    return t


def targets_from_counts(plan, label, counts, non_snp_train_weight: float = 1.0, keep_candidate_af: bool = True,
                        trust_weight=None) -> Dict[str, np.ndarray]:
    """The target arrays of the sites of ``plan`` (``site_assembly.SitePlan``) from their labels and centre-token counts."""
    tgs = [site_targets_from_counts(label[i], plan.vcfrec[i], plan.ref[i], counts[i], keep_candidate_af) for i in range(len(plan))]
    return target_arrays(tgs, non_snp_train_weight, trust_weight)


def assemble_training_batch(records, indices: Sequence[int], max_reads: int, seed: Optional[int] = None,
                            non_snp_train_weight: float = 1.0, keep_candidate_af: bool = True, use_q: bool = True,
                            use_strand: bool = True, trust_weight=None, downsample_rate: float = 0.0,
                            downsample_prob: float = 0.0) -> TrainBatch:
    """``records[i]`` is the structured record of absolute index ``indices[i]``.  ``seed`` pins the read subset of deep
    pileups as in ``dataset.assemble_batch`` (RandomState(seed + absolute index)), and with ``downsample_rate`` /
    ``downsample_prob`` the site's dynamic down-sampling (``dataset.plan_rows``)."""
    sites, tgs = [], []
    for rec, idx in zip(records, indices):
        rng = np.random.RandomState(seed + int(idx)) if seed is not None else None
        site = assemble_site(rec, max_reads, rng, use_q=use_q, use_strand=use_strand, downsample_rate=downsample_rate,
                             downsample_prob=downsample_prob)
        sites.append(site)
        tgs.append(site_targets(rec, site, keep_candidate_af))
    stack = lambda f: np.stack([getattr(s, f) for s in sites])   # noqa: E731
    batch = SiteBatch(stack("reads"), stack("qual"), stack("strand"), stack("ref"), stack("ref_mask"), stack("var_mask"),
                      [s.vcfrec for s in sites], np.array([s.num_reads for s in sites], np.int32))
    t = target_arrays(tgs, non_snp_train_weight, trust_weight)
    return TrainBatch(batch, t, np.asarray(indices, np.int64), np.array([s.blacklist for s in sites], bool),
                      [s.name for s in sites], np.array([s.sampled for s in sites], np.int32))


def read_indices(source, indices: np.ndarray) -> np.ndarray:
    """Records at arbitrary (shuffled) indices: sorted, read in runs of consecutive indices, returned in request order."""
    indices = np.asarray(indices, np.int64)
    order = np.argsort(indices, kind="stable")
    srt = indices[order]
    out = np.empty(len(indices), dtype=source.dtype)
    i = 0
    while i < len(srt):
        j = i
        while j + 1 < len(srt) and srt[j + 1] - srt[j] <= 1:
            j += 1
        block = source.read(int(srt[i]), int(srt[j]) + 1)
        out[order[i:j + 1]] = block[srt[i:j + 1] - srt[i]]
        i = j + 1
    return out


# ---- loader workers ---------------------------------------------------------------------------------------------------
_WORKER_SOURCE = None


def _worker_open(path: str) -> None:
    global _WORKER_SOURCE
    from .hdf5io import CandidateFile
    _WORKER_SOURCE = CandidateFile(path)


def _worker_batch(task):
    indices, kwargs = task
    return assemble_training_batch(read_indices(_WORKER_SOURCE, indices), indices, **kwargs)


class BatchPrefetcher:
    """Training batches assembled ahead of the consumer, in order.

    ``workers > 0``: a pool of that many SPAWNED processes (never forked: the parent has a HIP context), each holding its
    own read-only handle on ``path`` (libhdf5 is not thread-safe, so processes, as the reference's DataLoader workers are);
    at most ``depth`` batches are in flight.  ``workers == 0`` (the reference's "set to 0 if HDF problems"): batches are
    assembled in the calling process, one at a time."""

    def __init__(self, path: str, workers: int = 5, depth: Optional[int] = None):
        self.path, self.workers = path, max(0, int(workers))
        self.depth = int(depth) if depth else 2 * max(self.workers, 1)
        self._pool = None
        self._source = None
        if self.workers > 0:
            import multiprocessing as mp
            self._pool = mp.get_context("spawn").Pool(self.workers, initializer=_worker_open, initargs=(path,))
        else:
            from .hdf5io import CandidateFile
            self._source = CandidateFile(path)

    def batches(self, index_lists: Iterable[Sequence[int]], **kwargs) -> Iterator[TrainBatch]:
        """``assemble_training_batch(records[idx], idx, **kwargs)`` for every index list, yielded in the order given."""
        if self._pool is None:
            for idx in index_lists:
                idx = np.asarray(idx, np.int64)
                yield assemble_training_batch(read_indices(self._source, idx), idx, **kwargs)
            return
        pending = collections.deque()
        it = iter(index_lists)
        done = False
        while True:
            while not done and len(pending) < self.depth:
                try:
                    idx = np.asarray(next(it), np.int64)
                except StopIteration:
                    done = True
                    break
                pending.append(self._pool.apply_async(_worker_batch, ((idx, kwargs),)))
            if not pending:
                return
            yield pending.popleft().get()

    def close(self) -> None:
        if self._pool is not None:
            self._pool.terminate()
            self._pool.join()
            self._pool = None
        if self._source is not None:
            self._source.close()
            self._source = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@dataclass
class DeviceTrainBatch:
    """A batch whose six planes lie in device memory (``DeviceBatchPrefetcher``): uint8 torch tensors, views of one of the
    prefetcher's plane sets.  ``event`` was recorded on the loader's stream behind the assembly.  ``release()`` hands the
    plane set back to the loader; call it once the step (``backward_end``) or the forward that read the planes has returned."""
    device_planes: list
    targets: Dict[str, np.ndarray]
    index: np.ndarray
    blacklist: np.ndarray
    vcfrec: List[str]
    event: object
    _release: object = None
    num_reads: Optional[np.ndarray] = None
    sampled: Optional[np.ndarray] = None   # as ``TrainBatch.sampled``

    def planes(self):
        return self.device_planes

    def downsampled(self):
        return downsampled_share(self.num_reads, self.sampled)

    def release(self) -> None:
        rel, self._release = self._release, None
        if rel is not None:
            rel()

    def __len__(self):
        return len(self.index)


class _Stopped(Exception):
    pass


class BatchError(ValueError):
    """The device loader's worker could not make a batch of the records it was asked for (a record with more reads than stored
    rows, allele masks that cannot be built, a damaged chunk): the reason, for the command line to end the run with."""


class DeviceBatchPrefetcher:
    """``BatchPrefetcher``'s ``batches(index_lists, **kwargs)`` with the batches assembled on the GPU
    (``--train-loader-device gpu``): one worker thread with plane sets handed back and forth, the pattern of
    ``inference._FileBatches``.
    The worker reads the raw chunks the indices of the next ``ahead`` index lists fall in and inflates them on the device in one
    launch (``DeviceChunkLoader.inflate_lists``: a megabyte chunk keeps its one decoding lane busy for tens of milliseconds however
    many chunks the launch holds, longer than a training step, so a launch per batch would bound the step rate); then, per list,
    it plans rows and masks on the host, assembles the six planes into a free plane set and counts the centre tokens for the
    targets (``assemble_list``), all on its own stream, while the consumer's steps run, and records the batch's event.  There are
    ``2 * ahead`` plane sets, so that the lists of one launch can be assembled while the consumer still holds those of the one
    before.  The lists of an epoch are known at its start (the sampler's feedback acts at the next epoch), so the worker
    runs ahead as far as the plane sets allow.  A plane set returns to the worker through ``DeviceTrainBatch.release``.

    ``resident=True`` (``--train-cache-device gpu``): the file is inflated once, at construction, into a record store in device
    memory of at most ``cache_bytes`` (``chunk_loader.ResidentRecords``; a file that does not fit, or a damaged chunk, ends the
    construction with the reason) and closed; the worker skips ``inflate_lists`` and ``batches`` skips ``reserve``: a batch is the
    host plan, one gather kernel from the store and the counts (``record_format``: ``chunk_loader.RecordStore``'s, the same batches
    from fewer bytes).  ``stage`` then also holds ``fill_ms``, ``store_bytes`` and
    ``store_records``, and its ``chunks``, ``compressed_bytes`` and ``inflate_ms`` stop growing once the loader is open.

    ``path`` may be a ``chunk_loader.BamSource`` instead (``--train_bam``): the store is then filled from the GPU pileup encoder
    (``ResidentRecords.from_bam``) and no candidate file exists; ``resident=True`` is required (there is no other form), and
    ``cache_bytes`` may be a function, called once the fill's staging planes are allocated.  ``stage`` then holds the encoders'
    counts and ``encode_ms``.

    torch must have been imported before the HIP libraries were loaded (one HIP runtime per process).  Every queue wait ends
    after ``wait_s`` seconds with an error that names what it waited for; an exception of the worker is raised in the consumer."""

    AHEAD = 4        # index lists whose chunks are inflated in one launch; twice as many plane sets

    def __init__(self, path: str, reads: int, batch_sites: int, device: int = 0, use_q: bool = True, use_strand: bool = True,
                 wait_s: float = 600.0, ahead: int = AHEAD, resident: bool = False, cache_bytes: int = 0, slab_bytes: Optional[int] = None,
                 record_format: str = "rows"):
        import torch
        from .chunk_loader import BamSource, DeviceChunkLoader, ResidentRecords, STORE_SLAB_BYTES
        from .site_assembly import plane_set
        source = path if isinstance(path, BamSource) else None
        if source is not None:
            path = source.bam
            if not resident:
                raise ValueError("records encoded from a BAM are kept resident in device memory: there is no non-resident form")
        self.torch, self.path = torch, path
        self.B, self.wait_s = max(1, int(batch_sites)), float(wait_s)
        self.ahead = max(1, int(ahead))
        self.resident = bool(resident)
        self.dev = torch.device("cuda", device)
        if self.resident:
            # ``--train-cache-device gpu``: the whole file is inflated once, here, into a record store of at most ``cache_bytes``
            # (``chunk_loader.ResidentRecords``); every batch of every ``batches`` call is assembled from it
            with torch.cuda.device(self.dev):
                self.loader = ResidentRecords(source or path, reads, self.B, device=device, use_q=use_q, use_strand=use_strand,
                                              capacity_bytes=cache_bytes, slab_bytes=slab_bytes or STORE_SLAB_BYTES,
                                              record_format=record_format)
        else:
            # the record buffer starts at one chunk and is sized by ``batches`` for the lists it is given: a shuffled epoch needs up
            # to ``ahead * batch_sites`` chunks (1 MB each in the production layout), a sequential evaluation pass an eighth of that
            self.loader = DeviceChunkLoader(path, reads, self.B, device=device, use_q=use_q, use_strand=use_strand, shuffled=self.ahead,
                                            chunks=1)
        R, L = self.loader.reads, self.loader.window
        self.sets = [plane_set(torch, self.dev, self.B, R, L) for _ in range(2 * self.ahead)]
        self.stream = torch.cuda.Stream(self.dev)

    @property
    def stage(self):
        return self.loader.stage

    def __len__(self):
        return len(self.loader)

    def _wait(self, q, what: str, stop, put=None, alive=None):
        """``q.get()`` (or ``q.put(put)``) in short waits: gives up when ``stop`` is set, when ``alive`` says the other side has
        gone, and after ``wait_s`` seconds -- naming ``what``."""
        import queue
        import time
        deadline = time.monotonic() + self.wait_s
        while not stop.is_set():
            try:
                return q.get(timeout=0.2) if put is None else q.put(put[0], timeout=0.2)
            except (queue.Empty, queue.Full):
                pass
            if alive is not None and not alive() and (put is not None or q.empty()):
                raise RuntimeError("the device loader's worker thread ended while the consumer waited for %s" % what)
            if time.monotonic() > deadline:
                raise TimeoutError("the device loader of %s waited %.0f s for %s" % (self.path, self.wait_s, what))
        raise _Stopped()

    def _work(self, lists, kwargs, free, ready, stop):
        try:
            with self.torch.cuda.device(self.dev):
                for k, idx in enumerate(lists):
                    if k % self.ahead == 0 and not self.resident:    # the chunks of the next few batches, inflated in one launch
                        self.loader.inflate_lists(lists[k:k + self.ahead], self.stream.cuda_stream)
                    planes = self._wait(free, "a free plane set for batch %d (the step that read it has not released it)" % k, stop)
                    got = self.loader.assemble_list(idx, kwargs["seed"], [t.data_ptr() for t in planes], self.stream.cuda_stream,
                                                    downsample_rate=kwargs.get("downsample_rate", 0.0),
                                                    downsample_prob=kwargs.get("downsample_prob", 0.0))
                    targets = targets_from_counts(got.plan, got.label, got.counts, kwargs.get("non_snp_train_weight", 1.0),
                                                  kwargs.get("keep_candidate_af", True), kwargs.get("trust_weight"))
                    event = self.torch.cuda.Event()
                    event.record(self.stream)
                    batch = DeviceTrainBatch([t[:len(idx)] for t in planes], targets, idx, np.array(got.plan.blacklist, bool),
                                             list(got.plan.vcfrec), event, lambda planes=planes: free.put(planes),
                                             got.plan.num_reads, got.plan.sampled)
                    self._wait(ready, "the consumer to take batch %d" % k, stop, put=(batch,))
                self._wait(ready, "the consumer to take the end of the batches", stop, put=(None,))
        except _Stopped:
            pass
        except BaseException as e:      # noqa: BLE001 -- handed to the consumer, which raises it
            try:
                self._wait(ready, "the consumer to take the worker's error", stop, put=(e,))
            except (_Stopped, TimeoutError):
                pass

    def batches(self, index_lists: Iterable[Sequence[int]], **kwargs) -> Iterator[DeviceTrainBatch]:
        """A ``DeviceTrainBatch`` per index list, in the order given; ``kwargs`` as ``assemble_training_batch`` takes them
        (``seed`` is required: it pins the read subsets of deep pileups)."""
        import queue
        import threading
        if kwargs.get("seed") is None:
            raise ValueError("the device loader needs the seed of the read subsets")
        want = (self.loader.reads, bool(self.loader.use_q), bool(self.loader.use_strand))
        have = (kwargs.get("max_reads", want[0]), bool(kwargs.get("use_q", True)), bool(kwargs.get("use_strand", True)))
        if have != want:
            raise ValueError("the loader was opened for (reads, use_q, use_strand) = %s, the batches ask for %s" % (want, have))
        lists = [np.asarray(idx, np.int64) for idx in index_lists]
        if not self.resident:
            self.loader.reserve(max([self.loader.chunks_of(lists[k:k + self.ahead]) for k in range(0, len(lists), self.ahead)] or [0]))
        free, ready, stop = queue.Queue(), queue.Queue(), threading.Event()     # (the plane sets bound what is ready)
        for planes in self.sets:
            free.put(planes)
        worker = threading.Thread(target=self._work, args=(lists, kwargs, free, ready, stop), name="train-loader-device", daemon=True)
        worker.start()
        held = []                                        # batches handed out and (perhaps) not yet released, oldest first
        try:
            for k in range(len(lists) + 1):
                # the consumer asks for batch k after it began the step of batch k - 1, so the step of batch k - 2 has ended:
                # a batch the consumer did not release itself goes back now
                while len(held) > 1:
                    held.pop(0).release()
                item = self._wait(ready, "batch %d of %d" % (k, len(lists)), stop, alive=worker.is_alive)
                if isinstance(item, ValueError) and not isinstance(item, BatchError):
                    raise BatchError(str(item)) from item         # (a record the loader refuses, a damaged chunk)
                if isinstance(item, BaseException):
                    raise item
                if item is None:
                    return
                held.append(item)
                yield item
        finally:
            stop.set()
            worker.join(self.wait_s)
            if worker.is_alive():
                raise TimeoutError("the device loader's worker thread did not end within %.0f s" % self.wait_s)
            self.stream.synchronize()

    def close(self) -> None:
        if self.loader is not None:
            self.loader.close()
            self.loader = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class EasyExampleSampler:
    """``AdjustableDataSampler`` (dl4vc/dataset.py:683-749, built at main.py:72-74 when ``close_examples_sample_rate < 1``).

    Holds the per-example tables the training loop updates (``close``: trainer.py:263-264 via ``update_close_example``;
    ``blacklist``: trainer.py:267) and yields one epoch's index order.  ``rng`` is a ``np.random.RandomState``: the reference
    draws from numpy's global legacy generator, so ``RandomState(s)`` here reproduces ``np.random.seed(s)`` there draw for
    draw (one ``permutation`` of the close indices, one ``permutation`` of the merged list)."""

    def __init__(self, n_examples: int, close_keep: float = 0.15, holdout: Optional[np.ndarray] = None,
                 reverse_holdout: bool = False, shuffle: bool = True, rng: Optional[np.random.RandomState] = None,
                 plain: bool = False):
        # plain: main.py:75-77 -- with --close_examples_sample_rate >= 1 the reference builds NO sampler: a plain
        # DataLoader(shuffle=True) over the whole dataset, which filters nothing (not the close examples, not the blacklist
        # and -- a quirk kept, with a warning from main.py -- not the held-out chromosomes either)
        self.plain = bool(plain)
        self.n = int(n_examples)
        self.close_keep = float(close_keep)
        self.close = np.zeros(self.n, bool)
        self.blacklist = np.zeros(self.n, bool)
        self.holdout = np.zeros(self.n, bool) if holdout is None else np.asarray(holdout, bool)
        self.reverse_holdout, self.shuffle = reverse_holdout, shuffle
        self.rng = rng if rng is not None else np.random.RandomState()
        self.epochs = 0
        self.epoch_len = self.n

    def update_close(self, indices, flags) -> None:               # trainer.py:25-40
        self.close[np.asarray(indices, np.int64)] = np.asarray(flags, bool)

    def update_blacklist(self, indices, flags) -> None:           # trainer.py:52-59: only ever sets
        idx = np.asarray(indices, np.int64)[np.asarray(flags, bool)]
        self.blacklist[idx] = True

    def epoch(self) -> np.ndarray:
        self.epochs += 1
        if self.plain:
            self.epoch_len = self.n
            return self.rng.permutation(self.n).astype(np.int64)
        if self.reverse_holdout:                                  # dataset.py:706-711: evaluation on the held-out chromosomes only
            order = np.nonzero(~self.close & ~self.blacklist & self.holdout)[0]
        else:
            keep = np.nonzero(~self.close & ~self.blacklist & ~self.holdout)[0]
            n_close = int(self.close.sum())
            n_take = int(self.close_keep * n_close)               # dataset.py:720
            # dataset.py:727-729, quirk included: with no close example `[-0:]` is the WHOLE index array, so the reference
            # permutes all n indices (and keeps none) -- the draw is reproduced so the next shuffle sees the same state
            close_idx = np.argsort(self.close)[-n_close:]
            take = self.rng.permutation(close_idx)[:n_take]
            order = np.concatenate((keep, take)).astype(np.int64)
        self.epoch_len = len(order)
        if self.shuffle:
            return self.rng.permutation(order)                    # dataset.py:744
        return order

    def __len__(self):
        return self.epoch_len
