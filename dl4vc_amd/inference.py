"""Inference harness: HDF5 candidates -> scored VCF records.

Stands where ``trainer.test`` stands in the reference (dl4vc/trainer.py:474-681) for the inference-only
run of ``main.py`` (main.py:213-218): iterate the candidate records in order, assemble batches, call the
model, write ``BP/NV/HV/OV`` into the VCF ID column.  Everything the reference's loop does that does not
reach the VCF (loss logging, ROC/PR prints on the all-'FP' labels, trust-region weighting) is omitted.
"""
from __future__ import annotations

import sys
import time
from typing import Callable, Optional

import numpy as np

from .dataset import assemble_batch
from .hdf5io import CandidateFile
from .location_round import ENCODER_COUNTS, LocationRounds, default_encoder_options, default_threads   # noqa: F401 -- ENCODER_COUNTS is public here
from .shard import shard_range
from .vcf import scored_record, threshold_distance, FormatOptions, PIPELINE_OPTIONS


NEAR_EPS = 1e-4


class _Pipeline:
    """One batch of lookahead over ``net``: batch k+1 is enqueued (``forward_u8_async``: pinned staging, H2D on a copy
    stream) before batch k's scores are awaited and formatted, so the VCF text formatting -- the reference formats each
    score with ``'%.8f' % tensor``, one D2H sync per scalar, utils.py:168-178 -- and the loader hand-off overlap the
    forward.  A model without the asynchronous pair (the CPU test double) is called synchronously."""

    def __init__(self, net, write, use_var_type_threshold, stats=None):
        self.net, self.write, self.vt_thr = net, write, use_var_type_threshold
        self.stats = stats
        self.pending = None
        self.async_ok = hasattr(net, "forward_u8_async")
        self.max_batch = net.handle.query("max_batch") if self.async_ok else 0

    def _emit(self, batch, out):
        vt = out["vt_prob"]
        bp = (1.0 - vt[:, 0]) if self.vt_thr else out["bp"]                   # trainer.py:611-621
        self.write("".join(scored_record(r, b, v) + "\n" for r, b, v in zip(batch.vcfrec, bp, vt)))
        if self.stats is not None:
            # sites whose scores sit within 1e-4 (the score tolerance of the parity gate) of a genotype threshold of the published
            # pipeline (call_variants.sh:154-160): where a call could differ between two correct evaluations
            d = threshold_distance(batch.vcfrec, vt, FormatOptions(**PIPELINE_OPTIONS))
            self.stats["near_threshold"] = self.stats.get("near_threshold", 0) + int((d < NEAR_EPS).sum())
            self.stats["sites"] = self.stats.get("sites", 0) + len(batch.vcfrec)

    def submit(self, batch):
        if self.async_ok and len(batch.vcfrec) <= self.max_batch:
            token = self.net.forward_u8_async(*batch.arrays())
            self.drain()
            self.pending = (batch, token)
        else:
            self.drain()
            self._emit(batch, self.net.forward_u8(*batch.arrays()))

    def drain(self):
        if self.pending is not None:
            batch, token = self.pending
            self.pending = None
            self._emit(batch, self.net.wait(token))


def score_records(net, source: CandidateFile, write: Callable[[str], None], lo: int = 0, hi: Optional[int] = None,
                  sites_per_launch: int = 4096, reads_seed: int = 0, use_var_type_threshold: bool = False,
                  log=None, stats=None) -> int:
    """Score records ``[lo, hi)`` of ``source`` with ``net`` (anything with ``forward_u8`` and ``config``) and hand
    each scored VCF line (with '\\n') to ``write``.  Returns the number of sites scored."""
    cfg = net.config
    hi = len(source) if hi is None else min(hi, len(source))
    done = 0
    t0 = time.perf_counter()
    pipe = _Pipeline(net, write, use_var_type_threshold, stats)
    for b0 in range(lo, hi, sites_per_launch):
        recs = source.read(b0, min(b0 + sites_per_launch, hi))
        # the seed is tied to the ABSOLUTE record index, so shard boundaries never change a site's read subset
        batch = assemble_batch(recs, cfg.reads, seed=reads_seed + b0, use_q=cfg.use_q, use_strand=cfg.use_strand)
        pipe.submit(batch)
        done += len(recs)
        if log:
            dt = time.perf_counter() - t0
            log("  submitted %d/%d sites (%.0f sites/s)" % (done, hi - lo, done / max(dt, 1e-9)))
    pipe.drain()
    return done


def score_file_native(net, hdf_path: str, write: Callable[[str], None], lo: int, hi: int, sites_per_launch: int = 4096,
                      reads_seed: int = 0, use_var_type_threshold: bool = False, log=None,
                      threads: int = 0, stats=None) -> int:
    """Same contract as ``score_records`` but fed by the native batched loader (dl4vc_amd/loader.py): chunk
    inflate and site assembly of batch k+1.. run in C++ threads while the GPU scores batch k."""
    from .loader import NativeLoader
    cfg = net.config
    threads = threads or default_threads()
    done = 0
    t0 = time.perf_counter()
    with NativeLoader(hdf_path, cfg.reads, batch_sites=sites_per_launch, lo=lo, hi=hi, seed=reads_seed,
                      threads=threads) as nl:
        pipe = _Pipeline(net, write, use_var_type_threshold, stats)
        for batch in nl:
            if not cfg.use_q:
                batch.qual[:] = 0
            if not cfg.use_strand:
                batch.strand[:] = 0
            pipe.submit(batch)
            done += len(batch)
            if log:
                dt = time.perf_counter() - t0
                log("  submitted %d/%d sites (%.0f sites/s)" % (done, hi - lo, done / max(dt, 1e-9)))
        pipe.drain()
    return done


def select_sites(hdf_path: str, holdout_chromosomes=(), site_limit: int = 0, block: int = 8192) -> np.ndarray:
    """Record indices the reference's test loader would visit, in its order (ascending: ``shuffle=False``, main.py:94).

    * ``holdout_chromosomes`` (``--test_holdout_chromosomes``): ONLY records whose VCF chromosome -- the text before the
      first tab of ``vcfrec`` -- is in the set are tested (``ContextDatasetFromNumpy.update_holdout_chromosomes`` /
      ``process_location``, dl4vc/dataset.py:382-395,459-478, and ``AdjustableDataSampler(reverse_holdout=True)``,
      dataset.py:706-711, main.py:88-92);
    * ``site_limit``: stop after that many visited sites (``--max-test-batches``: the reference breaks when
      ``batch > max_test_batches``, i.e. after ``(max_test_batches + 1) * test_batch_size`` sites, trainer.py:513-515)."""
    with CandidateFile(hdf_path) as src:
        n = len(src)
        if holdout_chromosomes:
            want = set(str(c).encode() for c in holdout_chromosomes)
            hits = []
            for b0 in range(0, n, block):
                col = src.read_field(b0, b0 + block, "vcfrec")
                chrom = [bytes(v).split(b"\t", 1)[0] for v in col]
                hits.append(b0 + np.flatnonzero(np.fromiter((c in want for c in chrom), bool, len(chrom))))
                if site_limit > 0 and sum(len(h) for h in hits) >= site_limit:
                    break
            idx = np.concatenate(hits) if hits else np.zeros(0, np.int64)
        else:
            idx = np.arange(n, dtype=np.int64)
    if site_limit > 0:
        idx = idx[:site_limit]
    return idx.astype(np.int64)


def select_records(chromosomes, holdout_chromosomes=(), site_limit: int = 0) -> np.ndarray:
    """``select_sites`` for records that are in no file (``chunk_loader.ResidentRecords.chromosomes()``: the text before the first
    tab of each record's ``vcfrec``), by the same rule."""
    if holdout_chromosomes:
        want = set(str(c) for c in holdout_chromosomes)
        idx = np.flatnonzero(np.fromiter((c in want for c in chromosomes), bool, len(chromosomes)))
    else:
        idx = np.arange(len(chromosomes), dtype=np.int64)
    if site_limit > 0:
        idx = idx[:site_limit]
    return idx.astype(np.int64)


def index_runs(idx: np.ndarray):
    """Ascending indices -> maximal runs ``[(lo, hi), ...]`` of consecutive records."""
    if len(idx) == 0:
        return []
    cut = np.flatnonzero(np.diff(idx) != 1) + 1
    starts = np.concatenate(([0], cut))
    ends = np.concatenate((cut, [len(idx)]))
    return [(int(idx[a]), int(idx[b - 1]) + 1) for a, b in zip(starts, ends)]


def run_shard(net, hdf_path: str, out_path: str, shard_index: int = 0, shard_count: int = 1, native: bool = True,
              holdout_chromosomes=(), site_limit: int = 0, loader_device: Optional[str] = None, **kw) -> int:
    """Score this rank's contiguous slice of the selected sites into ``out_path`` (records only, no header).
    ``loader_device="gpu"``: every run goes through ``score_file_device`` (same lines)."""
    from . import loader
    if loader_device not in (None, "gpu"):
        raise ValueError("loader_device: None or 'gpu', not %r" % (loader_device,))
    idx = select_sites(hdf_path, holdout_chromosomes, site_limit)
    lo, hi = shard_range(len(idx), shard_index, shard_count)
    runs = index_runs(idx[lo:hi])
    done = 0
    with open(out_path, "w") as f:
        for a, b in runs:
            if loader_device == "gpu":
                done += score_file_device(net, hdf_path, f.write, a, b, **kw)
            elif native and loader.available():
                done += score_file_native(net, hdf_path, f.write, a, b, **kw)
            else:
                with CandidateFile(hdf_path) as src:
                    done += score_records(net, src, f.write, a, b, **kw)
    return done


# ---- BAM in, scored records out: no candidates.hdf ----------------------------------------------------------------------

class _Stopped(Exception):
    """The consumer of a ``_DeviceBatches`` has gone: the worker thread ends."""


class _Scored:
    """What ``_Pipeline._emit`` reads of a batch."""

    def __init__(self, vcfrec):
        self.vcfrec = vcfrec


def census_bam(bam: str, fasta: str, locations, encoder_options=None, device_id: int = 0, threads: int = 0,
               inflate_device: Optional[str] = None, batch: int = 16384, stage=None, log=None, subsample=None) -> np.ndarray:
    """The record census: one uint8 per location, 1 where ``score_bam`` would get a record from it.  The GPU encoder's status
    rule runs without writing a plane (``pg_census``); what it declines goes through the fallback of ``score_bam``
    (``location_round.LocationRounds.census``).  ``stage`` (a dict) receives ``pg_stats`` summed over the calls.  Needs torch's HIP
    device, as ``score_bam`` does.  ``subsample=(fraction, seed)``: as in ``score_bam``."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("census_bam: torch sees no HIP device")
    locations = list(locations)
    flags = np.zeros(len(locations), np.uint8)
    # (no stored planes: a census writes none)
    rounds = LocationRounds(bam, fasta, encoder_options or default_encoder_options(), 0, device_id, inflate_device=inflate_device,
                            threads=threads, subsample=subsample)
    try:
        with torch.cuda.device(device_id):
            for l0 in range(0, len(locations), batch):
                flags[l0:l0 + batch] = rounds.census(locations[l0:l0 + batch])
                if log:
                    log("  census of %d/%d locations" % (min(l0 + batch, len(locations)), len(locations)))
    finally:
        rounds.close()
        if stage is not None:
            for k, v in rounds.stage.items():
                stage[k] = stage.get(k, 0) + v
    return flags


class _DeviceBatches:
    """The hand-over of ``score_bam`` and ``score_file_device``: a worker thread (``_run``) fills one of two plane sets on a stream
    of its own while ``_score_device_batches`` scores the other; a free and a ready queue carry them back and forth."""

    def __init__(self, torch, dev, B, R, L, thread_name):
        import queue
        import threading
        from .site_assembly import plane_set
        self.torch, self.dev, self.B, self.R, self.L = torch, dev, B, R, L
        self.sets = [{"planes": plane_set(torch, dev, B, R, L), "vt": torch.empty((B, 3), dtype=torch.float32, device=dev),
                      "bp": torch.empty((B,), dtype=torch.float32, device=dev),
                      "h_vt": torch.empty((B, 3), dtype=torch.float32).pin_memory(),
                      "h_bp": torch.empty((B,), dtype=torch.float32).pin_memory(),
                      "done": torch.cuda.Event(), "vcfrec": [], "filled": 0} for _ in range(2)]
        self.stream = torch.cuda.Stream(dev)
        self.free, self.ready = queue.Queue(), queue.Queue(maxsize=1)
        for s in self.sets:
            self.free.put(s)
        self.stop = threading.Event()
        self.thread = threading.Thread(target=self._run, name=thread_name, daemon=True)

    # -- queue plumbing that gives up when the consumer has gone
    def _get_free(self):
        import queue
        while not self.stop.is_set():
            try:
                return self.free.get(timeout=0.2)
            except queue.Empty:
                pass
        raise _Stopped()

    def _put_ready(self, item):
        import queue
        while not self.stop.is_set():
            try:
                return self.ready.put(item, timeout=0.2)
            except queue.Full:
                pass
        raise _Stopped()

    def _run_guarded(self, body):
        """``body()`` on the worker's device, then the end mark; an exception goes to the consumer, which raises it."""
        try:
            with self.torch.cuda.device(self.dev):
                body()
            self._put_ready(None)
        except _Stopped:
            pass
        except BaseException as e:      # noqa: BLE001 -- handed to the consumer, which raises it
            try:
                self._put_ready(e)
            except _Stopped:
                pass

    def close(self):
        self.stop.set()
        if self.thread.is_alive():
            self.thread.join()


class _BamBatches(_DeviceBatches):
    """Worker side of ``score_bam``: a thread that turns ``sites_per_launch`` locations at a time into assembled device
    planes.  Per round: the location round into its stored planes (``location_round.LocationRounds.encode``; the BAM fetch and
    framing run in the encoder's host threads, or on the device with ``inflate_device="gpu"``), rows and masks on the host
    (``site_assembly.plan_sites``), ``pg_assemble_device`` into one of two plane sets.  A forward batch holds exactly
    ``sites_per_launch`` RECORDS, as a batch of the candidate file does, so a round's records may finish one set and start the next.

    Device memory, allocated once: the stored planes 3 * B * S * L bytes and two sets of 3 * B * (R + 1) * L bytes.  At B = 4096,
    S = 200, R = 100, L = 201 that is 494 MB + 2 * 249 MB = 0.99 GB (about 120 KB per site for the stored planes alone)."""

    def __init__(self, cfg, bam, fasta, locations, opt, sites_per_launch, reads_seed, site_limit, device_id, threads, counts,
                 inflate_device=None, first_record=0, census=None):
        import torch
        self.cfg, self.locations, self.seed, self.limit = cfg, locations, reads_seed, site_limit
        self.first_record, self.census = int(first_record), census
        if census is not None and len(census) != len(locations):
            raise ValueError("census: %d flags for %d locations" % (len(census), len(locations)))
        S, L = opt.max_reads, 2 * opt.window_size + 1
        if L != cfg.length:
            raise ValueError("the encoder's window gives %d columns, the model reads %d" % (L, cfg.length))
        if cfg.reads > S:
            raise ValueError("the model reads %d rows per site but the encoder stores only %d" % (cfg.reads, S))
        super().__init__(torch, torch.device("cuda", device_id), int(sites_per_launch), cfg.reads, L, "score_bam-encoder")
        self.S = S
        self.rounds = LocationRounds(bam, fasta, opt, self.B, device_id, inflate_device=inflate_device, threads=threads,
                                     stream=self.stream, counts=counts)
        self.stage = self.rounds.stage                   # pg_stats summed over the encoder's calls

    def _run(self):
        try:
            self._run_guarded(self._rounds)
        finally:
            self.rounds.host.close_python()              # (opened by this thread)

    def _rounds(self):
        from .site_assembly import plan_sites
        enc, stored = self.rounds.enc, self.rounds.stored
        cur = None
        records = 0
        for l0 in range(0, len(self.locations), self.B):
            locs = self.locations[l0:l0 + self.B]
            ref, num, status = self.rounds.encode(locs)
            if self.census is not None:
                self._check_census(l0, locs, status)
            plan = plan_sites(status, num, ref, [l.vcf_string for l in locs], self.R, self.S, self.seed,
                              first_record=self.first_record + records)
            if self.limit > 0:
                plan = plan.slice(0, max(0, self.limit - records))
            records += len(plan)
            off = 0
            while off < len(plan):
                if cur is None:
                    cur = self._get_free()
                    cur["vcfrec"], cur["filled"] = [], 0
                take = min(len(plan) - off, self.B - cur["filled"])
                part, at = plan.slice(off, off + take), cur["filled"]
                outs = [t[at:].data_ptr() for t in cur["planes"]]
                enc.assemble_device([t.data_ptr() for t in stored], len(locs), part, outs, self.cfg.use_q, self.cfg.use_strand,
                                    stream=self.stream.cuda_stream)
                cur["vcfrec"] += part.vcfrec
                cur["filled"] += take
                off += take
                if cur["filled"] == self.B:
                    self.stream.synchronize()
                    self._put_ready(cur)
                    cur = None
            self.stream.synchronize()          # the next round overwrites the stored planes
            if self.limit > 0 and records >= self.limit:
                break
        if cur is not None and cur["filled"]:
            self._put_ready(cur)

    def _check_census(self, l0, locs, status):
        """A location whose status differs from its census flag would shift every later record's seed: an error, never that."""
        flags = np.asarray(self.census[l0:l0 + len(locs)])
        bad = np.flatnonzero((status == 1) != (flags == 1))
        if len(bad):
            i = int(bad[0])
            raise RuntimeError("record census mismatch at location %s (%d of this run): the census says status %d, the encoder %d; "
                               "%d location(s) of this round differ.  The read-subset seeds of the records behind it would be wrong"
                               % (locs[i].name, l0 + i, int(flags[i]), int(status[i]), len(bad)))

    def close(self):
        super().close()
        self.rounds.close()


class _FileBatches(_DeviceBatches):
    """Worker side of ``score_file_device``: the hand-over with a candidate file in front instead of an encoder.  Per batch of
    ``sites_per_launch`` records: the raw chunks covering it are read into pinned memory, inflated on the device and assembled into
    a free plane set (``chunk_loader.DeviceChunkLoader.load``)."""

    def __init__(self, cfg, hdf_path, lo, hi, sites_per_launch, reads_seed, device_id):
        import torch
        from .chunk_loader import DeviceChunkLoader
        self.loader = DeviceChunkLoader(hdf_path, cfg.reads, int(sites_per_launch), seed=reads_seed, device=device_id, use_q=cfg.use_q,
                                        use_strand=cfg.use_strand)
        if self.loader.window != cfg.length:
            self.loader.close()
            raise ValueError("the file's windows have %d columns, the model reads %d" % (self.loader.window, cfg.length))
        self.lo, self.hi = lo, min(hi, len(self.loader))
        super().__init__(torch, torch.device("cuda", device_id), int(sites_per_launch), cfg.reads, self.loader.window, "score_file-loader")

    def _run(self):
        self._run_guarded(self._batches)

    def _batches(self):
        for b0 in range(self.lo, self.hi, self.B):
            cur = self._get_free()
            plan = self.loader.load(b0, min(b0 + self.B, self.hi), [t.data_ptr() for t in cur["planes"]], self.stream.cuda_stream)
            cur["vcfrec"], cur["filled"] = plan.vcfrec, len(plan)
            self.stream.synchronize()
            self._put_ready(cur)

    def close(self):
        super().close()
        self.loader.close()


def score_file_device(net, hdf_path: str, write: Callable[[str], None], lo: int, hi: int, sites_per_launch: int = 4096,
                      reads_seed: int = 0, use_var_type_threshold: bool = False, log=None, stats=None, device_id: int = 0,
                      loader_stats=None) -> int:
    """Same contract and same lines as ``score_file_native``, with the file's chunks inflated and its sites assembled on the
    device (``chunk_loader.DeviceChunkLoader``): the host reads the raw chunks and plans rows and allele masks, nothing else.
    While batch k's forward runs, a worker thread reads, inflates and assembles batch k+1 and batch k-1's text is formatted.
    ``loader_stats`` (a dict) receives the loader's stage times summed over the run.  ``net`` must have been created after
    ``import torch``."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("score_file_device: torch sees no HIP device.  It shares buffers and streams with torch, so torch has to be "
                           "imported before libdl4vc_dan.so / libdl4vc_pileup.so are loaded (one HIP runtime per process)")
    emit = _Pipeline(net, write, use_var_type_threshold, stats)._emit
    src = _FileBatches(net.config, hdf_path, lo, hi, sites_per_launch, reads_seed, device_id)
    done = _score_device_batches(net, src, emit, log, "%d records" % (src.hi - lo))
    if loader_stats is not None:
        for k, v in src.loader.stage.items():
            loader_stats[k] = loader_stats.get(k, 0) + v
    return done


def _score_device_batches(net, src, emit, log, of_what: str) -> int:
    """Consumer side of ``score_bam`` / ``score_file_device``: ``src`` (a ``_BamBatches`` or ``_FileBatches``) hands over sets of
    assembled device planes; each is scored on a stream of its own (``dan_forward_device``) and its scores copied back while the
    worker prepares the next set and the previous set's text is formatted.  Closes ``src``.  -> sites scored."""
    import torch
    fwd = torch.cuda.Stream(src.dev)
    done = 0
    t0 = time.perf_counter()

    def finish(s):
        s["done"].synchronize()
        n = s["filled"]
        emit(_Scored(s["vcfrec"]), {"vt_prob": s["h_vt"][:n].numpy().copy(), "bp": s["h_bp"][:n].numpy().copy()})
        src.free.put(s)

    prev = None
    try:
        src.thread.start()
        while True:
            item = src.ready.get()
            if isinstance(item, BaseException):
                raise item
            if item is None:
                break
            n = item["filled"]
            net.handle.forward_device([t.data_ptr() for t in item["planes"]], n, (0, 0, item["vt"].data_ptr(), item["bp"].data_ptr(), 0),
                                      stream=fwd.cuda_stream)
            with torch.cuda.stream(fwd):
                item["h_vt"][:n].copy_(item["vt"][:n], non_blocking=True)
                item["h_bp"][:n].copy_(item["bp"][:n], non_blocking=True)
                item["done"].record(fwd)
            if prev is not None:
                finish(prev)
            prev = item
            done += n
            if log:
                dt = time.perf_counter() - t0
                log("  submitted %d sites of %s (%.0f sites/s)" % (done, of_what, done / max(dt, 1e-9)))
        if prev is not None:
            finish(prev)
            prev = None
    finally:
        if prev is not None:
            prev["done"].synchronize()
        fwd.synchronize()
        src.close()
    return done


def score_bam(net, bam: str, fasta: str, locations, write: Callable[[str], None], sites_per_launch: int = 4096,
              reads_seed: int = 0, use_var_type_threshold: bool = False, log=None, stats=None, site_limit: int = 0,
              encoder_options=None, device_id: int = 0, threads: int = 0, encoder_counts=None,
              inflate_device: Optional[str] = None, first_record: int = 0, census=None, stage=None, subsample=None) -> int:
    """Score ``locations`` (``pileup_encoder.Location``s, e.g. ``locations_from_vcf(candidates.vcf, label=2)``) straight from
    the BAM: the same lines ``tools/convert_bam_single_reads.py`` + ``score_records`` write, without a candidate file.  The
    pileup planes are encoded (``pg_encode_device``) and assembled (``pg_assemble_device``) in device memory and scored there
    (``dan_forward_device``); only the rows, the allele masks and the scores cross the bus.

    While batch k's forward runs on its own stream, a worker thread encodes and assembles batch k+1, and batch k-1's scores
    are formatted.  Site i draws its read subset with ``reads_seed + i``, i counting the locations that gave a record;
    ``site_limit`` > 0 stops after that many records.  ``encoder_options``: ``pileup_encoder.EncoderOptions`` (default: what
    call_variants.sh passes to the converter).  ``encoder_counts`` (a dict) receives how many locations each encoder took
    (``ENCODER_COUNTS``).  ``inflate_device="gpu"``: the encoder inflates the BAM's BGZF blocks and frames its records on the
    device too (``pg_set_inflate_device``; needs the ``.bai``), same lines; with ``log``, the summary line then gives the
    encoder's stage times (``pg_stats`` summed over its calls).  Device memory: see ``_BamBatches`` -- about 1 GB at 4096 sites per launch.  ``net`` must have been
    created after ``import torch`` (see the error below).  Returns the number of sites scored.

    ``first_record``: the record index of the first record these locations give (a shard of a longer list, planned by
    ``shard.plan_bam_shard`` from the record census): site i then draws with ``reads_seed + first_record + i``.  ``census``: one
    flag per location (``census_bam``); a location whose status differs from its flag raises ``RuntimeError``.  ``stage`` (a
    dict) receives the encoder's stage times.

    ``subsample=(fraction, seed)``: every encoder drops the reads ``bamio.SampleRule`` drops, in front of the pileup (it is
    ``encoder_options.subsample`` for this call): the lines are those of the BAM ``tools/subsample_bam.py`` writes."""
    import torch
    from .location_round import with_subsample
    if not torch.cuda.is_available():
        raise RuntimeError("score_bam: torch sees no HIP device.  It shares buffers and streams with torch, so torch has to be "
                           "imported before libdl4vc_dan.so / libdl4vc_pileup.so are loaded (one HIP runtime per process)")
    emit = _Pipeline(net, write, use_var_type_threshold, stats)._emit
    src = _BamBatches(net.config, bam, fasta, list(locations), with_subsample(encoder_options or default_encoder_options(), subsample),
                      sites_per_launch,
                      reads_seed, site_limit, device_id, threads or default_threads(), encoder_counts, inflate_device, first_record,
                      census)
    done = _score_device_batches(net, src, emit, log, "%d locations" % len(src.locations))
    if stage is not None:
        for k, v in src.stage.items():
            stage[k] = stage.get(k, 0) + v
    if log:
        st = src.stage
        log("  pileup encoder (%s): %s" % ("BGZF inflate and framing on the device" if inflate_device == "gpu" else "host framing",
                                          ", ".join("%s %s" % (k, ("%.1f" % v) if k.endswith("_ms") else int(v)) for k, v in st.items())))
    return done
