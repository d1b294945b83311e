"""The location round: what every consumer of the GPU pileup encoder does with a round of locations.

The decline ladder is GPU encoder -> ``pe_encode`` for what it declines (status 2) -> the Python builder for what that declines.
``LocationRounds.encode`` runs it with the planes (every location that gives a record has them in its slot of the round's stored
planes), ``LocationRounds.census`` without.  Its consumers: ``inference.score_bam`` and ``census_bam``, the converter
(``pileup_encoder.encode_locations``) and the resident store's fill (``chunk_loader.ResidentRecords.from_bam``).
"""
from __future__ import annotations

import contextlib
import os

import numpy as np

from .hdf5_schema import record_dtype
from .pileup_encoder import EncoderOptions, encode_location, finish_record

ENCODER_COUNTS = ("locations", "gpu", "native", "python", "no_record")


def default_encoder_options() -> EncoderOptions:
    """What call_variants.sh passes to the converter."""
    return EncoderOptions(window_size=100, max_reads=200, max_insert_length=10, max_insert_length_variant=50, min_base_quality=0)


def with_subsample(opt: EncoderOptions, subsample) -> EncoderOptions:
    """``opt`` with ``subsample`` ((fraction, seed), a ``bamio.SampleRule`` or None: ``opt`` as it is) as its read subsampling."""
    if subsample is None:
        return opt
    from dataclasses import replace
    from .bamio import SampleRule
    rule = SampleRule.of(subsample)
    return replace(opt, subsample=(rule.fraction, rule.seed))


def with_read_filter(opt: EncoderOptions, read_filter, read_stats: bool = False) -> EncoderOptions:
    """``opt`` with ``read_filter`` ((exclude, require, min_mapq), a ``bamio.ReadFilter`` or None) and ``read_stats``."""
    if read_filter is None and not read_stats:
        return opt
    from dataclasses import replace
    from .bamio import ReadFilter
    f = ReadFilter.of(read_filter)
    return replace(opt, read_filter=f.as_tuple() if f is not None else None, read_stats=bool(read_stats))


def default_threads() -> int:
    return max(2, min(16, os.cpu_count() or 4))


def declined(status) -> np.ndarray:
    """The indices an encoder hands down the ladder: status 2 (1: a record, 0: none)."""
    return np.flatnonzero(status == 2)


class HostEncoders:
    """What takes a location the GPU encoder declines: ``pe_encode`` (not with ``native=False``), then the Python builder for what
    that declines, in location order.  The Python builder's files are opened on first use, by the thread that calls ``encode``;
    ``close_python`` closes them again, ``close`` everything.  ``cpu``: a stand-in for ``pe_encode``'s handle (tests)."""

    def __init__(self, bam, fasta, opt, threads, native=True, cpu=None):
        from . import loader
        self.bam, self.fasta, self.opt, self.threads = bam, fasta, opt, threads
        self.cpu = cpu if cpu is not None or not native else loader.NativePileupEncoder.from_options(bam, fasta, opt)
        self._py = None

    def python_record(self, loc):
        """The Python builder's record of ``loc``, or None."""
        if self._py is None:
            from .bamio import BamFile, FastaFile, WindowReader
            b = BamFile(self.bam, subsample=getattr(self.opt, "subsample", None), read_filter=getattr(self.opt, "read_filter", None))
            self._py = (b, FastaFile(self.fasta), WindowReader(b))
        b, f, reader = self._py
        res = encode_location(b, f, loc, self.opt, reader)
        dtype = record_dtype(self.opt.max_reads, 2 * self.opt.window_size + 1)
        return finish_record(res, loc, self.opt, dtype) if res is not None else None

    def encode(self, locs, declined, counts=None) -> dict:
        """``declined``: indices into ``locs`` -> {index: (reads, qual, strand, ref, num_reads)} for those that give a record;
        an index that is absent gives none.  ``counts["native"]`` / ``counts["python"]`` count the records of each encoder."""
        host = {}
        if len(declined) == 0:
            return host
        sub = None
        if self.cpu is not None:
            sub = self.cpu.encode([locs[i].contig for i in declined], [locs[i].pos for i in declined], self.threads)
        for k, i in enumerate(declined):
            status = int(sub[5][k]) if sub is not None else 2
            if status == 1:
                host[int(i)] = (sub[0][k], sub[1][k], sub[2][k], sub[3][k], int(sub[4][k]))
                if counts is not None:
                    counts["native"] += 1
            elif status == 2:
                rec = self.python_record(locs[i])
                if rec is not None:
                    host[int(i)] = (rec["single_reads"], rec["q-scores"], rec["strand"], rec["ref_bases"], int(rec["num_reads"]))
                    if counts is not None:
                        counts["python"] += 1
        return host

    def close_python(self):
        if self._py is not None:
            self._py[0].close()
            self._py[1].close()
            self._py = None

    def close(self):
        self.close_python()
        if self.cpu is not None:
            self.cpu.close()


class LocationRounds:
    """Rounds of at most ``round_locations`` locations through the ladder.  ``device`` >= 0: the GPU encoder on that device and
    three stored planes ``[round_locations][max_reads][window]`` in its memory (torch tensors); ``device`` < 0: the CPU definition
    -- every location starts as declined, the stored planes are numpy arrays.  ``stream``: the ``torch.cuda.Stream`` the encoder's
    planes and the slot copies are ordered on (None: the current one).  ``counts`` (``ENCODER_COUNTS``; a dict given is added to)
    and ``stage`` (``pg_stats`` summed over the calls) grow with every call.  ``encoder`` / ``host``: stand-ins for the
    ``GpuPileupEncoder`` and the ``HostEncoders`` (tests); a stand-in encoder writes numpy planes.  ``subsample=(fraction, seed)``:
    ``opt.subsample`` for these rounds -- every encoder of the ladder drops the reads the rule drops (``bamio.SampleRule``)."""

    def __init__(self, bam, fasta, opt, round_locations, device, inflate_device=None, compress_codes="fixed", threads=0, stream=None,
                 counts=None, encoder=None, host=None, subsample=None):
        opt = with_subsample(opt, subsample)
        self.device, self.stream, self.stage = int(device), stream, {}
        self.counts = counts if counts is not None else {}
        for k in ENCODER_COUNTS:
            self.counts.setdefault(k, 0)
        self.window = 2 * opt.window_size + 1
        shape = (int(round_locations), opt.max_reads, self.window)       # (0 slots: a census writes no plane)
        self.enc = self.host = self.torch = None
        if self.device >= 0 and encoder is None:
            import torch
            from .pileup_gpu import GpuPileupEncoder
            self.torch = torch
            self.stored = [torch.empty(shape, dtype=torch.uint8, device=torch.device("cuda", self.device)) for _ in range(3)]
            self.enc = GpuPileupEncoder.from_options(bam, fasta, opt, self.device, inflate_device, compress_codes)
        else:
            if self.device < 0 and inflate_device is not None:
                raise ValueError("inflate_device is the GPU encoder's option: the host filler (device < 0) has none")
            self.stored = [np.zeros(shape, np.uint8) for _ in range(3)]
            self.enc = encoder
        try:
            self.host = host if host is not None else HostEncoders(bam, fasta, opt, threads or default_threads())
        except Exception:
            self.close()
            raise

    def _sum_stats(self):
        for k, v in self.enc.stats().items():
            self.stage[k] = self.stage.get(k, 0) + v

    def last_stats(self) -> dict:
        """``pg_stats`` of the GPU encoder's last call."""
        return self.enc.stats() if self.enc is not None else {}

    def encode(self, locs):
        """One round -> (ref, num_reads, status), host arrays, status in {0, 1}; the planes of every location with status 1 are in
        its slot of ``stored``."""
        n, c = len(locs), self.counts
        if self.enc is not None:
            _r, _q, _s, ref, num, status = self.enc.encode_device([l.contig for l in locs], [l.pos for l in locs], stream=self.stream,
                                                                  out=self.stored)
            self._sum_stats()
            c["gpu"] += int((status == 1).sum())
        else:
            ref, num, status = np.zeros((n, self.window), np.uint8), np.zeros(n, np.int32), np.full(n, 2, np.int8)
        c["locations"] += n
        down = declined(status)
        if len(down):
            host = self.host.encode(locs, down, c)
            status[down] = 0
            torch = self.torch
            with torch.cuda.stream(self.stream) if torch is not None else contextlib.nullcontext():
                for i, (rd, ql, sd, rf, m) in host.items():
                    for plane, src in zip(self.stored, (rd, ql, sd)):
                        src = np.ascontiguousarray(src, np.uint8)
                        if torch is not None:
                            plane[i].copy_(torch.from_numpy(src))
                        else:
                            plane[i] = src
                    ref[i], num[i], status[i] = rf, m, 1
        c["no_record"] += int((status == 0).sum())
        return ref, num, status

    def census(self, locs) -> np.ndarray:
        """One uint8 per location: 1 where ``encode`` would give status 1.  No plane is written, ``counts`` stay."""
        if self.enc is not None:
            status = self.enc.census([l.contig for l in locs], [l.pos for l in locs], stream=self.stream)
            self._sum_stats()
        else:
            status = np.full(len(locs), 2, np.int8)
        flags = (status == 1).astype(np.uint8)
        for i in self.host.encode(locs, declined(status)):
            flags[i] = 1
        return flags

    def close(self):
        if self.host is not None:
            self.host.close()
        if self.enc is not None:
            self.enc.close()


def record_members(locs, keep, ref, num, dtype) -> np.ndarray:
    """The members of a record outside its planes (``dtype``: ``hdf5_schema.blob_dtype``) for the locations ``locs[keep]`` of a round
    that gave ``ref`` and ``num``; ``name`` and ``vcfrec`` cut to the stored widths, as the converter's file cuts them."""
    blob = np.zeros(len(keep), dtype)
    blob["ref_bases"], blob["num_reads"] = ref[keep], num[keep]
    if len(keep):
        blob["name"] = [locs[i].name.encode()[:dtype["name"].itemsize] for i in keep]
        blob["label"] = [locs[i].label for i in keep]
        blob["vcfrec"] = [locs[i].vcf_string.encode()[:dtype["vcfrec"].itemsize] for i in keep]
    return blob
