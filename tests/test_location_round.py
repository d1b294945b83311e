"""The location round (dl4vc_amd/location_round.py) without a GPU: ``LocationRounds(device=-1)`` on the labelled BAM fixture against
``encode_locations(native=True)``, ``record_members`` against the members that wrote, and the ladder on scripted stand-ins for all
three encoders."""
import numpy as np
import pytest

from dl4vc_amd import pileup_encoder as PE
from dl4vc_amd.hdf5_schema import PLANE_FIELDS, blob_dtype, record_dtype
from dl4vc_amd.location_round import ENCODER_COUNTS, HostEncoders, LocationRounds, default_encoder_options, record_members
from tests import train_bam_cases as TC

FILL = 0xAB


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    f = TC.labelled_fixture(tmp_path_factory.mktemp("location_round"))
    f["locs"] = TC.locations(f, "train")
    # the reference, once: the converter's records of the same list, and which location each came from
    f["recs"], f["errors"] = PE.encode_locations(f["bam"], f["fasta"], f["locs"], default_encoder_options(), native=True, threads=2)
    names = [bytes(v).decode() for v in f["recs"]["name"]]
    assert len(set(l.name for l in f["locs"])) == len(f["locs"]) and all(len(l.name) <= 16 for l in f["locs"])
    f["status"] = np.array([l.name in names for l in f["locs"]], np.int8)
    assert names == [l.name for l, s in zip(f["locs"], f["status"]) if s]
    return f


def all_rounds(fx, B):
    """Every training location through ``LocationRounds(device=-1)`` in rounds of B -> (ref, num, status, the slot planes of every
    location, counts)."""
    locs = fx["locs"]
    rounds = LocationRounds(fx["bam"], fx["fasta"], default_encoder_options(), B, -1, threads=2)
    try:
        for p in rounds.stored:
            assert isinstance(p, np.ndarray) and p.shape == (B, 200, 201)
        out = []
        for l0 in range(0, len(locs), B):
            part = locs[l0:l0 + B]
            ref, num, status = rounds.encode(part)
            out.append((ref, num, status, [p[:len(part)].copy() for p in rounds.stored]))
        assert rounds.enc is None and rounds.last_stats() == {} and rounds.stage == {}
        return (np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out]),
                [np.concatenate([o[3][k] for o in out]) for k in range(3)], dict(rounds.counts))
    finally:
        rounds.close()


@pytest.mark.parametrize("B", [16, 43])
def test_the_host_rounds_equal_encode_locations_location_by_location(fx, B):
    locs, recs = fx["locs"], fx["recs"]
    assert len(locs) == 43 and len(recs) == TC.TRAIN_RECORDS and fx["errors"] == 3
    ref, num, status, planes, counts = all_rounds(fx, B)
    assert status.dtype == np.int8 and status.tolist() == fx["status"].tolist()
    k = 0
    for i in range(len(locs)):
        if status[i]:
            assert ref[i].tobytes() == recs["ref_bases"][k].tobytes() and int(num[i]) == int(recs["num_reads"][k]), locs[i].name
            for plane, name in zip(planes, PLANE_FIELDS):
                assert plane[i].tobytes() == recs[name][k].tobytes(), (locs[i].name, name)
            k += 1
    assert k == len(recs)
    assert set(counts) == set(ENCODER_COUNTS)
    assert counts["locations"] == 43 == counts["native"] + counts["python"] + counts["no_record"]
    assert counts["python"] >= 1 and counts["no_record"] >= 3 and counts["gpu"] == 0


def test_census_of_the_host_rounds_equals_the_statuses(fx):
    rounds = LocationRounds(fx["bam"], fx["fasta"], default_encoder_options(), 0, -1, threads=2)
    try:
        flags = np.concatenate([rounds.census(fx["locs"][l0:l0 + 16]) for l0 in range(0, 43, 16)])
        assert flags.dtype == np.uint8 and flags.tolist() == fx["status"].tolist()
        assert all(v == 0 for v in rounds.counts.values())
    finally:
        rounds.close()
    with pytest.raises(ValueError, match="inflate_device is the GPU encoder's option"):
        LocationRounds(fx["bam"], fx["fasta"], default_encoder_options(), 16, -1, inflate_device="gpu")


def test_record_members_are_the_members_encode_locations_wrote(fx):
    locs, recs = fx["locs"], fx["recs"]
    ref, num, status, _planes, _counts = all_rounds(fx, 43)
    keep = np.flatnonzero(status == 1)
    bdt = blob_dtype(201)
    blob = record_members(locs, keep, ref, num, bdt)
    assert blob.dtype == bdt and len(blob) == len(recs)
    assert set(bdt.names) | set(PLANE_FIELDS) == set(recs.dtype.names)
    for name in bdt.names:
        assert blob[name].tobytes() == np.ascontiguousarray(recs[name]).tobytes(), name
    # the one text longer than the 128 stored bytes is cut, not dropped
    long = [k for k, i in enumerate(keep) if len(locs[i].vcf_string) > 128]
    assert len(long) == 1 and bytes(blob["vcfrec"][long[0]]) == locs[keep[long[0]]].vcf_string.encode()[:128]
    assert len(record_members(locs, keep[:0], ref, num, bdt)) == 0


# ---- the ladder on scripted encoders -------------------------------------------------------------------------------------------
OPT = PE.EncoderOptions(window_size=3, max_reads=4)
S, W = 4, 7
GPU_STATUS = [1, 2, 0, 2, 2, 1, 2, 0]
NATIVE_STATUS = [1, 2, 2, 0]             # of the four the GPU declines: 1, 3, 4, 6
FINAL = [1, 1, 0, 1, 0, 1, 0, 0]


class StubGpu:
    """A plain object with the GPU encoder's four calls; its "device" planes are numpy arrays."""

    def __init__(self):
        self.calls, self.closed = [], False

    def encode_device(self, contigs, positions, stream=None, out=None):
        self.calls.append("encode_device")
        n, status = len(positions), np.array(GPU_STATUS, np.int8)
        ref, num = np.zeros((n, W), np.uint8), np.zeros(n, np.int32)
        for i in np.flatnonzero(status == 1):
            for k, p in enumerate(out):
                p[i] = 10 * (k + 1) + i
            ref[i], num[i] = 100 + i, i + 1
        return out[0][:n], out[1][:n], out[2][:n], ref, num, status

    def census(self, contigs, positions, stream=None):
        self.calls.append("census")
        return np.array(GPU_STATUS, np.int8)

    def stats(self):
        return {"encode_ms": 1.5, "runs": 2}

    def close(self):
        self.closed = True


class StubNative:
    def __init__(self):
        self.asked, self.closed = [], False

    def encode(self, contigs, positions, threads=1):
        self.asked.append(list(positions))
        n = len(positions)
        planes = [np.full((n, S, W), 40 + k, np.uint8) for k in range(3)]
        return (*planes, np.full((n, W), 50, np.uint8), np.full(n, 3, np.int32), np.array(NATIVE_STATUS, np.int8))

    def close(self):
        self.closed = True


class StubHost(HostEncoders):
    """``pe_encode`` scripted, and a Python rung that has a record for position 3 and none for position 4."""

    def __init__(self):
        super().__init__(None, None, OPT, 1, cpu=StubNative())
        self.python_asked = []

    def python_record(self, loc):
        self.python_asked.append(loc.pos)
        if loc.pos != 3:
            return None
        rec = np.zeros((), record_dtype(S, W))
        rec["single_reads"], rec["q-scores"], rec["strand"], rec["ref_bases"], rec["num_reads"] = 60, 61, 62, 63, 2
        return rec


def scripted():
    gpu, host = StubGpu(), StubHost()
    rounds = LocationRounds(None, None, OPT, 8, 0, encoder=gpu, host=host)
    for p in rounds.stored:
        assert isinstance(p, np.ndarray) and p.shape == (8, S, W)
        p[:] = FILL
    return rounds, gpu, host, [PE.Location("c", i, "c:%d" % i, 2, "c\t%d" % i) for i in range(8)]


def test_the_ladder_on_scripted_encoders():
    rounds, gpu, host, locs = scripted()
    ref, num, status = rounds.encode(locs)
    assert status.tolist() == FINAL
    assert host.cpu.asked == [[1, 3, 4, 6]] and host.python_asked == [3, 4]          # each rung gets what the one above declines, in order
    reads, qual, strand = rounds.stored
    for i in (0, 5):                                      # taken by the GPU encoder: as it wrote them
        assert (reads[i] == 10 + i).all() and (qual[i] == 20 + i).all() and (strand[i] == 30 + i).all()
        assert (ref[i] == 100 + i).all() and num[i] == i + 1
    assert (reads[1] == 40).all() and (qual[1] == 41).all() and (strand[1] == 42).all() and (ref[1] == 50).all() and num[1] == 3
    assert (reads[3] == 60).all() and (qual[3] == 61).all() and (strand[3] == 62).all() and (ref[3] == 63).all() and num[3] == 2
    for i in (2, 4, 6, 7):                                # no record: no plane written
        assert all((p[i] == FILL).all() for p in rounds.stored)
    assert rounds.counts == {"locations": 8, "gpu": 2, "native": 1, "python": 1, "no_record": 4}
    assert rounds.stage == {"encode_ms": 1.5, "runs": 2} and rounds.last_stats() == gpu.stats()
    rounds.encode(locs)
    assert rounds.stage == {"encode_ms": 3.0, "runs": 4} and rounds.counts["locations"] == 16
    rounds.close()
    assert gpu.closed and host.cpu.closed


def test_the_census_of_the_scripted_encoders_equals_the_final_status_and_writes_no_plane():
    rounds, gpu, host, locs = scripted()
    flags = rounds.census(locs)
    assert flags.dtype == np.uint8 and flags.tolist() == FINAL
    assert gpu.calls == ["census"] and host.cpu.asked == [[1, 3, 4, 6]] and host.python_asked == [3, 4]
    assert all((p == FILL).all() for p in rounds.stored)
    assert all(v == 0 for v in rounds.counts.values()) and rounds.stage == {"encode_ms": 1.5, "runs": 2}
    rounds.close()
