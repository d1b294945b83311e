"""The location round on the GPU: ``LocationRounds(device=0)`` over the labelled BAM fixture against its CPU definition
(``device=-1``, tests/test_location_round.py holds that to ``encode_locations``), byte for byte."""
import numpy as np
import pytest

from dl4vc_amd.location_round import LocationRounds, default_encoder_options
from tests import train_bam_cases as TC

pytestmark = pytest.mark.gpu
B = 16          # the smallest round that splits the 43 locations and still holds a declined and an accepted one in one round


def all_rounds(fx, locs, device, inflate_device=None):
    """-> per round (ref, num, status, the slot planes copied back, the census flags)."""
    rounds = LocationRounds(fx["bam"], fx["fasta"], default_encoder_options(), B, device, inflate_device=inflate_device, threads=2)
    try:
        out = []
        for l0 in range(0, len(locs), B):
            part = locs[l0:l0 + B]
            ref, num, status = rounds.encode(part)
            # (the encoder's planes and the slot copies are ordered on the current stream, and so is the copy back)
            planes = [p[:len(part)].cpu().numpy() if device >= 0 else p[:len(part)].copy() for p in rounds.stored]
            out.append((ref.copy(), num.copy(), status.copy(), planes, rounds.census(part)))
        return out, dict(rounds.counts), dict(rounds.stage)
    finally:
        rounds.close()


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    f = TC.labelled_fixture(tmp_path_factory.mktemp("location_round_gpu"))
    f["locs"] = TC.locations(f, "train")
    f["host"] = all_rounds(f, f["locs"], -1)
    return f


@pytest.mark.parametrize("inflate_device", [None, "gpu"])
def test_the_device_rounds_equal_the_host_rounds(fx, inflate_device):
    locs = fx["locs"]
    want, host_counts, _ = fx["host"]
    got, counts, stage = all_rounds(fx, locs, 0, inflate_device)
    assert len(got) == len(want) == 3
    for r, ((ref, num, status, planes, flags), (wref, wnum, wstatus, wplanes, wflags)) in enumerate(zip(got, want)):
        assert status.tolist() == wstatus.tolist() and flags.tolist() == status.tolist() == wflags.tolist(), r
        keep = status == 1
        assert ref[keep].tobytes() == wref[keep].tobytes() and num[keep].tolist() == wnum[keep].tolist(), r
        for k in range(3):
            assert planes[k][keep].tobytes() == wplanes[k][keep].tobytes(), (r, k)
    # the counts add up; the twin pair is the Python builder's on every path, and the same three locations give no record
    assert counts["locations"] == 43 == counts["gpu"] + counts["native"] + counts["python"] + counts["no_record"]
    assert counts["gpu"] >= 1 and counts["python"] >= 1 and counts["no_record"] == host_counts["no_record"] == 3
    assert stage and all(v >= 0 for v in stage.values())
