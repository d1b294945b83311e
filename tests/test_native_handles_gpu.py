"""The native handles (``pg_*``, ``cg_*``, ``cl_*``) over their lives on the MI355X: every device resource of a handle is a member
that frees itself (dl4vc_amd/csrc/device_buffer.h), so what can go wrong is the order in which they go, two handles sharing a
process, and a handle that is used again after a call failed.  Each case repeats a call whose result is known and compares
byte for byte; the shapes are the smallest the fixtures offer (20 locations at window 16 and 8 reads, two regions, two chunks)."""
import numpy as np
import pytest

from dl4vc_amd import hdf5io, pileup_gpu
from dl4vc_amd.candgen import CandidateCounter
from tests.candidates_fixture import load, write_bam
from tests.loader_device_cases import SEED, make_records

pytestmark = pytest.mark.gpu
W, MR = 16, 8


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """The candidate generator's random fixture with and without its index, a FASTA for it and its first 20 candidate sites."""
    d = tmp_path_factory.mktemp("handles")
    fx = load("random")
    bam = write_bam(fx, str(d / "r.bam"))
    bare = write_bam(fx, str(d / "bare.bam"), index=False)
    rng = np.random.default_rng(3)
    fa = str(d / "ref.fa")
    with open(fa, "w") as f:
        for name, length in fx["references"]:
            s = "".join(rng.choice(list("ACGT"), length))
            f.write(">%s\n%s\n" % (name, "\n".join(s[i:i + 60] for i in range(0, length, 60))))
    lines = [run for run in fx["runs"] if run["name"] == "cli"][0]["lines"][:20]
    assert len(lines) == 20
    contigs, pos = [l.split("\t")[0] for l in lines], [int(l.split("\t")[1]) for l in lines]
    regions = [(tid, 0, length) for tid, (_, length) in enumerate(fx["references"])][:2]
    assert len(regions) == 2
    return {"bam": bam, "bare": bare, "fa": fa, "contigs": contigs, "pos": pos, "regions": regions}


def _encoder(inputs, bam="bam"):
    return pileup_gpu.GpuPileupEncoder(inputs[bam], inputs["fa"], W, MR, 10, 50)


def _encode(g, inputs):
    out = g.encode_device(inputs["contigs"], inputs["pos"])
    return b"".join([t.cpu().numpy().tobytes() for t in out[:3]] + [a.tobytes() for a in out[3:]])


@pytest.fixture(scope="module")
def first(inputs):
    """The result every later call is compared with: one encoder, one call."""
    with _encoder(inputs) as g:
        out = g.encode_device(inputs["contigs"], inputs["pos"])
        assert (out[5] == 1).any(), out[5]
        return _encode(g, inputs)


def test_pileup_handle_opened_and_closed_twice(inputs, first):
    for _ in range(2):
        with _encoder(inputs) as g:
            assert _encode(g, inputs) == first


def test_two_pileup_handles_called_alternately(inputs, first):
    with _encoder(inputs) as a, _encoder(inputs) as b:
        b.set_inflate_device(True)
        for _ in range(2):
            assert _encode(a, inputs) == first
            assert _encode(b, inputs) == first


def test_pileup_handle_with_the_device_inflate_on_and_off(inputs, first):
    with _encoder(inputs) as g:
        for on in (True, False, True, False):
            g.set_inflate_device(on)
            assert _encode(g, inputs) == first
            assert (g.stats()["blocks"] > 0) == on


def test_pileup_handle_after_a_refused_call(inputs, first):
    with _encoder(inputs, "bare") as g:
        assert g.lib.pg_set_inflate_device(g._h, 1, 0) == -1
        assert b"needs the BAI index" in g.lib.pg_last_error(g._h)
        assert _encode(g, inputs) == first
        assert g.stats()["blocks"] == 0


def test_two_candidate_handles_interleaved(inputs):
    with CandidateCounter(inputs["bam"]) as a, CandidateCounter(inputs["bam"], inflate_device="gpu") as b:
        got = []
        for _ in range(2):
            for h in (a, b):
                res, stats = h.run(inputs["regions"])
                assert (stats.get("inflate_blocks", 0) > 0) == (h is b)
                got.append(sorted(res))
    assert len(got[0]) > 0 and all(g == got[0] for g in got[1:])


def test_chunk_loader_handle_opened_and_closed_twice(tmp_path):
    from dl4vc_amd.chunk_loader import DeviceChunkLoader
    from dl4vc_amd.loader import NativeLoader
    path = str(tmp_path / "two_chunks.hdf")
    hdf5io.write_candidates(path, make_records(20, 10)[:16])            # two chunks of 8 records
    with NativeLoader(path, 10, batch_sites=16, seed=SEED, threads=1) as nl:
        (want,) = list(nl)
    for _ in range(2):
        with DeviceChunkLoader(path, 10, batch_sites=16, seed=SEED) as dl:
            ((plan, outs),) = list(dl.batches())
            assert dl.stage["chunks"] == 2 and len(plan) == 16
            for t, ref in zip(outs, (want.reads, want.qual, want.strand, want.ref, want.ref_mask, want.var_mask)):
                assert (t.cpu().numpy() == ref).all()
            assert plan.vcfrec == list(want.vcfrec)
