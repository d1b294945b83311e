"""The hand-built grid of tests/pileup_cases.py through the two CPU pileup encoders: ``pe_encode`` (libdl4vc_loader.so) gives
every location the status its case states, and wherever the Python builder (``encode_locations(native=False)``) returns, the
two agree byte for byte and in their error counts; where it raises, the type is the one the case names and
``native=True`` (which hands a status 2 to the Python builder) raises it too.  CPU only.

``pe_encode`` runs in a child process with a time limit: a read with a zero-length alignment (``0M 5I``, ``5S 0D``) inside the
window once took it down with SIGSEGV (the image builder read ``quals[0]`` of an empty span), and a crash must show as an
exit status of that child, not end the test run.  Such a read, and one whose SEQ is shorter than its CIGAR's query length
(SEQ ``*``), is declined (status 2) by ``pe_encode`` and a named ``ValueError`` in the Python builder."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dl4vc_amd import loader
from dl4vc_amd import pileup_encoder as PE
from tests import pileup_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not loader.available(), reason="libdl4vc_loader.so not built")
FIELDS = ("single_reads", "q-scores", "strand", "ref_bases", "num_reads")
ERRORS = {"KeyError": KeyError, "ValueError": ValueError}

CHILD = """import sys
sys.path.insert(0, %r)
import numpy as np
from dl4vc_amd import loader
with loader.NativePileupEncoder(%r, %r, *%r) as e:
    out = e.encode(%r, %r, 1)
np.savez(%r, *out)
print('OK')
"""


def pe_encode_in_child(tmp, bam, fa, options, contigs, pos):
    """``NativePileupEncoder.encode`` in its own interpreter -> the six arrays."""
    out = os.path.join(str(tmp), "pe_%d.npz" % len(os.listdir(str(tmp))))
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, bam, fa, tuple(options), list(contigs), [int(p) for p in pos], out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "pe_encode's process ended with status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    z = np.load(out)
    return [z["arr_%d" % k] for k in range(6)]


def _location(l):
    return PE.Location(l.contig, l.pos, "%s:%d" % (l.contig, l.pos), 2, "%s\t%d\t.\tA\tC" % (l.contig, l.pos))


def _options(case):
    return PE.EncoderOptions(window_size=case.w, max_reads=case.max_reads, max_insert_length=case.mil,
                             max_insert_length_variant=case.milv, min_base_quality=case.mbq)


@pytest.mark.parametrize("name", PC.CASE_NAMES)
def test_case_on_the_cpu_encoders(tmp_path, name):
    case = PC.get_case(name)
    bam, fa = PC.write_case(tmp_path, case)
    opt = _options(case)
    contigs, pos = [l.contig for l in case.locs], [l.pos for l in case.locs]
    want = pe_encode_in_child(tmp_path, bam, fa, case.options(), contigs, pos)
    stated = [l.cpu for l in case.locs]
    assert want[5].tolist() == stated, [(l.pos, l.note, int(s)) for l, s in zip(case.locs, want[5]) if s != l.cpu]
    for i, l in enumerate(case.locs):
        one = [_location(l)]
        if l.py:
            assert l.cpu == 2
            for native in (False, True):
                with pytest.raises(ERRORS[l.py]) as info:
                    PE.encode_locations(bam, fa, one, opt, native=native)
                assert type(info.value) is ERRORS[l.py], (l.note, info.value)
                if l.py == "ValueError":
                    assert "read '" in str(info.value), info.value          # the read is named
            continue
        py, e_py = PE.encode_locations(bam, fa, one, opt, native=False)
        nat, e_nat = PE.encode_locations(bam, fa, one, opt, native=True)
        assert e_py == e_nat and py.tobytes() == nat.tobytes(), (l.pos, l.note)
        if l.cpu == 0:
            assert e_py == 1 and len(py) == 0, (l.pos, l.note)
        elif l.cpu == 1:
            assert e_py == 0 and len(py) == 1, (l.pos, l.note)
            for k, f in enumerate(FIELDS):
                assert np.array_equal(py[0][f], want[k][i]), (l.pos, l.note, f)
            assert 1 <= int(want[4][i]) <= case.max_reads
        else:
            assert len(py) + e_py == 1
    if not any(l.py for l in case.locs):              # the whole list in one call (the window reader moves along)
        py, e_py = PE.encode_locations(bam, fa, [_location(l) for l in case.locs], opt, native=False)
        nat, e_nat = PE.encode_locations(bam, fa, [_location(l) for l in case.locs], opt, native=True, threads=2)
        assert e_py == e_nat and py.tobytes() == nat.tobytes()
        assert e_py == stated.count(0) or 2 in stated


def test_every_bullet_of_the_grid_has_a_location():
    """The grid states what it covers: the depths either side of the GPU's track limit, every decline reason, both windows."""
    notes = {}
    for name in PC.CASE_NAMES:
        case = PC.get_case(name)
        pile = PC.Pileup.of_case(case)
        for l in case.locs:
            why = PC.expected_decline(pile, l.contig, l.pos, case.w, case.mbq)
            notes.setdefault(name, []).append((l, why))
            if l.gpu_declines:
                assert why, (name, l)
            if l.must_encode():
                assert not why, (name, l, why)
    seen = set().union(*[why for v in notes.values() for _, why in v])
    assert seen >= {"window", "min_base_quality", "contig_not_in_fasta", "unsorted", "zero_length_alignment", "too_many_tracks",
                    "reference_skip", "eq_base", "short_seq", "duplicate_key", "unknown_reference_base"}
    alone = [why for name in ("declines", "zero_length", "seq_star") for l, why in notes[name] if l.gpu_declines]
    assert all(len(why) == 1 for why in alone), alone                        # each reason alone
    assert [l.gpu_declines for l, _ in notes["depth"]] == [n > 1024 for n in PC.DEPTHS]
