"""libdl4vc_pileup.so (include/dl4vc_pileup_gpu.h) without a GPU: the header, the library's exports and
``dl4vc_amd.pileup_gpu`` agree, the option struct mirrors ``pe_options``, and ``encode_locations`` refuses an unknown device."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from dl4vc_amd import loader, pileup_gpu
from dl4vc_amd import pileup_encoder as PE

HEADER = os.path.join(ROOT, "include", "dl4vc_pileup_gpu.h")


def _text(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


@pytest.fixture(scope="module")
def lib():
    if not pileup_gpu.available():
        import __graft_entry__ as g
        g.build()
    return pileup_gpu.load_library()


def test_header_symbols_equal_exports_and_bindings(lib):
    declared = set(re.findall(r"\b(pg_[a-z_]+)\s*\(", _text(HEADER)))
    assert declared == set(pileup_gpu.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pileup_gpu.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("pg_")}
    assert exported == declared
    for n in declared:
        assert hasattr(lib, n), n


def test_option_struct_and_limits_mirror_the_headers():
    body = re.search(r"typedef struct pe_options \{(.*?)\} pe_options;", _text(os.path.join(ROOT, "include", "dl4vc_loader.h")),
                     flags=re.S).group(1)
    fields = re.findall(r"int32_t\s+([a-z_]+);", body)
    assert fields == [n for n, _ in loader.PileupOptions._fields_]
    text = _text(HEADER)
    assert int(re.search(r"#define PG_MAX_TRACKS (\d+)", text).group(1)) == pileup_gpu.MAX_TRACKS >= 1024
    assert int(re.search(r"#define PG_MAX_WINDOW (\d+)", text).group(1)) == pileup_gpu.MAX_WINDOW >= 100


def test_encode_locations_refuses_an_unknown_device():
    for bad in ("cpu", "tpu"):
        with pytest.raises(ValueError):
            PE.encode_locations("x.bam", "x.fa", [], PE.EncoderOptions(), device=bad)
