"""The BGZF inflate kernel on the MI355X (``bz_inflate``): the case grid of tests/bgzf_cases.py with the assertions of
tests/test_bgzf_inflate_host.py (the same decode core runs there on the CPU, and under sanitizers by tools/asan_bgzf.sh), then
many blocks in one launch."""
import numpy as np
import pytest

from tests import bgzf_cases as G

pytestmark = pytest.mark.gpu


def test_valid_cases_equal_zlib():
    cases = G.valid_cases()
    out, out_off, status = G.run(cases, 0)
    G.assert_valid(cases, out, out_off, status)


@pytest.mark.parametrize("bad", G.damaged_cases(), ids=lambda c: c.name)
def test_damaged_case_is_a_status(bad):
    G.check_damaged(bad, 0)


def test_300_mixed_blocks_in_any_order():
    """Many workgroups and every slot alignment: 300 blocks of the valid cases in one call equal zlib, and the same blocks
    given in reversed order with their slots permuted give the same bytes in each block's slot."""
    valid = G.valid_cases()
    cases = [valid[(i * 5 + i // 7) % len(valid)] for i in range(300)]
    out, out_off, status = G.run(cases, 0, gap=3)
    G.assert_valid(cases, out, out_off, status)
    perm = list(np.random.default_rng(2).permutation(300))
    rev = cases[::-1]
    out2, out_off2, status2 = G.run(rev, 0, gap=7, order=perm)
    G.assert_valid(rev, out2, out_off2, status2)
    for i, c in enumerate(cases):
        a, b = int(out_off[i]), int(out_off2[299 - i])
        assert (out[a:a + c.isize] == out2[b:b + c.isize]).all()
