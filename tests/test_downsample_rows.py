"""Dynamic read down-sampling (``--reads-dynamic-downsample-rate`` / ``-prob``) without a GPU: the row plan against what the
reference's own ``sample_single_reads`` returned (tests/golden/dataset_downsample.npz, written by
tools/gen_golden_downsample.py), the native plan against the Python one, the flags at 0 against today's functions, the host
loaders against each other, and the CPU twin of the store's gather with flagged plan entries."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
import train_loader_device_cases as TC
from dl4vc_amd import hdf5io, loader
from dl4vc_amd.dataset import gather_rows, plan_rows, select_rows
from dl4vc_amd.site_assembly import ZERO_READS, SitePlan, assemble_host, plan_records

N, STORED, READS = 24, 20, 12
RATE, PROB = 0.3, 0.5


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "dataset_downsample.npz")))


def _cases(g):
    return zip(g["num_reads"].tolist(), g["model_reads"].tolist(), g["rate"].tolist(), g["prob"].tolist(), g["seed"].tolist())


def test_fixture_holds_the_cases_of_the_issue(golden):
    g = golden
    assert set(g["num_reads"].tolist()) == {0, 1, 3, 4, 5, 40, 99, 100, 101, 150, 199, 200, 201, 260, 400}
    assert set(g["model_reads"].tolist()) == {8, 64, 100}
    assert set(zip(g["rate"].tolist(), g["prob"].tolist())) == {(0.3, 1.0), (0.3, 0.5), (0.79, 1.0), (0.3, 0.0)}
    assert len(g["seed"]) == 15 * 3 * 4 * 8
    for j, kind in enumerate(g["kind_names"].tolist()):
        assert g["kinds"][:, j].any(), kind
    for p in ("record_reads", "record_qual", "record_strand"):
        assert g[p].shape == (200, 9) and g[p].all()               # row 199 included: the reads-only zeroing shows


def test_python_plan_and_planes_equal_the_reference(golden):
    g = golden
    S = g["record_reads"].shape[0]
    for i, (n, R, rate, prob, seed) in enumerate(_cases(g)):
        rows, zero, sampled = plan_rows(n, S, R, np.random.RandomState(seed), rate, prob)
        k = min(R, S)
        assert len(rows) == k and np.array_equal(rows, g["perm"][i, :k]), (i, n, R, rate, prob, seed)
        assert np.array_equal(zero, g["zero_reads"][i, :k] != 0) and sampled == g["sampled"][i], (i, n, R, rate, prob, seed)
        got = (gather_rows(g["record_reads"], rows, zero), gather_rows(g["record_qual"], rows), gather_rows(g["record_strand"], rows))
        for name, a in zip(("reads", "qual", "strand"), got):
            assert a.tobytes() == g[name][i, :k].tobytes(), (name, i, n, R, rate, prob, seed)


def test_native_plan_equals_the_python_plan(golden):
    g = golden
    S = g["record_reads"].shape[0]
    for i, (n, R, rate, prob, seed) in enumerate(_cases(g)):
        rows, zero, sampled = loader.select_rows_downsample(seed, n, S, R, rate, prob)
        k = min(R, S)
        assert np.array_equal(rows, g["perm"][i, :k]) and np.array_equal(zero, g["zero_reads"][i, :k] != 0), (i, n, R, rate, prob, seed)
        assert sampled == g["sampled"][i], (i, n, R, rate, prob, seed)       # (the legacy normal, through the integer it gives)
    rng = np.random.RandomState(11)
    for _ in range(2000):
        seed, n, S, R = int(rng.randint(0, 2 ** 31)), int(rng.randint(0, 420)), int(rng.choice([20, 150, 200])), int(rng.choice([8, 64, 100]))
        rate, prob = float(rng.choice([0.05, 0.3, 0.5, 0.79, 0.95])), float(rng.choice([0.2, 0.5, 1.0]))
        want = plan_rows(n, S, R, np.random.RandomState(seed), rate, prob)
        got = loader.select_rows_downsample(seed, n, S, R, rate, prob)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (seed, n, S, R, rate, prob)


def test_flags_off_is_todays_plan():
    lib = loader.load_library()
    rng = np.random.RandomState(12)
    out = np.zeros(512, np.int32)
    for _ in range(2000):
        seed, n, S, R = int(rng.randint(0, 2 ** 31)), int(rng.randint(0, 420)), int(rng.choice([20, 150, 200])), int(rng.choice([8, 64, 100]))
        today = np.random.RandomState(seed)
        today.random_sample()
        want = select_rows(n, S, R, today)
        rows, zero, sampled = plan_rows(n, S, R, np.random.RandomState(seed), 0.0, 0.0)
        assert np.array_equal(rows, want) and not zero.any() and sampled == n
        k = lib.dl_select_rows(seed, n, S, R, out.ctypes.data_as(C.POINTER(C.c_int32)))
        got = loader.select_rows_downsample(seed, n, S, R, 0.0, 0.0)
        assert np.array_equal(got[0], out[:k]) and np.array_equal(got[0], want) and not got[1].any() and got[2] == n


def test_native_plan_refuses_bad_arguments():
    for rate, prob in ((1.0, 0.5), (-0.1, 0.5), (0.3, 1.5), (0.3, -0.5), (float("nan"), 0.5)):
        with pytest.raises(ValueError, match="dl_select_rows_downsample: bad argument"):
            loader.select_rows_downsample(1, 10, 20, 8, rate, prob)


def test_native_plan_and_cpu_twin_under_the_sanitizers():
    """tools/asan_downsample.sh: a stand-alone program over the golden cases, every buffer ending where its data ends."""
    import subprocess
    from conftest import ROOT
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan_downsample.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "asan_downsample: ok (1440 cases" in r.stdout


@pytest.fixture(scope="module")
def train_file(tmp_path_factory):
    recs = TC.labelled_records(N, STORED, READS)
    path = str(tmp_path_factory.mktemp("downsample") / "train.hdf")
    hdf5io.write_candidates(path, recs)
    return path, recs


def _native_planes(recs, idx, seed, rate, prob):
    """The batch by the native plan (``plan_records`` -> ``dl_select_rows_downsample``) and the numpy gather."""
    texts = [bytes(v).rstrip(b"\x00").decode() for v in recs["vcfrec"]]
    plan = plan_records(np.asarray(idx, np.int32), idx, recs["num_reads"].reshape(-1), recs["ref_bases"], texts, READS, STORED, seed, rate, prob)
    return plan, assemble_host(recs["single_reads"], recs["q-scores"], recs["strand"], plan)


def test_host_loaders_give_identical_batches(train_file):
    from dl4vc_amd.train_data import BatchPrefetcher
    path, recs = train_file
    order = np.random.RandomState(3).permutation(N).astype(np.int64)
    lists = [order[0:7], order[7:14], order[14:21], order[21:24]]
    epochs = {}
    for epoch in (1, 2):
        seed = TC.draw_seed(epoch, N)
        kw = dict(max_reads=READS, seed=seed, non_snp_train_weight=0.5, downsample_rate=RATE, downsample_prob=PROB)
        with BatchPrefetcher(path, workers=0) as p0:
            want = list(p0.batches(iter(lists), **kw))
        with BatchPrefetcher(path, workers=2, depth=2) as p2:
            got = list(p2.batches(iter(lists), **kw))
        assert len(want) == len(got) == len(lists)
        for g, w, idx in zip(got, want, lists):
            plan, native = _native_planes(recs, idx, seed, RATE, PROB)
            assert np.array_equal(g.index, idx) and np.array_equal(w.index, idx)
            for name, a, b, c in zip(TC.PLANES, g.planes(), w.planes(), native):
                assert a.tobytes() == b.tobytes() == np.ascontiguousarray(c).tobytes(), (name, epoch)
            for k in w.targets:
                assert g.targets[k].tobytes() == w.targets[k].tobytes(), k
            assert np.array_equal(g.sampled, w.sampled) and np.array_equal(plan.sampled, w.sampled)
        epochs[epoch] = want
    # an epoch drops other reads than the one before: at a site both epochs down-sampled the planes differ
    differ = both = 0
    for a, b in zip(epochs[1], epochs[2]):
        hit = (a.sampled < a.sites.num_reads) & (b.sampled < b.sites.num_reads)
        both += int(hit.sum())
        differ += sum(a.sites.reads[i].tobytes() != b.sites.reads[i].tobytes() for i in np.flatnonzero(hit))
    assert both > 0 and differ > 0
    # a fill row shows zero tokens over the last stored row's quality
    filled = [(b, i) for b in epochs[1] for i in np.flatnonzero((b.sampled < b.sites.num_reads) & (b.sampled < READS))]
    assert filled
    for b, i in filled:
        assert not b.sites.reads[i][-1].any() and b.sites.qual[i][-1].tobytes() == recs[b.index[i]]["q-scores"][STORED - 1].tobytes()


def test_plans_with_the_flags_off_carry_no_flag_bit(train_file):
    _path, recs = train_file
    idx = np.arange(N, dtype=np.int64)
    plan, planes = _native_planes(recs, idx, 77, 0.0, 0.0)
    assert not (plan.rows & ZERO_READS).any() and np.array_equal(plan.sampled, plan.num_reads)
    texts = [bytes(v).rstrip(b"\x00").decode() for v in recs["vcfrec"]]
    today = plan_records(idx.astype(np.int32), idx, recs["num_reads"].reshape(-1), recs["ref_bases"], texts, READS, STORED, 77)
    assert np.array_equal(today.rows, plan.rows) and np.array_equal(today.first_rows, plan.first_rows)
    on, _ = _native_planes(recs, idx, 77, RATE, 1.0)
    assert (on.rows & ZERO_READS).any()                              # (and with them on, some do)


@pytest.mark.parametrize("record_format", ["rows", "compact"])
def test_cpu_twin_of_the_store_gather_follows_flagged_plans(train_file, record_format):
    """``cl_store_assemble_host`` against the numpy gather: plans of a down-sampled epoch, one that flags every row and one that
    flags none."""
    from dl4vc_amd.chunk_loader import RecordStore
    _path, recs = train_file
    planes = [np.ascontiguousarray(recs[f]) for f in ("single_reads", "q-scores", "strand")]
    idx = np.arange(N, dtype=np.int64)
    with RecordStore(201, STORED, N, 1 << 30, 1 << 20, device=-1, record_format=record_format) as st:
        st.pack_planes_host(*planes, np.arange(N), np.arange(N))
        if record_format == "compact":
            assert st.format_stats().compact_records > 0
        plan, want = _native_planes(recs, idx, 91, RATE, 1.0)
        every = SitePlan(plan.slots, (np.arange(STORED - READS, STORED, dtype=np.int16) | ZERO_READS)[None, :].repeat(N, 0),
                         np.zeros(N, np.uint8), plan.ref, plan.ref_mask, plan.var_mask, plan.vcfrec, plan.num_reads, plan.blacklist)
        none = SitePlan(plan.slots, np.arange(1, READS + 1, dtype=np.int16)[None, :].repeat(N, 0), np.zeros(N, np.uint8), plan.ref,
                        plan.ref_mask, plan.var_mask, plan.vcfrec, plan.num_reads, plan.blacklist)
        for p in (plan, every, none):
            want = assemble_host(*planes, p)
            got = st.assemble_host(p.slots, p.rows, p.first_rows, READS, (p.ref, p.ref_mask, p.var_mask))
            for name, a, b in zip(TC.PLANES, got, want):
                assert a.tobytes() == np.ascontiguousarray(b).tobytes(), name
        assert not assemble_host(*planes, every)[0].any() and assemble_host(*planes, every)[1].any()
        # the bit is not part of the row: a flagged entry past the stored rows is refused like a plain one
        bad = plan.rows.copy()
        bad[0, 0] = STORED | ZERO_READS
        with pytest.raises(ValueError, match="names stored row %d of %d" % (STORED, STORED)):
            st.assemble_host(plan.slots, bad, np.zeros(N, np.uint8), READS, (plan.ref, plan.ref_mask, plan.var_mask))
