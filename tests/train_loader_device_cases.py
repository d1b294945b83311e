"""Fixtures of the device training loader's tests (tests/test_train_loader_device_cli.py on the CPU,
tests/test_train_loader_device_gpu.py on the GPU): 45 labelled records in the layout of tests/loader_device_cases.py -- five whole
chunks of 8 and one of 5 -- the index lists a training epoch may ask for, and the host definition of what the device loader makes
of them: raw chunks -> ``zi_inflate_host`` -> ``site_assembly.plan_records`` -> ``site_assembly.assemble_host`` ->
``cl_center_counts_host`` -> targets."""
import numpy as np

from dl4vc_amd import hdf5io, synth, zinflate
from dl4vc_amd.chunk_loader import center_counts_host
from dl4vc_amd.hdf5_schema import record_dtype
from dl4vc_amd.site_assembly import assemble_host, plan_records
from dl4vc_amd.train_data import assemble_training_batch, read_indices, targets_from_counts

N = 45                      # five whole chunks of 8 and one of 5
STORED, READS = 20, 12      # stored rows per record, rows the model reads
READS_SEED = 5
DEEP, NO_READ, BLACK = (2, 9, 17, 30, 44), 11, 7
PLANES = ("reads", "qual", "strand", "ref", "ref_mask", "var_mask")


def labelled_records(n=N, stored=STORED, reads=READS, seed=31):
    """``synth.make_labelled_records`` narrowed to ``stored`` rows: some sites deeper than ``reads`` (their subset is drawn with
    the seed), one without any read, one blacklisted (REF does not match the window)."""
    wide = synth.make_labelled_records(n, reads, seed)
    recs = np.zeros(n, record_dtype(stored, 201))
    for name in recs.dtype.names:
        recs[name] = wide[name][:, :stored] if name in ("single_reads", "q-scores", "strand") else wide[name]
    rng = np.random.default_rng(3)
    for i in (d for d in DEEP if d < n):
        k = stored - (i % 4)
        have = max(1, int(recs[i]["num_reads"]))
        recs[i]["num_reads"] = k
        for f in ("single_reads", "q-scores", "strand"):
            recs[i][f][reads:k] = recs[i][f][rng.integers(0, have, k - reads)]
    if NO_READ < n:
        recs[NO_READ]["num_reads"] = 0
        for f in ("single_reads", "q-scores", "strand"):
            recs[NO_READ][f][:] = 0
    if BLACK < n:
        cols = recs[BLACK]["vcfrec"].decode().split("\t")
        cols[3] = next(b for b in "ACGT" if b not in (cols[3][0], cols[4][0])) + cols[3][1:]
        recs[BLACK]["vcfrec"] = "\t".join(cols).encode()
    return recs


def index_lists():
    """The lists of the issue: a seeded permutation of all 45 in batches of 8 (the last holds 5), a whole chunk in reverse, two
    non-adjacent indices of one chunk around another chunk's record, one index in the 5-record edge chunk, a single index."""
    perm = np.random.RandomState(17).permutation(N).astype(np.int64)
    lists = [perm[k:k + 8] for k in range(0, N, 8)]
    assert len(lists[-1]) == 5
    lists.append(np.arange(23, 15, -1, dtype=np.int64))                  # chunk 2, reversed
    lists.append(np.array([9, 30, 14], np.int64))                        # chunk 1, chunk 3, chunk 1
    lists.append(np.array([42], np.int64))                               # the edge chunk
    lists.append(np.array([NO_READ], np.int64))
    return lists


def draw_seed(epoch, n=N, reads_seed=READS_SEED):
    """``train_epoch``'s seed of the read subsets (epoch >= 1), evaluation's with ``epoch = 0``."""
    return reads_seed + epoch * n


def host_definition(path, idx, seed, reads=READS, non_snp_train_weight=2.0, keep_candidate_af=True):
    """-> (six planes, targets, blacklist, vcfrec) of the records ``idx`` of ``path`` by the loader's host definition."""
    idx = np.asarray(idx, np.int64)
    with hdf5io.RawChunkFile(path) as f:
        chunks, where = np.unique(idx // f.chunk, return_inverse=True)
        sizes = [f.stored_size(int(c)) for c in chunks]
        offs = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
        buf = np.zeros(sum(sizes), np.uint8)
        raw = [f.read_chunk(int(c), buf.ctypes.data + int(o)) & 1 for c, o in zip(chunks, offs)]
        out = np.full(len(chunks) * f.chunk_bytes, 0xAB, np.uint8)
        status = zinflate.inflate_streams(buf, offs, sizes, out, [k * f.chunk_bytes for k in range(len(chunks))],
                                          [f.chunk_bytes] * len(chunks), raw)
        assert (status == 0).all(), status
        dt = record_dtype((f.offsets["strand"] - f.offsets["q-scores"]) // 201, 201)
        assert dt.itemsize == f.itemsize
        slots = (where.reshape(-1) * f.chunk + idx % f.chunk).astype(np.int32)
    part = out.view(dt)
    texts = [bytes(v).decode() for v in part["vcfrec"]]
    plan = plan_records(slots, idx, part["num_reads"].reshape(-1), part["ref_bases"], texts, reads, dt["single_reads"].shape[0], seed)
    planes = assemble_host(part["single_reads"], part["q-scores"], part["strand"], plan)
    counts = center_counts_host(planes[0])
    targets = targets_from_counts(plan, part["label"].reshape(-1)[slots], counts, non_snp_train_weight, keep_candidate_af)
    return planes, targets, np.array(plan.blacklist, bool), list(plan.vcfrec)


def reference_batch(path, idx, seed, reads=READS, non_snp_train_weight=2.0, keep_candidate_af=True):
    """``assemble_training_batch`` on the records libhdf5 reads: what the host loaders hand the trainer."""
    idx = np.asarray(idx, np.int64)
    with hdf5io.CandidateFile(path) as src:
        return assemble_training_batch(read_indices(src, idx), idx, max_reads=reads, seed=seed, non_snp_train_weight=non_snp_train_weight,
                                       keep_candidate_af=keep_candidate_af)


def assert_equals_reference(got, want, idx):
    """``got``: (planes, targets, blacklist, vcfrec) as ``host_definition`` returns them; ``want``: a ``TrainBatch``."""
    planes, targets, blacklist, vcfrec = got
    for name, x, y in zip(PLANES, planes, want.planes()):
        x = np.asarray(x)
        assert x.dtype == np.uint8 and x.shape == y.shape and x.tobytes() == np.ascontiguousarray(y).tobytes(), name
    assert sorted(targets) == sorted(want.targets)
    for k, v in want.targets.items():
        assert targets[k].dtype == v.dtype and targets[k].tobytes() == v.tobytes(), (k, targets[k], v)
    assert (blacklist == want.blacklist).all() and vcfrec == list(want.sites.vcfrec)
    assert (np.asarray(idx, np.int64) == want.index).all()
