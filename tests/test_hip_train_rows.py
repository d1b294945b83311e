"""The HIP training step at the row counts (sites x reads) where its launch schedules change, against the float64 training oracle.
GPU only.

Every launch of the step sizes its grid from the number of pileup rows and the card's compute-unit count: above ~128 rows the
half-read kernel staggers its second workgroup per CU, above ~256 a workgroup walks several units (alternating the 7-tile and the
6-tile half by round), the weight-gradient kernels take several rows per workgroup (prefetching across the row boundary), layer 1's
binned backward sums 256 partials 16 at a time, above 4096 statistics entries a block takes more than 32 of them, and from 17 sites
the FC stack runs on the tiled GEMM (several tiles, split K, a scalar store path for widths that are no multiple of 4).  The rest of
the suite stops at 112 rows; the benchmark runs 6400 and checks that the loss is finite.

Each case asserts, through the trainer's ``sched:`` facts (include/dl4vc_dan_train.h), that the step it ran DID cross the threshold
it is there for -- the row counts are chosen for 256 CUs, and on another count a case fails loudly instead of passing without
coverage -- then holds losses (5e-5), clip norm (2e-4) and every gradient tensor to the float64 oracle with the bars of
test_hip_train.run_train_step_check.  The slack is the fp32 oracle's distance under the SAME decisions as the float64 oracle it is
compared with, asserted <= 5e-5 (a cap on the reference: a case whose reference alone breaks it gets another seed, never a wider
cap).  Every case prints its record and writes it to train_row_schedules.json in the report directory of test_hip_train's production-width
record (-> profiles/train_row_schedules.json)."""
import dataclasses
import json
import os

import numpy as np
import pytest

import test_hip_train as H
from dl4vc_amd.config import DanConfig
from dl4vc_amd.train import DanTrainer, TrainHyper

pytestmark = pytest.mark.gpu

SCHED_KEYS = ("rowh_units_per_wg_max", "rowh_units_per_wg_min", "rowh_stagger", "row_reads_per_wg_max", "wgrad3_rows_per_wg_max",
              "wgrad3_rows_per_wg_min", "wgrad1_rows_per_wg_max", "wgradpool_rows_per_wg_max", "l0_rows_per_wg_max", "l0_partials",
              "stats_entries_per_block_max", "stats_blocks_max", "gemm_tiles_m_max", "gemm_tiles_n_max", "gemm_k_tiles_max",
              "gemm_splits_max", "fc1_streaming")


def sched_facts(tr):
    return {k: tr.query("sched:" + k) for k in SCHED_KEYS}


# 4 layers x 128 channels, bottleneck 32, BatchNorm, dilation 2, a pool after layer 2 (the generic weight-gradient form), residual
# layers 3 and 4 (the 1x1 weight-gradient form).  120 columns: the shortest window at which the 6-tile half of a read (columns >= 112)
# holds live columns; 3 weight-gradient chunks per row.
def S(reads, **kw):
    return DanConfig(reads=reads, length=120, layers=4, pool_layers=(2,), residual_start=3, fc_sizes=kw.pop("fc_sizes", (40, 12)), **kw)


def E(reads, fc_sizes):         # a small conv stack in front of the FC shapes under test (2 rows per site keep the oracle cheap)
    return DanConfig(reads=reads, length=64, layers=2, pool_layers=(), residual_start=0, c_init=16, c_final=16, bottleneck=4, fc_sizes=fc_sizes)


def D(reads):                   # 201 columns x 1320 rows = 4146 statistics tiles of the pointwise launches: more than 32 entries per block
    return DanConfig(reads=reads, length=201, layers=3, pool_layers=(1,), residual_start=2, c_init=8, c_final=8, bottleneck=4, fc_sizes=(24, 12))


def hyper(dropout, grad_clip, focal_gamma, label_smoothing, fp_train_weight=0.2):
    return TrainHyper(dropout=dropout, grad_clip=grad_clip, focal_gamma=focal_gamma, label_smoothing=label_smoothing, fp_train_weight=fp_train_weight)


# name -> (cfg, hyper, sites, (weight, pileup, target) seeds, what the step's schedule must have been: key -> (relation, value))
CASES = {
    # every half-read workgroup walks exactly 2 units, stagger on; 2 rows per 3-tap weight-gradient workgroup; 256 layer-1 partials
    "A_260_rows": (S(13), hyper(0.1, 1.0, 0.2, 0.001), 20, (101, 102, 103),
                   {"rowh_units_per_wg_max": ("==", 2), "rowh_units_per_wg_min": ("==", 2), "rowh_stagger": ("==", 1),
                    "wgrad3_rows_per_wg_max": ("==", 2), "l0_rows_per_wg_max": ("==", 2), "l0_partials": ("==", 256)}),
    # uneven rounds: some workgroups walk 2 units / rows, some 1
    "B_301_rows": (S(7), hyper(0.1, 0.0, 2.0, 0.05, 1.0), 43, (111, 112, 113),
                   {"rowh_units_per_wg_max": (">=", 2), "rowh_units_per_wg_min": ("<", "rowh_units_per_wg_max"),
                    "wgrad3_rows_per_wg_max": (">=", 2), "wgrad3_rows_per_wg_min": ("<", "wgrad3_rows_per_wg_max")}),
    # the same step with the whole-read Winograd form persistent (more rows than workgroups)
    "Bw_301_rows_winograd": (S(7, conv_algo=2), hyper(0.1, 0.0, 2.0, 0.05, 1.0), 43, (111, 112, 113),
                             {"row_reads_per_wg_max": (">=", 2)}),
    # (weight seed 124: with 121 one FC1 ReLU input of the float64 oracle is 2.1e-7 from zero and the fp32 oracle alone, flipping it,
    # sits 5.6e-2 of a tensor's max from float64 -- the reference broke its cap, so the seed changed)
    # three rounds (odd and even k_it), several rows per workgroup in the 1x1 and the pooled weight-gradient forms, 2 x 2 GEMM tiles
    "C_520_rows": (S(4, fc_sizes=(136, 20)), hyper(0.1, 1.0, 0.0, 0.0), 130, (124, 122, 123),
                   {"rowh_units_per_wg_max": (">=", 3), "wgrad1_rows_per_wg_max": (">=", 2), "wgradpool_rows_per_wg_max": (">=", 2),
                    "gemm_tiles_m_max": (">=", 2), "gemm_tiles_n_max": (">=", 2), "fc1_streaming": ("==", 0)}),
    # more than 32 statistics entries per block, >= 100 block partials for the single-workgroup BatchNorm kernels, six rounds
    "D_1320_rows": (D(12), hyper(0.0, 0.0, 0.2, 0.001), 110, (131, 132, 133),
                    {"stats_entries_per_block_max": (">", 32), "stats_blocks_max": (">=", 100), "rowh_units_per_wg_max": (">=", 6)}),
    # split K with more than one M tile
    "E1_129_sites_fc_520_132": (E(2, (520, 132)), hyper(0.1, 1.0, 0.2, 0.001), 129, (141, 142, 143),
                                {"gemm_splits_max": (">=", 2), "gemm_tiles_m_max": (">=", 2), "fc1_streaming": ("==", 0)}),
    # widths that are no multiple of 4 (the scalar store path); K = 257 in the weight gradients (eight k-tiles and a tail of 1);
    # three M tiles, one live row in the last
    "E2_257_sites_fc_130_18": (E(2, (130, 18)), hyper(0.1, 0.0, 2.0, 0.05), 257, (151, 152, 153),
                               {"gemm_k_tiles_max": (">=", 9), "gemm_tiles_m_max": ("==", 3), "gemm_tiles_n_max": (">=", 2), "fc1_streaming": ("==", 0)}),
    # the smallest tiled-GEMM batch at the odd widths (M is the sites in the forward and data-gradient products -- one tile with 17
    # live rows -- and FC1's 130 outputs, two tiles, in its weight gradient)
    "E3_17_sites_fc_130_18": (E(2, (130, 18)), hyper(0.1, 1.0, 0.0, 0.0, 1.0), 17, (161, 162, 163),
                              {"gemm_tiles_m_max": ("==", 2), "gemm_tiles_n_max": (">=", 2), "gemm_k_tiles_max": (">=", 1), "fc1_streaming": ("==", 0)}),
}

FREE_DECISION_MARGIN = 2e-6     # no highway / FC / coverage ReLU input of a case closer to zero than this in float64 (those decisions are
                                # not imposed on either oracle; FC1's fp32 forward sits ~1e-6 from float64, tests/test_hip_train.py)
_ORACLES = {}             # (structure without conv_algo, sites, seeds) -> the float64 oracle's result: B and B-w share one
_SESSION = {}             # case -> record, of THIS pytest session (the JSON file is rewritten from it, never merged with an older one)


def _report_path():
    return os.path.join(os.path.dirname(H._prod_width_report_path()), "train_row_schedules.json")    # (that helper creates the directory)


def assert_schedule(name, facts, expect):
    ops = {"==": lambda a, b: a == b, ">=": lambda a, b: a >= b, ">": lambda a, b: a > b, "<": lambda a, b: a < b}
    for key, (rel, value) in expect.items():
        bound = facts[value] if isinstance(value, str) else value
        assert ops[rel](facts[key], bound), "%s: sched:%s = %d, the case needs %s %s (%s): this card's CU count moves the threshold, re-size the case -- %s" % (
            name, key, facts[key], rel, value, bound, facts)


@pytest.mark.parametrize("name", list(CASES))
def test_train_step_at_schedule_thresholds(name):
    cfg, hp, sites, seeds, expect = CASES[name]
    if name.startswith(("E2", "E3")):
        assert cfg.fc_sizes[0] % 4 and cfg.fc_sizes[1] % 4, "E2 / E3 are the widths that are no multiple of 4 (the GEMM's scalar store path)"
    if name.startswith("E2"):
        assert sites // 32 == 8 and sites % 32 == 1 and (sites - 1) % 128 == 0, "K = sites: eight full k-tiles and a tail of 1; one live row in the last M tile"
    sd, planes, tg, masks = H.seeded_train_case(cfg, hp, sites, seeds)
    key = (dataclasses.replace(cfg, conv_algo=0), sites, seeds)
    tag = "%s: %d sites x %d reads x %d, fc %s, conv_algo %d" % (name, sites, cfg.reads, cfg.length, cfg.fc_sizes, cfg.conv_algo)
    rec = H.run_train_step_check(cfg, hp, sd, planes, tg, masks, sites, tag, slack_cap=H.SLACK_CAP,
                                 conv_margin_from_activations=cfg.conv_algo == 2, inspect=sched_facts,
                                 oracle_cache=_ORACLES.setdefault(key, {}), free_decision_margin=FREE_DECISION_MARGIN)
    rec["sched"] = rec.pop("inspect")
    rec["rows"] = sites * cfg.reads
    _SESSION[name] = rec
    json.dump(_SESSION, open(_report_path(), "w"), indent=1)
    print("%s: %d rows, %s branch, %d decisions differ, worst gradient %s at %.2g of its max, reference alone %.2g; sched %s" % (
        name, rec["rows"], rec["branch"], sum(d["count"] for d in rec["decisions_differing"]), rec["worst_gradient"]["tensor"],
        rec["worst_gradient"]["error_over_max"], rec["fp32_oracle_worst_distance_under_shared_decisions"], rec["sched"]))
    assert_schedule(name, rec["sched"], expect)


def test_larger_max_batch_gives_the_same_gradient_bytes():
    """Case C's step on a trainer created for 160 sites: the buffers a larger max_batch sizes (statistics, partials, the split-K
    workspace, the highway blocks) must not reach the result -- the flat gradient buffer and the losses are byte-equal to the
    step of the trainer created for exactly 130."""
    cfg, hp, sites, seeds, _ = CASES["C_520_rows"]
    sd, planes, tg, masks = H.seeded_train_case(cfg, hp, sites, seeds)
    got = []
    for max_batch in (sites, 160):
        tr = DanTrainer(cfg, hp, max_batch=max_batch).load_state_dict(sd)
        out = tr.train_step(planes, tg, dropout_masks=masks)
        got.append((tr.grad_tensor().cpu().numpy().tobytes(), [np.float32(out[k]).tobytes() for k in ("loss", "bin", "vt", "af", "cov", "vb", "vr")],
                    np.float32(out["grad_norm"]).tobytes(), sched_facts(tr)))
        tr.close()
    assert np.abs(np.frombuffer(got[0][0], np.float32)).max() > 0
    assert got[0][3] == got[1][3], "max_batch changed the schedule: %s vs %s" % (got[0][3], got[1][3])
    assert got[0][1] == got[1][1] and got[0][2] == got[1][2], "losses / clip norm differ between max_batch 130 and 160"
    assert got[0][0] == got[1][0], "the flat gradient buffer differs between max_batch 130 and 160"


def test_schedule_facts_follow_the_last_step_and_unknown_keys_stay_errors():
    """The facts are those of the LAST step (a 2-site step after a 20-site one reports the streaming FC forms), zero before any step
    and for forms that did not run, and an unknown key -- under ``sched:`` too -- keeps dan_train_query's error."""
    cfg = DanConfig(reads=2, length=64, layers=2, pool_layers=(), residual_start=0, bottleneck=4, fc_sizes=(24, 12))
    assert cfg.feature_width >= 8192, "the streaming forms need a long feature row"
    hp = hyper(0.0, 0.0, 0.2, 0.001)
    tr = None
    for sites in (20, 2):
        sd, planes, tg, masks = H.seeded_train_case(cfg, hp, sites, (171, 172, 173))
        if tr is None:
            tr = DanTrainer(cfg, hp, max_batch=20).load_state_dict(sd)
            assert all(tr.query("sched:" + k) == 0 for k in SCHED_KEYS), "no step has run yet"
        tr.backward(planes, tg, dropout_masks=masks)
        f = sched_facts(tr)
        assert f["rowh_units_per_wg_max"] == f["rowh_units_per_wg_min"] == 1 and f["rowh_stagger"] == 0, f
        assert f["row_reads_per_wg_max"] == 0 and f["wgradpool_rows_per_wg_max"] == 0, f          # (no Winograd form, no pool)
        assert f["wgrad3_rows_per_wg_max"] == f["wgrad3_rows_per_wg_min"] == 1, f
        assert f["l0_partials"] == 2 * sites and f["l0_rows_per_wg_max"] == 1, f
        assert 1 <= f["stats_blocks_max"] <= 3 and f["stats_entries_per_block_max"] == min(32, 4 * sites), f
        assert f["fc1_streaming"] == (1 if sites <= 16 else 0) and f["gemm_tiles_m_max"] == 1 and f["gemm_splits_max"] >= 1, f
    with pytest.raises(RuntimeError, match="unknown key 'sched:no_such_fact'"):
        tr.query("sched:no_such_fact")
    with pytest.raises(RuntimeError, match="unknown key 'rowh_stagger'"):
        tr.query("rowh_stagger")
    tr.close()
