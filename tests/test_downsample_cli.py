"""The command line of dynamic read down-sampling: what ``main.py`` refuses, with the reason, before it touches a device, and how
the two flags parse."""
import os
import sys

import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), ".."))
import main as cli   # noqa: E402
from arguments import create_arg_parser, parse_args   # noqa: E402

TRAIN = ["--train_file", "t.hdf", "--test_file", "x.hdf", "--model_pool_combine_dimension", "0"]
RATE, PROB = "--reads-dynamic-downsample-rate", "--reads-dynamic-downsample-prob"


@pytest.mark.parametrize("flags, message", [
    ([RATE, "1.0", PROB, "0.5"], r"--reads-dynamic-downsample-rate must lie in \[0, 1\)"),
    ([RATE, "-0.1", PROB, "0.5"], r"--reads-dynamic-downsample-rate must lie in \[0, 1\)"),
    ([RATE, "0.3", PROB, "1.5"], r"--reads-dynamic-downsample-prob must lie in \[0, 1\]"),
    ([RATE, "0.3", PROB, "-0.5"], r"--reads-dynamic-downsample-prob must lie in \[0, 1\]"),
    ([RATE, "0.3"], "--reads-dynamic-downsample-rate is given without --reads-dynamic-downsample-prob"),
    ([PROB, "0.5"], "--reads-dynamic-downsample-prob is given without --reads-dynamic-downsample-rate"),
])
def test_refusals_with_a_training_file(flags, message):
    with pytest.raises(SystemExit, match=message):
        cli.main(TRAIN + flags)


def test_refused_without_a_training_source():
    with pytest.raises(SystemExit, match="training options: they need --train_file or --train_bam"):
        cli.main(["--test_file", "x.hdf", "--model_pool_combine_dimension", "0", RATE, "0.3", PROB, "0.5"])


def test_flags_parse_as_the_reference_declares_them():
    """The reference's arguments.py:102-103: both ``type=float, default=0.``."""
    args = parse_args(TRAIN)
    assert args.reads_dynamic_downsample_rate == 0.0 and args.reads_dynamic_downsample_prob == 0.0
    assert isinstance(args.reads_dynamic_downsample_rate, float) and isinstance(args.reads_dynamic_downsample_prob, float)
    args = parse_args(TRAIN + [RATE, "0.3", PROB, "0.5"])
    assert (args.reads_dynamic_downsample_rate, args.reads_dynamic_downsample_prob) == (0.3, 0.5)
    cli.check_downsample_arguments(args)                              # accepted: no longer on the refused list
    cli.check_downsample_arguments(parse_args(TRAIN))                 # both off: nothing to refuse
    text = create_arg_parser().format_help()
    assert "reads_seed + e * n + i" in " ".join(text.split())          # the per-epoch seed is stated where the flag is


def test_other_augmentations_stay_refused():
    with pytest.raises(SystemExit, match="augment-single-reads"):
        cli.main(TRAIN + ["--augment-single-reads", RATE, "0.3", PROB, "0.5"])
    with pytest.raises(SystemExit, match="rm_var_reads_rate"):
        cli.main(TRAIN + ["--rm_var_reads_rate", "0.1"])
