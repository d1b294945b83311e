"""Command-line surface of ``main.py`` -- a drop-in for the reference's flag set.

``call_variants.sh`` passes training-only flags to the inference run as well (reference:
call_variants.sh:101-147), so every flag of the reference parser (arguments.py:5-135) is accepted with
the same name, type and default; the ones the inference hot path acts on are marked ``*``.  The table
form (rather than a transcription of the reference's ``add_argument`` calls) is deliberate: one row
per flag = (names, kind, default).  Kinds: ``flag`` = store_true, ``int``/``float``/``str`` scalars,
``ints``/``strs`` = one-or-more values.
"""
from __future__ import annotations

import argparse

_FLAGS = [
    # ---- files / run control
    ("--train_file", "str", None), ("--test_file*", "req-str", None), ("--debug", "flag", False),
    ("--loss-debug-freq", "int", 0), ("--max-train-batches", "int", 0), ("--max-test-batches*", "int", 0),
    ("--batch-size", "int", 1000), ("--test-batch-size*", "int", 1000), ("--epochs", "int", 20),
    ("--epochs_skip_eval", "int", 0), ("--lr", "float", 0.01), ("--lr-decay", "float", 1.0),
    ("--grad-clip", "float", 0.0),
    # ---- loss shaping (training only)
    ("--label-smoothing", "float", 0.0), ("--close_match_window", "float", 2.0), ("--focal_loss_gamma", "float", 0.0),
    ("--focal_loss_alpha", "float", 1.0), ("--close_examples_sample_rate", "float", 1.0),
    ("--save_hard_example_records", "flag", False),
    ("--use-var-type-threshold*", "flag", False), ("--binary-weight", "float", 1.0), ("--no-cuda", "flag", False),
    ("--seed*", "int", 1), ("--log-interval", "int", 10),
    ("--save_vcf_records*", "flag", False), ("--save_vcf_records_file*", "str", ""), ("--sample_vcf*", "str", None),
    ("--gpus*", "int", 1), ("--num-data-workers", "int", 5), ("--modelsave", "str", "checkpoint.pth.tar"),
    ("--modelload*", "str", None),
    ("--train_holdout_chromosomes", "strs", []), ("--test_holdout_chromosomes", "strs", []),
    ("--shuffle_test", "flag", False), ("--gatk-table", "str", ""), ("--giab-table", "str", ""),
    ("--test-trust-region-table", "str", ""), ("--train-trust-region-table", "str", ""),
    ("--non-trust-train-weight", "float", 0.01), ("--fp-train-weight", "float", 1.0), ("--trust-snp-only", "flag", False),
    ("--non-snp-train-weight", "float", 1.0), ("--auxillary-loss-weight", "float", 0.0),
    ("--auxillary-loss-bases-weight", "float", 0.1), ("--auxillary-loss-allele-weight", "float", 1.0),
    ("--aux-keep-candidate-af", "flag", False), ("--early_loss_layers*", "ints", []),
    ("--early_loss_weight", "float", 0.1), ("--learn_early_loss_weight", "flag", False),
    ("--layer_loss_weight", "float", 0.01),
    # ---- augmentation (training only)
    ("--delay_augmentation_epochs", "int", 0), ("--rm_var_reads_rate", "float", 0.0),
    ("--rm_non_var_reads_rate", "float", 0.0), ("--training_use_directional_augmentation", "flag", False),
    ("--augmented_example_weight", "float", 0.2), ("--delta_loss_weight", "float", 10.0),
    ("--augment-single-reads", "flag", False), ("--augment-reference", "flag", False),
    ("--reads-dynamic-downsample-rate", "float", 0.0), ("--reads-dynamic-downsample-prob", "float", 0.0),
    # ---- model structure
    ("--model-conv-layers*", "int", 5), ("--model-ave-pool-layers*", "ints", [2]),
    ("--model-residual-layer-start*", "int", 0), ("--model-init-conv-channels*", "int", 128),
    ("--model-final-conv-channels*", "int", 128), ("--model_final_layer_dilation*", "int", 1),
    ("--model_middle_layer_dilation*", "int", 1), ("--model-hidden-dropout*", "float", 0.0),
    ("--model-batchnorm*", "flag", False), ("--model-use-q-scores*", "flag", False),
    ("--model-use-strands*", "flag", False), ("--model-highway-single-reads*", "flag", False),
    ("--model-bottleneck-size*", "int", 32), ("--model_concat_hw_reads*", "flag", False),
    ("--model-use-naive-var-vector*", "flag", False), ("--model-use-reads-ref-var-mask*", "flag", False),
    ("--model-use-AF*", "flag", False), ("--model_skip_final_maxpool*", "flag", False),
    ("--model_pool_combine_dimension*", "int", 2048),
    # ---- transformer variant (rejected by the hot path, parsed for compatibility)
    ("--use_transformer*", "flag", False), ("--transformer_encoder_heads", "int", 4),
    ("--num_transformer_layers", "int", 4), ("--transformer_feedforward_dim", "int", 64),
    ("--final_transformer_dims", "int", 64), ("--transformer_residual", "flag", False),
    ("--transformer_encoder_dropout", "float", 0.1),
]

# additions of this implementation (not in the reference); all optional
_EXTRA = [
    ("--reads-seed", "int", 0, "pins the random read subset of pileups deeper than 100 reads (the reference draws "
                               "it from an unseeded RNG, dl4vc/dataset.py:274-281)"),
    ("--sites-per-launch", "int", 4096, "candidate sites per device launch (FC macro-batch)"),
    ("--shard", "str", "", "i/n: process only the i-th of n contiguous site shards (multi-GPU launch sets this)"),
    ("--precision", "str", "fp32", "conv-stack arithmetic: fp32 (exact fp32 MFMA, default), bf16x3 (split bf16, scores "
                                   "within 1e-4, ~2.3x faster) or bf16"),
    ("--compute-empty-rows", "flag", False, "compute every all-padding pileup row separately, as the reference does (default: once "
                                            "per site -- their inputs are identical, the outputs bit-identical)"),
    ("--test_bam", "str", None, "inference straight from a coordinate-sorted BAM (with --test_fasta and --sample_vcf, the candidate "
                                "VCF): pileups are encoded and scored on the GPU and no candidates.hdf is written; replaces --test_file"),
    ("--test_fasta", "str", None, "reference FASTA of --test_bam"),
    ("--inflate-device", "str", None, "gpu: with --test_bam or --train_bam, the pileup encoder inflates the BAM's BGZF blocks and frames its records "
                                      "on the GPU as well (needs the .bai; same scored VCF)"),
    ("--loader-device", "str", None, "gpu: with --test_file, the file's HDF5 chunks are inflated and its sites assembled on the GPU "
                                     "(the host only reads the raw chunks and plans rows and allele masks); same scored VCF"),
    ("--train-loader-device", "str", None, "gpu: with --train_file, the training batches and the per-epoch evaluation batches are "
                                           "assembled on the GPU (raw HDF5 chunks inflated on the device, shuffled records "
                                           "gathered there, targets from a device histogram); --num-data-workers starts no "
                                           "worker process; same losses, checkpoints and scored VCF"),
    ("--train-cache-device", "str", argparse.SUPPRESS,
     "gpu: with --train-loader-device gpu, each of the two files is inflated ONCE when its loader opens and kept in device memory, "
     "its records trimmed of their trailing all-zero rows (an estimated sixth of the inflated size at 30x, not measured; the fill prints the real ratio); every batch of every epoch "
     "and every evaluation pass is gathered from there, with no file read and no inflate beside the step.  The whole file is resident "
     "or the run ends (no fallback); a damaged chunk ends the run during the fill, whether or not an index would ever have fallen "
     "in it; --gpus N keeps one copy per rank; 3.4 KB of host memory per record; same losses, checkpoints and scored VCF"),
    ("--train-cache-bytes", "int", argparse.SUPPRESS,
     "with --train-cache-device gpu: the bytes the trimmed records of --train_file and --test_file may take together in device "
     "memory (default 0: three quarters of the device memory that is free when the first loader opens).  It bounds the records' bytes, "
     "not the allocations: the store grows in slabs of 256 MiB (or what the budget leaves), so each file may take up to one slab more"),
    ("--train-cache-format", "str", argparse.SUPPRESS,
     "with --train-cache-device gpu: rows (the default: the three planes of every record trimmed of their trailing all-zero rows) or "
     "compact (every stored row cut to the columns between its first and its last non-zero byte, token and strand merged into one "
     "byte; a record with a token or strand value of 16 or more keeps the rows layout).  compact took 0.30 of the rows layout's "
     "bytes on the records of a synthetic 30x pileup (computed on the CPU; no real pileup measured), so the same budget holds that "
     "many more records; the fill prints the real ratio and how many records fell back; same batches, losses, checkpoints and "
     "scored VCF"),
    ("--train_bam", "str", argparse.SUPPRESS,
     "training straight from a coordinate-sorted BAM (with --train_fasta, the labelled location VCFs --train_tp_vcf / --train_fn_vcf / "
     "--train_fp_vcf, --train-loader-device gpu and --train-cache-device gpu): the GPU pileup encoder's planes go into the resident "
     "record store where they lie and no train.hdf is written; replaces --train_file.  Record i is record i of the file "
     "tools/convert_bam_single_reads.py would write from the same VCFs; same losses, checkpoints and scored VCF.  Evaluation reads "
     "--test_file, or --test_bam with --test_fasta (locations from the --test_*_vcf flags, or --sample_vcf with label 2)"),
    ("--train_fasta", "str", argparse.SUPPRESS, "reference FASTA of --train_bam"),
    ("--train_tp_vcf", "str", argparse.SUPPRESS, "with --train_bam: VCF of the true-positive locations (label 0), the converter's --tp_vcf"),
    ("--train_tp_full_vcf", "str", argparse.SUPPRESS, "with --train_tp_vcf: the VCF that carries their genotypes, the converter's --tp_full_vcf"),
    ("--train_fn_vcf", "str", argparse.SUPPRESS, "with --train_bam: VCF of the false-negative locations (label 1), the converter's --fn_vcf"),
    ("--train_fp_vcf", "str", argparse.SUPPRESS, "with --train_bam: VCF of the false-positive locations (label 2), the converter's --fp_vcf"),
    ("--test_tp_vcf", "str", argparse.SUPPRESS, "with --train_bam and --test_bam: as --train_tp_vcf, for the evaluation records"),
    ("--test_tp_full_vcf", "str", argparse.SUPPRESS, "with --test_tp_vcf: as --train_tp_full_vcf"),
    ("--test_fn_vcf", "str", argparse.SUPPRESS, "with --train_bam and --test_bam: as --train_fn_vcf"),
    ("--test_fp_vcf", "str", argparse.SUPPRESS, "with --train_bam and --test_bam: as --train_fp_vcf"),
    ("--subsample", "float", argparse.SUPPRESS,
     "with --test_bam / --train_bam: keep the fraction F in (0, 1] of the reads of every BAM this run opens, chosen by a hash of the "
     "read name as `samtools view --subsample F` chooses them (mates stay together), in front of the pileup: the scored VCF, losses "
     "and checkpoints are those of the BAM tools/subsample_bam.py writes.  Give candidate generation the same F and seed"),
    ("--subsample-seed", "int", argparse.SUPPRESS, "seed of --subsample in [0, 2^32) (default 0): another seed keeps another subset"),
    ("--min-mapq", "int", argparse.SUPPRESS,
     "with --test_bam / --train_bam: drop the reads of every BAM this run opens whose mapping quality is below Q in [0, 255], in front "
     "of the pileup (samtools view -q).  Give candidate generation the same filter"),
    ("--exclude-flags", "str", argparse.SUPPRESS, "with --test_bam / --train_bam: drop the reads with any of these flag bits (decimal "
                                                  "or 0x..., samtools view -F)"),
    ("--require-flags", "str", argparse.SUPPRESS, "with --test_bam / --train_bam: drop the reads that lack any of these flag bits "
                                                  "(decimal or 0x..., samtools view -f)"),
    ("--read-stats", "flag", False, "with --test_bam / --train_bam: print the read census of the GPU encoder's records (totals, flag "
                                    "bits by name, MAPQ histogram), with or without a filter"),
    ("--record-census", "str", None, "gpu: with --test_bam, the locations are censused first (which of them give a record, by the GPU "
                                     "encoder's status rule without its planes), so that --gpus N, --shard g/N, "
                                     "--test_holdout_chromosomes and --max-test-batches select and seed the records as --test_file "
                                     "does; same scored VCF"),
    ("--census-timeout", "float", 600.0, "seconds a --record-census shard waits for the census of the other shards"),
    ("--conv-algo", "str", "auto", "fp32 conv form: auto (Winograd F(2,3) where every layer after the first has "
                                   "dilation 2), direct, or winograd"),
]

_TYPES = {"int": int, "float": float, "str": str}
# help texts of reference flags whose meaning here needs a word
_HELP = {
    "--reads-dynamic-downsample-rate": "training: mean share of a site's reads dropped by dynamic read down-sampling, in [0, 1); the "
                                       "site's own share is drawn from a normal around it and clipped to [0, 0.8].  Needs "
                                       "--reads-dynamic-downsample-prob.  Every loader applies it, the GPU-resident ones included; "
                                       "evaluation never does",
    "--reads-dynamic-downsample-prob": "training: share of the sites that are down-sampled, in [0, 1].  The reference draws from "
                                       "the unseeded global generator; here site i of a file of n records draws in epoch e (from 1) "
                                       "with RandomState(reads_seed + e * n + i), the seed of its read subset, so every epoch "
                                       "drops other reads and a run is reproducible",
}


def create_arg_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="DL4VC DAN variant caller -- MI355X-native inference path")
    for name, kind, default in _FLAGS:
        name = name.rstrip("*")
        if kind == "flag":
            p.add_argument(name, action="store_true", default=default)
        elif kind == "req-str":
            p.add_argument(name, type=str, required=True)
        elif kind in ("ints", "strs"):
            p.add_argument(name, type=int if kind == "ints" else str, nargs="+", default=list(default))
        else:
            p.add_argument(name, type=_TYPES[kind], default=default, help=_HELP.get(name))
    for name, kind, default, text in _EXTRA:
        if kind == "flag":
            p.add_argument(name, action="store_true", default=default, help=text)
        else:
            p.add_argument(name, type=_TYPES[kind], default=default, help=text)
    return p


def parse_args(argv=None) -> argparse.Namespace:
    """``create_arg_parser().parse_args(argv)``, except that ``--test_file`` is not required where ``--test_bam`` stands in
    for it, or where ``--train_bam`` is given (main.py then says which of the two is missing); the parser itself keeps the
    reference's ``required=True``."""
    import sys
    argv = list(sys.argv[1:] if argv is None else argv)
    p = create_arg_parser()
    if any(a in ("--test_bam", "--train_bam") or a.startswith(("--test_bam=", "--train_bam=")) for a in argv):
        for a in p._actions:
            if a.dest == "test_file":
                a.required = False
    return p.parse_args(argv)
