#!/bin/bash
# Steps 1-2 of the training recipe (reference docs/Step-by-step.md:40-96) as one command: BAM -> candidates.vcf
# (tools/candidate_generator.py, allele counting on the GPU, with the docs' flags) -> true / false positives against a truth
# VCF (tools/vcf_isec.py, bcftools isec -p's pairing: same CHROM, POS, REF and ALT set) -> OUTDIR/train.hdf
# (tools/convert_bam_single_reads.py: isec/0003.vcf as --tp_vcf with label 0, isec/0002.vcf as --tp_full_vcf for the truth's
# GT, isec/0001.vcf as --fp_vcf with label 2).  A multi-allelic truth record (1/2) pairs only with a candidate of the same
# ALT set, so its split candidates are labelled false positives; split such truth records beforehand if that is not wanted.
# Stages whose output already exists in OUTDIR are skipped.
# -c: the converter builds the pileups on the GPU and packs and compresses train.hdf's chunks there (--pileup-device gpu
# --compress-device gpu): the same records.
# -y (with -c): the compressed chunks get dynamic Huffman codes where they are smaller (--compress-codes dynamic): a smaller file.
# -n: stop after isec/ -- no train.hdf is written -- and print the main.py flags that train straight from the BAM with these
# outputs (--train_bam: the pileups are encoded on the GPU into the resident record store, the same records in the same order).
# -f: the candidate generator walks the reads that have no MD tag against REFERENCE (--reference; whole contigs on the GPU, 1 byte
# per base) instead of giving them no alleles; reads with an MD tag are walked by it as before.  Not passed by default.
# -L (implies -f): the candidate generator moves every insertion and deletion to its left-most placement on REFERENCE before it is
# counted (--left-align), and tools/vcf_isec.py left-aligns the simple indels of both the truth set and the candidates the same
# way before it pairs them (--left-align REFERENCE): a candidate and a truth record that name one event at two placements of a
# repeat pair.  Reads are not realigned.  Not passed by default.
# -s F [-S SEED]: candidate generation and the converter (with -n: the printed --train_bam flags) keep the fraction F in (0, 1] of
# the BAM's reads, chosen by a hash of the read name (--subsample / --subsample-seed): training data at F of the coverage.
# -q Q, -F MASK, -R MASK: candidate generation and the converter (with -n: the printed --train_bam flags) drop the reads with
# MAPQ < Q, with any flag bit of -F or without a flag bit of -R (--min-mapq / --exclude-flags / --require-flags).
set -e
usage() { echo "Usage: $0 -i BAM -r REFERENCE -t TRUTH.vcf[.gz] -o OUTDIR [-b BED] [-p PROCESSES] [-c [-y]] [-n] [-f] [-L] [-s FRACTION [-S SEED]] [-q MIN_MAPQ] [-F EXCLUDE_FLAGS] [-R REQUIRE_FLAGS]"; exit 1; }
PROCS=16
COMPRESS=""
CODES=""
NOFILE=""
FROMREF=""
LEFTALIGN=""
SUBSAMPLE=""
SEED=""
MINMAPQ=""
EXCLUDE=""
REQUIRE=""
while getopts "i:r:t:o:b:p:s:S:q:F:R:nfLcyh" opt; do
  case $opt in
    i) BAM=$OPTARG ;;
    r) REFERENCE=$OPTARG ;;
    t) TRUTH=$OPTARG ;;
    o) OUTDIR=$OPTARG ;;
    b) BED=$OPTARG ;;       # candidate generation only
    p) PROCS=$OPTARG ;;
    c) COMPRESS=gpu ;;
    y) CODES=dynamic ;;
    n) NOFILE=1 ;;
    f) FROMREF=1 ;;         # candidate generation: reads without MD are walked against REFERENCE
    L) LEFTALIGN=1; FROMREF=1 ;;  # indels left-aligned on REFERENCE: in candidate generation and on both sides of the pairing
    s) SUBSAMPLE=$OPTARG ;; # every BAM reader keeps this fraction of the reads (--subsample)
    S) SEED=$OPTARG ;;      # with -s: the seed (--subsample-seed)
    q) MINMAPQ=$OPTARG ;;   # every BAM reader drops the reads below this mapping quality (--min-mapq)
    F) EXCLUDE=$OPTARG ;;   # ... and the reads with any of these flag bits (--exclude-flags)
    R) REQUIRE=$OPTARG ;;   # ... and the reads without any of these flag bits (--require-flags)
    *) usage ;;
  esac
done
[ -n "$LEFTALIGN" ] && [ -z "$REFERENCE" ] && { echo "-L left-aligns the indels on the reference: give -r REFERENCE as well"; exit 1; }
[ -n "$FROMREF" ] && [ -z "$REFERENCE" ] && { echo "-f walks the reads without MD against the reference: give -r REFERENCE as well"; exit 1; }
[ -z "$BAM" ] || [ -z "$REFERENCE" ] || [ -z "$TRUTH" ] || [ -z "$OUTDIR" ] && usage
[ -n "$CODES" ] && [ -z "$COMPRESS" ] && { echo "-y chooses the codes of the chunks -c compresses: give -c as well"; exit 1; }
[ -n "$NOFILE" ] && [ -n "$COMPRESS" ] && { echo "-n writes no train.hdf, so there is nothing for -c to compress: give one of them"; exit 1; }
[ -n "$SEED" ] && [ -z "$SUBSAMPLE" ] && { echo "-S is the seed of -s: give -s FRACTION as well"; exit 1; }
SUBFLAGS=(${SUBSAMPLE:+--subsample "$SUBSAMPLE"} ${SEED:+--subsample-seed "$SEED"} ${MINMAPQ:+--min-mapq "$MINMAPQ"} \
          ${EXCLUDE:+--exclude-flags "$EXCLUDE"} ${REQUIRE:+--require-flags "$REQUIRE"})
SCRIPTDIR="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
mkdir -p "$OUTDIR"
if [ ! -f "$OUTDIR/candidates.vcf" ]; then
  printf "Generate candidate VCF...\n"
  python "$SCRIPTDIR/tools/candidate_generator.py" --input "$BAM" --output "$OUTDIR/candidates.vcf" \
      --snp_min_freq 0.075 --indel_min_freq 0.02 ${BED:+--bedfile "$BED"} --keep_multialleles \
      ${FROMREF:+--reference "$REFERENCE"} ${LEFTALIGN:+--left-align} "${SUBFLAGS[@]}" > "$OUTDIR/candidate_generator.log" 2>&1
fi
if [ ! -f "$OUTDIR/isec/0003.vcf" ]; then
  printf "Intersect candidates with the truth set...\n"
  python "$SCRIPTDIR/tools/vcf_isec.py" -p "$OUTDIR/isec" ${LEFTALIGN:+--left-align "$REFERENCE"} "$TRUTH" "$OUTDIR/candidates.vcf" > "$OUTDIR/isec.log" 2>&1
fi
if [ -n "$NOFILE" ]; then
  echo "No train.hdf written.  Train straight from the BAM with:"
  echo "  python $SCRIPTDIR/main.py --train_bam $BAM --train_fasta $REFERENCE --train_tp_vcf $OUTDIR/isec/0003.vcf" \
       "--train_tp_full_vcf $OUTDIR/isec/0002.vcf --train_fp_vcf $OUTDIR/isec/0001.vcf --train-loader-device gpu --train-cache-device gpu" \
       "[--train-cache-format compact]"${SUBFLAGS:+ "${SUBFLAGS[*]}"} \
       "( --test_file V.hdf | --test_bam Y.bam --test_fasta REF [--test_tp_vcf ... --test_tp_full_vcf ... --test_fp_vcf ...] )" \
       "<flags of train_variant_caller.sh>"
  exit 0
fi
if [ ! -f "$OUTDIR/train.hdf" ]; then
  printf "Convert candidates to HDF...\n"
  python "$SCRIPTDIR/tools/convert_bam_single_reads.py" --input "$BAM" --tp_vcf "$OUTDIR/isec/0003.vcf" \
      --tp_full_vcf "$OUTDIR/isec/0002.vcf" --fp_vcf "$OUTDIR/isec/0001.vcf" --fasta-input "$REFERENCE" \
      --output "$OUTDIR/train.hdf" --max-reads 200 --num-processes "$PROCS" --locations-process-step 100000 \
      --max-insert-length 10 --max-insert-length-variant 50 --save-q-scores --save-strand \
      ${COMPRESS:+--pileup-device gpu --compress-device "$COMPRESS"} \
      ${CODES:+--compress-codes "$CODES"} "${SUBFLAGS[@]}" > "$OUTDIR/training_data.log" 2>&1
fi
echo "Training data in $OUTDIR/train.hdf"
