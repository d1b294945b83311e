#!/bin/bash
# Drop-in for the reference's call_variants.sh from the candidate VCF on (call_variants.sh:85-168): candidates.vcf + BAM ->
# candidates.hdf (tools/convert_bam_single_reads.py here: own BAM / FASTA readers, no pysam), scoring with the MI355X-native DAN
# forward, then sort, genotype thresholds, multi-allele join and bgzip/tabix (with bcftools/htslib when installed, else in
# process: dl4vc_amd/vcfpost.py).  The first stage -- BAM -> candidates.vcf (tools/candidate_generator.py, reference
# call_variants.sh:76-83) -- runs when OUTDIR holds neither candidates.hdf nor candidates.vcf and -i is given: per-read allele
# detection and per-locus counting on the GPU (libdl4vc_cand.so), with the reference's flags; -b restricts it to a BED file
# (the reference requires -b; here it is optional and its absence means the whole BAM).  An existing candidates.vcf is used
# as it is.  With an OUTDIR that also holds candidates.hdf, -i / -r are not needed and the conversion is skipped.
# -d (direct; needs -i and -r): no candidates.hdf at all -- main.py --test_bam encodes the pileups on the GPU, assembles
# and scores them there.  The scored VCF is byte-identical to the two-step path's.  Without -d nothing changes.
# -d with -g N, N > 1: the candidate generator runs one process per GPU (--gpus N) and main.py counts the records first
# (--record-census gpu), so that its N shards seed their read subsets as one process does; both outputs are the same bytes.
# -z: the candidate generator inflates the BAM's BGZF blocks and frames its records on the GPU (--inflate-device gpu; needs
# BAM.bai); candidates.vcf is the same.  With -d, main.py --test_bam gets --inflate-device gpu as well, so no stage inflates or
# frames a record on the host; the scored VCF is the same.
# -c (on the path through candidates.hdf, no effect with -d): the converter builds the pileups on the GPU and packs and compresses
# the file's chunks there as well (--pileup-device gpu --compress-device gpu); candidates.hdf holds the same records, the scored
# VCF is the same.
# -y (with -c): the compressed chunks get dynamic Huffman codes where they are smaller (--compress-codes dynamic): a smaller
# candidates.hdf with the same records.
# -l (on the path through candidates.hdf; an error with -d): main.py inflates the file's chunks and assembles its sites on the GPU
# (--loader-device gpu); the scored VCF is the same.
# -f (needs -r): the candidate generator walks the reads that have no MD tag against REFERENCE (--reference; whole contigs on the
# GPU, 1 byte per base) instead of giving them no alleles; reads with an MD tag are walked by it as before.  Not passed by
# default: without -f candidates.vcf is what it was.
# -L (needs -r; implies -f): the candidate generator moves every insertion and deletion to its left-most placement on REFERENCE
# before it is counted (--left-align), so that the placements of one event inside a repeat give one candidate.  Reads are not
# realigned: the pileups show them as they are aligned.  Not passed by default.
# -s F [-S SEED] (needs -i): every stage that reads the BAM keeps the fraction F in (0, 1] of its reads, chosen by a hash of the
# read name as `samtools view --subsample F --subsample-seed SEED` chooses them (--subsample / --subsample-seed): candidate
# generation and the pileup step (the converter, or main.py --test_bam with -d) see the same reads, so the calls are those of the
# BAM tools/subsample_bam.py writes -- the run at F of the coverage.  A candidates.vcf or candidates.hdf already in OUTDIR is used
# as it is: give a fresh OUTDIR per fraction.
# -q Q, -F MASK, -R MASK (need -i): every stage that reads the BAM drops the reads with MAPQ < Q, with any flag bit of -F or
# without a flag bit of -R (--min-mapq / --exclude-flags / --require-flags; the masks decimal or 0x..., as samtools view -q -F
# -f): candidate generation and the pileup step are filtered alike, e.g. -q 20 -F 0x704 counts the candidates over the reads the
# pileup shows.  As with -s, give a fresh OUTDIR per filter.
set -e
usage() { echo "Usage: $0 -m MODEL -o OUTDIR [-i BAM -r REFERENCE] [-b BED] [-g GPUS] [-p PROCESSES] [-d] [-z] [-f] [-L] [-c [-y]] [-l] [-s FRACTION [-S SEED]] [-q MIN_MAPQ] [-F EXCLUDE_FLAGS] [-R REQUIRE_FLAGS]"; exit 1; }
GPUS=1
PROCS=16
DIRECT=0
INFLATE=""
COMPRESS=""
CODES=""
LOADER=""
FROMREF=""
LEFTALIGN=""
SUBSAMPLE=""
SEED=""
MINMAPQ=""
EXCLUDE=""
REQUIRE=""
while getopts "m:o:g:i:r:b:p:s:S:q:F:R:fLldzcyh" opt; do
  case $opt in
    m) MODEL=$OPTARG ;;
    o) OUTDIR=$OPTARG ;;
    g) GPUS=$OPTARG ;;
    i) BAM=$OPTARG ;;
    r) REFERENCE=$OPTARG ;;
    b) BED=$OPTARG ;;       # candidate generation only
    p) PROCS=$OPTARG ;;
    d) DIRECT=1 ;;          # score straight from the BAM (main.py --test_bam)
    z) INFLATE=gpu ;;       # BGZF inflate and record framing on the GPU: candidate generation, and with -d the pileup encoder
    c) COMPRESS=gpu ;;      # candidates.hdf: pileups, record packing and chunk compression on the GPU
    y) CODES=dynamic ;;     # with -c: dynamic Huffman codes in the compressed chunks
    f) FROMREF=1 ;;         # candidate generation: reads without MD are walked against REFERENCE
    L) LEFTALIGN=1; FROMREF=1 ;;  # candidate generation: indels are left-aligned on REFERENCE before they are counted
    s) SUBSAMPLE=$OPTARG ;; # every BAM reader keeps this fraction of the reads (--subsample)
    S) SEED=$OPTARG ;;      # with -s: the seed (--subsample-seed)
    q) MINMAPQ=$OPTARG ;;   # every BAM reader drops the reads below this mapping quality (--min-mapq)
    F) EXCLUDE=$OPTARG ;;   # ... and the reads with any of these flag bits (--exclude-flags)
    R) REQUIRE=$OPTARG ;;   # ... and the reads without any of these flag bits (--require-flags)
    l) LOADER=gpu ;;        # candidates.hdf is inflated and its sites assembled on the GPU (main.py --loader-device gpu)
    *) usage ;;
  esac
done
[ -z "$MODEL" ] || [ -z "$OUTDIR" ] && usage
[ -n "$CODES" ] && [ -z "$COMPRESS" ] && { echo "-y chooses the codes of the chunks -c compresses: give -c as well"; exit 1; }
[ -n "$LOADER" ] && [ "$DIRECT" = 1 ] && { echo "-l loads candidates.hdf on the GPU and -d reads no candidates.hdf: give one of them"; exit 1; }
[ -n "$LEFTALIGN" ] && [ -z "$REFERENCE" ] && { echo "-L left-aligns the indels on the reference: give -r REFERENCE as well"; exit 1; }
[ -n "$FROMREF" ] && [ -z "$REFERENCE" ] && { echo "-f walks the reads without MD against the reference: give -r REFERENCE as well"; exit 1; }
[ -n "$SEED" ] && [ -z "$SUBSAMPLE" ] && { echo "-S is the seed of -s: give -s FRACTION as well"; exit 1; }
[ -n "$SUBSAMPLE" ] && [ -z "$BAM" ] && { echo "-s thins the reads of the BAM: give -i BAM as well (a candidates.hdf holds pileups already encoded)"; exit 1; }
[ -n "$MINMAPQ$EXCLUDE$REQUIRE" ] && [ -z "$BAM" ] && { echo "-q / -F / -R filter the reads of the BAM: give -i BAM as well (a candidates.hdf holds pileups already encoded)"; exit 1; }
SUBFLAGS=(${SUBSAMPLE:+--subsample "$SUBSAMPLE"} ${SEED:+--subsample-seed "$SEED"} ${MINMAPQ:+--min-mapq "$MINMAPQ"} \
          ${EXCLUDE:+--exclude-flags "$EXCLUDE"} ${REQUIRE:+--require-flags "$REQUIRE"})
MULTI=""
[ "$DIRECT" = 1 ] && [ "$GPUS" -gt 1 ] && MULTI=1
SCRIPTDIR="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
if [ ! -f "$OUTDIR/candidates.hdf" ] && [ ! -f "$OUTDIR/candidates.vcf" ] && [ -n "$BAM" ]; then
  mkdir -p "$OUTDIR"
  printf "Generate candidate VCF...\n"
  python "$SCRIPTDIR/tools/candidate_generator.py" --input "$BAM" --output "$OUTDIR/candidates.vcf" \
      --snp_min_freq 0.075 --indel_min_freq 0.02 ${BED:+--bedfile "$BED"} --keep_multialleles \
      ${INFLATE:+--inflate-device "$INFLATE"} ${MULTI:+--gpus "$GPUS"} ${FROMREF:+--reference "$REFERENCE"} \
      ${LEFTALIGN:+--left-align} "${SUBFLAGS[@]}" > "$OUTDIR/candidate_generator.log" 2>&1
fi
if [ "$DIRECT" = 1 ]; then
  [ -f "$OUTDIR/candidates.vcf" ] && [ -n "$BAM" ] && [ -n "$REFERENCE" ] || { echo "-d needs -i BAM -r REFERENCE (and $OUTDIR/candidates.vcf, made from the BAM when absent)"; exit 1; }
  TEST_INPUT=(--test_bam "$BAM" --test_fasta "$REFERENCE" ${INFLATE:+--inflate-device "$INFLATE"} ${MULTI:+--record-census gpu} "${SUBFLAGS[@]}")
else
  TEST_INPUT=(--test_file "$OUTDIR/candidates.hdf" ${LOADER:+--loader-device "$LOADER"})
fi
if [ "$DIRECT" != 1 ] && [ ! -f "$OUTDIR/candidates.hdf" ]; then
  [ -f "$OUTDIR/candidates.vcf" ] && [ -n "$BAM" ] && [ -n "$REFERENCE" ] || { echo "missing $OUTDIR/candidates.hdf (or candidates.vcf with -i BAM -r REFERENCE to make it)"; exit 1; }
  printf "Convert candidates to HDF...\n"
  python "$SCRIPTDIR/tools/convert_bam_single_reads.py" --input "$BAM" --fp_vcf "$OUTDIR/candidates.vcf" \
      --fasta-input "$REFERENCE" --output "$OUTDIR/candidates.hdf" --max-reads 200 --num-processes "$PROCS" \
      --locations-process-step 100000 --max-insert-length 10 --max-insert-length-variant 50 \
      --save-q-scores --save-strand ${COMPRESS:+--pileup-device gpu --compress-device "$COMPRESS"} \
      ${CODES:+--compress-codes "$CODES"} "${SUBFLAGS[@]}" > "$OUTDIR/training_data.log" 2>&1
fi

printf "Run inference...\n"
python "$SCRIPTDIR/main.py" \
    --model-hidden-dropout 0.1 --model-batchnorm --model-use-q-scores --model-use-strands \
    --model-use-reads-ref-var-mask --model-conv-layers 7 --model-residual-layer-start 5 \
    --model-ave-pool-layers 2 --model-init-conv-channels 128 --model-final-conv-channels 128 \
    --model_pool_combine_dimension 0 --model-bottleneck-size 32 --model_final_layer_dilation 2 \
    --model_middle_layer_dilation 2 --model_concat_hw_reads --model-highway-single-reads \
    --gpus "$GPUS" --test-batch-size 200 --save_vcf_records \
    --save_vcf_records_file "$OUTDIR/model_test.vcf" "${TEST_INPUT[@]}" \
    --sample_vcf "$OUTDIR/candidates.vcf" --modelload "$MODEL" > "$OUTDIR/training.log" 2>&1

printf "Sort output VCF...\n"
awk '$1 ~ /^#/ {print $0;next} {print $0 | "sort -k1,1 -k2,2n"}' "$OUTDIR/epoch1_model_test.vcf" > "$OUTDIR/model_test_sorted.vcf"

printf "Threshold and combine multi-allele...\n"
python "$SCRIPTDIR/tools/format_vcf.py" --input_file "$OUTDIR/model_test_sorted.vcf" \
    --output_file "$OUTDIR/model_test_sorted_thres.vcf" --snp_threshold 0.1 --indel_threshold 0.2 \
    --snp_zygo_threshold 0.75 --indel_zygo_threshold 0.8 > "$OUTDIR/format_vcf.log" 2>&1

if command -v bcftools >/dev/null 2>&1; then
  bcftools norm -m +any "$OUTDIR/model_test_sorted_thres.vcf" > "$OUTDIR/model_test_sorted_thres-join.vcf" 2> "$OUTDIR/bcftools_norm.log"
  sed -i 's/0\/2/1\/2/' "$OUTDIR/model_test_sorted_thres-join.vcf"
  sed -i 's/2\/2/1\/2/' "$OUTDIR/model_test_sorted_thres-join.vcf"
  bgzip -c "$OUTDIR/model_test_sorted_thres-join.vcf" > "$OUTDIR/called_variants.vcf.gz"
  tabix -p vcf "$OUTDIR/called_variants.vcf.gz"
  echo "Called variants in $OUTDIR/called_variants.vcf.gz"
else
  # no bcftools / bgzip / tabix on this machine: the in-process restatement of the same five commands
  python "$SCRIPTDIR/tools/finish_calls.py" --input_file "$OUTDIR/model_test_sorted_thres.vcf" \
      --joined_file "$OUTDIR/model_test_sorted_thres-join.vcf" --output_gz "$OUTDIR/called_variants.vcf.gz"
  echo "Called variants in $OUTDIR/called_variants.vcf.gz (joined and indexed in process: bcftools not found)"
fi
