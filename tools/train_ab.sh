# same-box A/B of builds of libdl4vc_dan.so on the training step:  tools/train_ab.sh [<rounds> [<build> <build> ...]]
#   <build> = tree (the tree's library) or NAME for tools/ab/libdl4vc_dan_NAME.so; default: 3 rounds of base, tree, alternating.
# bench.py --mode train at the default batch and at --train-batch 10, each run under its own time limit; the first failure ends
# the job.  Ends with each build's median and max - min ms/step per batch size: the yardstick for "unchanged" is the first build's
# own max - min.  The bench lines go to $TRAIN_AB_OUT (default: train_ab_out).
set -e
N=${1:-3}
shift || true
BUILDS="${@:-base tree}"
export OUT=${TRAIN_AB_OUT:-train_ab_out}
mkdir -p $OUT
run() {  # run <out prefix> <bench args...>
  local out=$1; shift
  timeout -k 10 240 python bench.py --mode train --no-cpu-baseline "$@" > $out.json 2> $out.err || { echo "FAILED ($?): $out"; tail -5 $out.err; exit 1; }
}
for i in $(seq 1 $N); do
for v in $BUILDS; do
  if [ $v = tree ]; then unset DL4VC_DAN_LIB; else export DL4VC_DAN_LIB=$PWD/tools/ab/libdl4vc_dan_$v.so; fi
  run $OUT/tab_${v}_$i --steps 10 --warmup 2
  run $OUT/tab10_${v}_$i --train-batch 10 --steps 20 --warmup 3
  python - $v $i <<'PY'
import json,os,sys
for pre in ('tab','tab10'):
    d=json.loads(open('%s/%s_%s_%s.json'%(os.environ['OUT'],pre,sys.argv[1],sys.argv[2])).read().strip().splitlines()[-1])
    print(pre,sys.argv[1],sys.argv[2],d['value'],'ms/step',d['ms_per_step'],'frac',d['roofline']['frac'])
PY
done
done
python - $N $BUILDS <<'PY'
import json,os,statistics,sys
n,builds=int(sys.argv[1]),sys.argv[2:]
for pre,name in (('tab','default batch'),('tab10','--train-batch 10')):
    for v in builds:
        ms=[json.loads(open('%s/%s_%s_%d.json'%(os.environ['OUT'],pre,v,i)).read().strip().splitlines()[-1])['ms_per_step'] for i in range(1,n+1)]
        print('%-16s %-8s ms/step %s median %.4f max-min %.4f' % (name,v,' / '.join('%.4f'%m for m in ms),statistics.median(ms),max(ms)-min(ms)))
PY
