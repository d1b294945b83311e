# same-box A/B of several builds of libdl4vc_dan.so on one bench command:  tools/lib_ab.sh "<bench args>" <rounds> <build> [<build> ...]
#   <build> = tree (the tree's library) or NAME for tools/ab/libdl4vc_dan_NAME.so, e.g. built from HEAD's sources with other flags:
#     git archive HEAD dl4vc_amd/csrc include | tar -x -C /tmp/b && make -C /tmp/b/dl4vc_amd/csrc libdl4vc_dan.so CXXFLAGS='...' && cp ... tools/ab/
#   every bench runs under its own time limit (BENCH_LIMIT seconds, default 600); the first failure ends the script
#   TIMING_ONLY="NAME ..." names builds that compute wrong numbers on purpose (a gate: the schedule of a change without its work):
#   for them alone a bench that ends by failing the parity check, which it does behind its result line, counts as run
set -e
PY=$(command -v python)
ERRLOG=$(mktemp)
python() {
  if [ "$1" != bench.py ]; then "$PY" "$@"; return; fi
  local rc=0
  timeout -k 10 ${BENCH_LIMIT:-600} "$PY" "$@" 2> "$ERRLOG" || rc=$?
  cat "$ERRLOG" >&2
  case " $TIMING_ONLY " in *" $v "*) if [ $rc -ne 0 ] && grep -q "failed the parity check" "$ERRLOG"; then rc=0; fi ;; esac
  return $rc
}
ARGS="${1:---precision 1 --sites 32768}"
N=${2:-2}
TAG=$(echo "$ARGS" | tr -c "a-zA-Z0-9" "_")
ARGS="--full $ARGS"          # the parity of the timed outputs printed below is checked under --full
shift 2 || true
BUILDS="${@:-base tree}"
for i in $(seq 1 $N); do
  for v in $BUILDS; do
    if [ $v = tree ]; then unset DL4VC_DAN_LIB; else export DL4VC_DAN_LIB=$PWD/tools/ab/libdl4vc_dan_$v.so; fi
    python bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-skip-pass --no-host-path $ARGS > gpurun_out/ab_${TAG}_${v}_$i.json 2> gpurun_out/ab_${TAG}_${v}_$i.err || { tail -5 gpurun_out/ab_${TAG}_${v}_$i.err; exit 1; }
    python - $v $i $TAG <<'PY'
import json,sys
d=json.loads(open('gpurun_out/ab_%s_%s_%s.json'%(sys.argv[3],sys.argv[1],sys.argv[2])).read().strip().splitlines()[-1]); r=d.get('roofline',{})
p=d.get('parity',{})
print('%-8s %s %10.1f ms/step %9.2f seg launch ms %s parity %s %s %s' % (sys.argv[1],sys.argv[2],d['value'],d['ms_per_step'],r.get('avg_launch_ms'),p.get('ok'),p.get('tiled_identical'),p.get('max_abs_vt_prob')))
PY
  done
done
