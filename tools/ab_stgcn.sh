# Same-box A/B of builds of the library under the recogniser bench: tools/ab_stgcn.sh NAME_A NAME_B ... [-- bench flags] (build/lib_NAME.so), three
# alternating rounds, ms per forward (T = 60, T = 150). Every bench runs under its own time limit (BENCH_TIMEOUT seconds, default 300); the first run that
# fails or times out ends the script with its exit status - nothing more is started on the GPU - and the displaced library comes back on every exit path.
set -u
export TMPDIR=/tmp
NAMES=(); while [ $# -gt 0 ] && [ "$1" != "--" ]; do NAMES+=("$1"); shift; done
[ $# -gt 0 ] && shift
KEEP=$(mktemp /tmp/lib_keep.XXXXXX) && ERR=$(mktemp /tmp/ab_err.XXXXXX) && cp regennet_amd/libregennet_hip.so "$KEEP" || exit 1
trap 'cp "$KEEP" regennet_amd/libregennet_hip.so; rm -f "$KEEP" "$ERR"' EXIT
for r in 1 2 3; do
  for L in "${NAMES[@]}"; do
    cp build/lib_$L.so regennet_amd/libregennet_hip.so || exit 1
    out=$(timeout -k 10 "${BENCH_TIMEOUT:-300}" python bench.py --config stgcn --steps 10 --warmup 2 "$@" 2>"$ERR"); st=$?
    if [ $st -ne 0 ]; then echo "  $L: bench ended with status $st, stopping" >&2; tail -n 5 "$ERR" >&2; exit $st; fi
    printf '%s\n' "$out" | python -c "import sys, json; d = json.loads(sys.stdin.readline()); print('  $L', [p['ms_per_forward'] for p in d['per_length']])" || exit 1
  done
done
