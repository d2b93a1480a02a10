# Same-box A/B of two whole TREES of this repository (library + host code): tools/ab_trees.sh rounds treeA treeB -- bench flags
# (ab_many.sh swaps builds of the library under ONE host tree; across rounds the C-ABI grew, so an older library needs its own host code.)
# A tree is a directory holding bench.py and a built regennet_amd/libregennet_hip.so, e.g. `git archive <commit> | tar -x -C build/r4_tree`
# + `python __graft_entry__.py` inside it. Every bench runs under its own time limit (BENCH_TIMEOUT seconds, default 600); the first run that fails or
# times out ends the script with its exit status: nothing more is started on the GPU.
set -u
N=$1; shift
TREES=(); while [ $# -gt 0 ] && [ "$1" != "--" ]; do TREES+=("$1"); shift; done
[ $# -gt 0 ] && shift
ERR=$(mktemp /tmp/ab_err.XXXXXX) || exit 1
trap 'rm -f "$ERR"' EXIT
for r in $(seq $N); do
  for T in "${TREES[@]}"; do
    out=$(cd $T && timeout -k 10 "${BENCH_TIMEOUT:-600}" python bench.py --no-cpu-baseline --profile-evals 0 "$@" 2>"$ERR"); st=$?
    if [ $st -ne 0 ]; then echo "$T: bench ended with status $st, stopping" >&2; tail -n 5 "$ERR" >&2; exit $st; fi
    v=$(printf '%s\n' "$out" | python -c "import sys, json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['value'], d['ms_per_step'])") || exit 1
    echo "$T $v"
  done
done
