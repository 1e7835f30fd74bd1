#!/bin/bash
# A/B of two builds of the library on the receive chain and the decoder's options WITH their flag on, fresh processes in alternation:
#   bash profiles/ab_chain.sh OUT.jsonl ROUNDS LIB_A LIB_B
# Per round and library: the chain leg of the benchmark, measure_list.py (11 dB input, list on), measure_soft.py (soft on) and
# measure_biterr.py (hard route, counts on); one JSON line per process.  Whichever library runs first in a round tends to come out
# a few hundredths of a millisecond faster (profiles/r17/README.md): run it twice, once in either order.
# Every process runs under its own time limit and the script ends at the first one that fails.
set -o pipefail
OUT=$1; ROUNDS=$2; shift 2
: > "$OUT"
step() {   # step LABEL LIB command...
    local label=$1 lib=$2 line; shift 2
    line=$(TETRA_DEMOD_LIB=$lib timeout -k 10 170 "$@" 2>/dev/null | grep '^{' | tail -1)
    if [ $? -ne 0 ] || [ -z "$line" ]; then echo "FAILED: $label $lib"; exit 1; fi
    echo "{\"what\": \"$label\", \"lib\": \"$(basename "$(dirname "$lib")")\", \"result\": $line}" >> "$OUT"
}
for round in $(seq "$ROUNDS"); do
    for lib in "$@"; do
        lib=$(realpath "$lib")
        step bench_chain "$lib" python bench.py --gpus 1 --steps 10 --warmup 3 --chain-only
        step list_on_11dB "$lib" python profiles/measure_list.py --child 11 --reps 5
        step soft_on "$lib" python profiles/measure_soft.py --child 1 --reps 5
        step biterr_on_hard "$lib" python profiles/measure_biterr.py --child 01 --reps 5
    done
done
