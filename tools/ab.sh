#!/bin/bash
# A/B of two builds on the SAME GPU box (boxes differ by a few percent, so timings of separate runs cannot resolve
# 1-2 % effects).  Without a GPU: tools/ab.sh build  -> A = git HEAD, the whole tree (its Python binds its own library's
# symbols: a working tree that adds exports cannot load HEAD's library) with its library built, in ab_libs/A; B = the
# working tree, built in place.  On the box: tools/ab.sh run [reps] -> alternates A's bench.py and B's.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
if [ "$1" = "build" ]; then
    rm -rf ab_libs/A && mkdir -p ab_libs/A
    git archive HEAD warpdemux_amd include bench.py | tar -x -C ab_libs/A   # (--no-cpu: the CPU oracle is never imported)
    make -C ab_libs/A/warpdemux_amd/csrc -j4 -s 2>&1 | grep -E "error" || true
    make -C warpdemux_amd/csrc -j4 -s 2>&1 | grep -E "error" || true
    ls -la ab_libs/A/warpdemux_amd/csrc/libwdx_hip.so warpdemux_amd/csrc/libwdx_hip.so
else
    REPS=${2:-2}
    for r in $(seq $REPS); do
        for v in A B; do
            if [ $v = A ]; then BENCH=$ROOT/ab_libs/A/bench.py; else BENCH=$ROOT/bench.py; fi
            timeout -k 10 150 python3 $BENCH --full --steps 5 --warmup 1 --no-cpu --no-secondary 2>/dev/null | tail -1 |
                python3 -c "import sys,json; j=json.loads(sys.stdin.read()); k=j['kernels_ms_per_step']; print('$v', round(j['value']/1e6,3), 'M reads/s  fp', round(k['fingerprint'],2), 'dtw', round(k['dtw'],2))"
        done
    done
fi
