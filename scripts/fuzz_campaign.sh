#!/bin/bash
# The round's randomised parity campaign on the GPU box: scripts/fuzz_campaign.sh <tag>  -> gpurun_out/<tag>/fuzz_log.txt
# (one summary line per seed range; a mismatch stops the range and is logged with its parameters)
# A second argument names the streams: "search" (the search kernels against the oracle), "classifier" (the device classifier against
# its host statements, fuzz_classifier.txt beside fuzz_log.txt) or both (the default: the classifier then runs only after seven
# bit-exact search ranges)
tag=${1:-fuzz}
streams=${2:-search classifier}
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/gpurun_out/$tag; mkdir -p "$out"
cd "$root" || exit 1
export PG_QUIET=1     # (no notes on stderr: a context whose length tables are not the fixed-length kernels' says so, once per context)
case " $streams " in *" search "*)
{
    echo "library: $(sha256sum pindel_amd/libpindel_pg.so | cut -c1-16)  kernels source: $(sha256sum pindel_amd/csrc/pg_kernels.hip | cut -c1-16)  $(date -u +%FT%TZ)"
    echo "== random parameters, lengths, references, window clusters (seeds < 200000: -x <= 4)"
    FUZZ_QUIET=1 timeout 900 python scripts/fuzz_parity.py ${N1:-400} 70000 2>&1 | grep -v amdgpu.ids | tail -3
    echo "== the wide stream (seeds >= 200000: -x <= 6, more insert sizes)"
    FUZZ_QUIET=1 timeout 900 python scripts/fuzz_parity.py ${N2:-600} 500000 2>&1 | grep -v amdgpu.ids | tail -3
    echo "== Pindel's default search parameters (seeds 300000-399999), each seed through the default-parameter AND the generic kernels"
    FUZZ_QUIET=1 FUZZ_BOTH_FAMILIES=1 timeout 1200 python scripts/fuzz_parity.py ${N3:-400} 310000 2>&1 | grep -v amdgpu.ids | tail -3
    echo "== characters outside ACGTN in one read in twelve (seeds >= 600000): the exact kernel"
    FUZZ_QUIET=1 timeout 900 python scripts/fuzz_parity.py ${N4:-300} 600000 2>&1 | grep -v amdgpu.ids | tail -3
    echo "== every launch packing in place (PG_PACK_IN_PLACE_MIN=1: the chunks of the host path, any size), seeds of the first and the fourth stream"
    PG_PACK_IN_PLACE_MIN=1 FUZZ_QUIET=1 timeout 900 python scripts/fuzz_parity.py ${N5:-200} 90000 2>&1 | grep -v amdgpu.ids | tail -3
    PG_PACK_IN_PLACE_MIN=1 FUZZ_QUIET=1 timeout 900 python scripts/fuzz_parity.py ${N5:-200} 620000 2>&1 | grep -v amdgpu.ids | tail -3
} | tee "$out/fuzz_log.txt"
[ "$(grep -c "iterations bit-exact" "$out/fuzz_log.txt")" = 7 ] || exit 1
esac
case " $streams " in *" classifier "*) ;; *) exit 0 ;; esac
# The device classifier against its host statements (scripts/fuzz_classifier.py), one range per stream, each under its own time limit
# and chained: a range that ends in a mismatch, a fault or its time limit starts nothing after it; a mismatch
# leaves its seed and drawn arguments beside the log (FUZZ_OUT)
export FUZZ_OUT="$out"
{
    echo "commit: ${COMMIT:-$(git rev-parse --short HEAD 2>/dev/null || echo unknown)}  library: $(sha256sum pindel_amd/libpindel_pg.so | cut -c1-16)  host library: $(sha256sum pindel_amd/libpindel_host.so | cut -c1-16)  $(date -u +%FT%TZ)"
    c() { FUZZ_QUIET=1 timeout -k 10 ${CT:-300} python scripts/fuzz_classifier.py "$1" "$2" 2>&1 | grep -v amdgpu.ids | tail -3; return "${PIPESTATUS[0]}"; }
    echo "== the device classifier: random parameters (seeds < 200000), the wide stream, Pindel's default parameters, two or three chromosomes, characters outside ACGTN" &&
    c ${C1:-60} 70000 && c ${C2:-60} 500000 && c ${C3:-60} 310000 && c ${C4:-60} 410000 && c ${C5:-60} 610000
    echo "exit status of the last range: $?"
} | tee "$out/fuzz_classifier.txt"
