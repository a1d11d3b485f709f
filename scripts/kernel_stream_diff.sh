#!/bin/bash
# Diagnostics: two builds of the library side by side (profiles/table_prims/README.md): scripts/resources.sh of both, and the
# instruction streams (addresses, encodings and the padding behind s_endpgm dropped) of the table kernels of the device classifier,
# kernel by kernel, over every code object of the library.  No GPU needed.
#   scripts/kernel_stream_diff.sh parent/libpindel_pg.so branch/libpindel_pg.so outdir
set -e
here=$(dirname "$(readlink -f "$0")")
P=$(readlink -f "$1"); B=$(readlink -f "$2"); mkdir -p "$3"; out=$(readlink -f "$3")
bash "$here/resources.sh" "$P" > "$out/resources_parent.txt"
bash "$here/resources.sh" "$B" > "$out/resources_branch.txt"
ex() { # lib dir
    mkdir -p "$2"; cp "$1" "$2/lib.so"; (cd "$2" && /opt/rocm/lib/llvm/bin/llvm-objdump --offloading lib.so > /dev/null 2>&1
    for co in lib.so.*gfx950*; do /opt/rocm/lib/llvm/bin/llvm-objdump -d "$co"; done > all.s)
}
ex "$P" "$out/p"; ex "$B" "$out/b"
sym() { # all.s symbol -> instruction stream without addresses / encodings
    awk -v s="<$2>:" '/^[0-9a-f]+ <.*>:$/ {p = ($2 == s)} p' "$1" | sed -e 's,//.*$,,' -e 's/[ \t]*$//' | grep -v '^[0-9a-f]* <' | grep '^	' | awk '{a[NR] = $0} /s_endpgm/ {last = NR} END {for (i = 1; i <= last; i++) print a[i]}' || true
}
cmpk() { # parent symbol, branch symbol: the streams stay in outdir/p and outdir/b
    sym "$out/p/all.s" "$1" > "$out/p/$1.s"; sym "$out/b/all.s" "$2" > "$out/b/$2.s"
    np=$(wc -l < "$out/p/$1.s"); nb=$(wc -l < "$out/b/$2.s")
    if diff -q "$out/p/$1.s" "$out/b/$2.s" > /dev/null; then echo "$1 -> $2: identical ($np instructions)"; else
        echo "$1 -> $2: DIFFER ($np vs $nb instructions, $(diff "$out/p/$1.s" "$out/b/$2.s" | grep -c '^[<>]') differing lines)"; fi
}
for f in events sv_events li; do for k in digit_count scatter compact; do cmpk pg_${f}_${k}_kernel pg_${f}_${k}_kernel; done; done
cmpk pg_events_rank_kernel pg_table_rank_kernel
cmpk pg_events_scan_kernel pg_table_scan_kernel
cmpk pg_li_flag_kernel pg_li_flag_kernel
cmpk pg_events_cascade_kernel pg_events_cascade_kernel
cmpk pg_sv_events_gather_kernel pg_sv_events_gather_kernel
cmpk pg_events_event_kernel pg_events_event_kernel
cmpk pg_sv_events_event_kernel pg_sv_events_event_kernel
cmpk pg_sv_events_run_kernel pg_sv_events_run_kernel
