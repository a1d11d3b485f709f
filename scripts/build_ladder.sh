#!/bin/bash
# Diagnostics: the stop-ladder builds (-DPG_STOP=k, bench-only instantiations), 8 compiles at a time.
#   LADDER_FLAGS="-DPG_DIAG" LADDER_PREFIX=dg_ scripts/build_ladder.sh 12 33 ...   -> libpindel_pg_dg_stop12.so ... (a second family)
cd "$(dirname "$0")/.." || exit 1
pts="${*:-1 10 11 12 33 34 13 37 14 15 16 17 18 19 20 21 22 35 36 23 24 25 26 27 28 29 30 31 32}"
export LADDER_FLAGS LADDER_PREFIX
printf '%s\n' plain $pts | xargs -P ${LADDER_JOBS:-8} -I{} bash -c 'if [ {} = plain ]; then bash scripts/build_variant.sh ${LADDER_PREFIX}plain -DPG_ONLY_BENCH $LADDER_FLAGS; else bash scripts/build_variant.sh ${LADDER_PREFIX}stop{} -DPG_ONLY_BENCH $LADDER_FLAGS -DPG_STOP={}; fi; echo built {} $?'
