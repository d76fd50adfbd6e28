#!/bin/bash
# The -m gpu suite once per A/B switch (every fallback path is kept green); one line per switch.
# PART=a|b runs one half, PART=c the switches in $SWITCHES.  Every name must be a flag of the switch table
# (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_switches.h).  Lines go to $SWEEP_OUT (default
# switch_sweep_<part>.txt); a run that times out, aborts or faults (exit 124, 134, 137, 139) ends the sweep.
ALL_A="IPD_NO_BPOLY IPD_NO_BLKDENSE IPD_NO_BLK IPD_NO_POLY IPD_NO_MIS_SMALL IPD_NO_SUBCYCLE"
ALL_B="IPD_NO_RESIDENT_REMOTE IPD_NO_RESIDENT_THREE IPD_NO_PAD IPD_NO_DONOR IPD_NO_STEP_DONOR IPD_NO_RESIDENT IPD_NO_RESIDENT_BIG IPD_NO_RESIDENT_DEEP IPD_NO_RES_POLY4"
case "${PART:-ab}" in a) LIST="$ALL_A";; b) LIST="$ALL_B";; c) LIST="$SWITCHES";; *) LIST="$ALL_A $ALL_B";; esac
TABLE="$(dirname "$0")/../codes_of_ipd_ssn_amg_method_amd/csrc/ipd_switches.h"
for sw in $LIST; do
  grep -q "{\"$sw\", SW_FLAG," "$TABLE" || { echo "$sw is not a flag of $TABLE"; exit 2; }
done
OUT=${SWEEP_OUT:-switch_sweep_${PART:-ab}.txt}
LOG=$(mktemp)
trap 'rm -f "$LOG"' EXIT
: > "$OUT"
for sw in $LIST; do
  env $sw=1 timeout -k 10 400 python -m pytest tests -m gpu -q > "$LOG" 2>&1
  rc=$?
  res=$(tail -1 "$LOG")
  fails=$(grep "^FAILED" "$LOG" | cut -c1-150 | tr '\n' ';')
  echo "$sw=1: $res $fails" >> "$OUT"
  case $rc in
    124|134|137|139) echo "$sw=1: exit $rc, sweep stopped" >> "$OUT"; echo "$sw: exit $rc, sweep stopped"; exit $rc;;
  esac
  echo "$sw done"
done
