#!/bin/bash
# tools/round_plan_check.sh — the schedule of a device-driven round (highs_amd/csrc/pdlp_round.hpp) against the reference's
# under AddressSanitizer + UBSan: a stand-alone host program (tools/round_plan_check.cpp), no device needed and none used.
set -euo pipefail
cd "$(dirname "$0")/.."
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=${OUT:-$(mktemp -d)/round_plan_check}
"$HIPCC" --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
  -Iinclude -Ihighs_amd/csrc tools/round_plan_check.cpp -fsanitize=address,undefined -o "$OUT"
"$OUT"
