#!/bin/bash
# tools/pool_driver_check.sh — the pool driver behind canned lanes under AddressSanitizer + UBSan: a stand-alone host
# program (tools/pool_driver_check.cpp), no device needed and none used.
set -euo pipefail
cd "$(dirname "$0")/.."
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=${OUT:-$(mktemp -d)/pool_driver_check}
"$HIPCC" --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
  -Iinclude -Ihighs_amd/csrc tools/pool_driver_check.cpp highs_amd/csrc/pdlp_pool.cpp -fsanitize=address,undefined -o "$OUT"
"$OUT"
