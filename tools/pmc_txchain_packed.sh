#!/bin/bash
# Read traffic of the chain finalize over CSR descriptors (rns_tx_fill_chain_dev) and over the
# compact descriptors (rns_tx_fill_chain_packed_dev) on one config, same process, same arena:
# one rocprofv3 --pmc pass (FETCH_SIZE; counters only, no tracing) over tools/bench_ops.py with
# the one-fragment payload layout.  The two entries are two instantiations of csum_txrows_kernel,
# so pmc_write.py lists them apart.  Summarise with
#   python tools/pmc_write.py <outdir> --out profiles/<name>.json
# Usage: bash tools/pmc_txchain_packed.sh <outdir> <config>
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$ROOT/rocprof_out/pmctcp}; CFG=${2:-c5_imix}
mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd); export TMPDIR=/tmp; cd /tmp
timeout -s KILL 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/tx_chain_p0" -o run -- \
  python3 "$ROOT/tools/bench_ops.py" --ops tx_chain,tx_chain_packed --configs $CFG --tx-frags 0 --steps 3 \
  --rounds 1 > "$OUT/tx_chain_p0.log" 2>&1
rc=$?; echo "tx_chain + tx_chain_packed FETCH_SIZE pass rc=$rc"; exit $rc
