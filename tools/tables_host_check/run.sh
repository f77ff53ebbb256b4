#!/bin/bash
# Build tables_host_check and the host unit it calls (lwhip_tables.hip) with AddressSanitizer and UBSan and run it.  The rest of
# the library comes from the built liblwhip.so (python -m lightweaver_amd.build), unsanitized.  For a machine WITHOUT a GPU:
# the program calls no HIP function.  Usage: tools/tables_host_check/run.sh
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
root=$(cd "$here/../.." && pwd)
out=${TMPDIR:-/tmp}/tables_host_check.$$
mkdir -p "$out"
trap 'rm -rf "$out"' EXIT
hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -x hip "$root/lightweaver_amd/csrc/lwhip_tables.hip" "$here/main.cpp" \
    -L"$root/lightweaver_amd" -llwhip -Wl,-rpath,"$root/lightweaver_amd" -o "$out/tables_host_check"
"$out/tables_host_check"
