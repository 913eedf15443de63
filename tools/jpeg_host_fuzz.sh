#!/bin/bash
# ASan + UBSan over the JPEG host front end (all five host entry points), on the CPU: unpacks the files of
# tests/golden/jpeg_goldens.npz and tests/golden/jpeg_progressive_goldens.npz (damaged ones included), builds
# tools/jpeg_host_fuzz.cpp with csrc/jpeg_host.hip as plain C++ (no HIP, no Python, nothing preloaded) and runs it.
# Usage: tools/jpeg_host_fuzz.sh [log file]
set -e -o pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
log=${1:-$root/profiles/jpeg_host_sanitizers.txt}
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
cxx=${CXX:-$(ls /opt/rocm/lib/llvm/bin/clang++ 2>/dev/null || command -v clang++ || command -v g++)}
flags="-O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
python - "$root" "$work" <<'PY'
import sys, numpy as np
root, work = sys.argv[1:]
for archive, prefix in (("jpeg_goldens", "baseline_"), ("jpeg_progressive_goldens", "")):       # (a name may be in both)
    with np.load(f"{root}/tests/golden/{archive}.npz") as z:
        for n in z["names"]:
            open(f"{work}/{prefix}{n}.jpg", "wb").write(z[f"{n}/jpeg"].tobytes())
with np.load(root + "/tests/golden/jpeg_progressive_goldens.npz") as z:
    for n in z["damaged"]:
        open(f"{work}/damaged_{n}.bin", "wb").write(z[f"damaged/{n}"].tobytes())
PY
$cxx $flags -x c++ "$root/multiposenet_amd/csrc/jpeg_host.hip" "$root/tools/jpeg_host_fuzz.cpp" -o "$work/jpeg_host_fuzz"
first="$work/37x53_p420_rst3.jpg $work/17x17_pcmyk_rst2_opt.jpg $work/37x53_cmyk_opt_rst.jpg"
rest=$(ls "$work"/*.jpg | grep -v -e /37x53_p420_rst3.jpg -e /17x17_pcmyk_rst2_opt.jpg -e /37x53_cmyk_opt_rst.jpg)
{
  echo "# ASan + UBSan over the JPEG host front end, five entry points (tools/jpeg_host_fuzz.sh), $(date -u +%Y-%m-%dT%H:%MZ), on the CPU:"
  echo "# $(basename $cxx) $flags -x c++ multiposenet_amd/csrc/jpeg_host.hip tools/jpeg_host_fuzz.cpp"
  echo "# jpeg_host_fuzz <the $(ls "$work"/*.jpg | wc -l) golden files and the $(ls "$work"/damaged_*.bin | wc -l) damaged ones; every prefix of 37x53_p420_rst3, 17x17_pcmyk_rst2_opt, 37x53_cmyk_opt_rst>"
  rc=0
  ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
    "$work/jpeg_host_fuzz" $first $rest "$work"/damaged_*.bin 2>&1 || rc=$?
  echo "# exit status $rc"
} | tee "$log"
