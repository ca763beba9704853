#!/bin/bash
# Build libwgrt.so of a git revision (its csrc/ and include/) into exp_libs/NAME/ for tools/ab.py,
# with the tree's compile flags (_build.FLAGS) and the revision's own source list (its csrc/*.hip and
# wgrt_scene_build.cpp: units are added and renamed between revisions).
#   tools/ab_build_rev.sh NAME REV [-Dmacro ...]
set -e
cd "$(dirname "$0")/.."
name=$1 rev=$2; shift 2
src=$(mktemp -d)
pkg=gpu_ray_tracing_for_waveguide_based_ar_display_amd
git archive "$rev" include "$pkg/csrc" | tar -x -C "$src"
mkdir -p exp_libs/$name
python3 - "$src" "exp_libs/$name/libwgrt.so" "$@" <<'PY'
import glob, os, subprocess, sys
sys.path.insert(0, os.getcwd())
from gpu_ray_tracing_for_waveguide_based_ar_display_amd import _build
src, out, defs = sys.argv[1], sys.argv[2], sys.argv[3:]
csrc = os.path.join(src, "gpu_ray_tracing_for_waveguide_based_ar_display_amd", "csrc")
cmd = [_build._hipcc(), *_build.FLAGS, *defs, "-I", os.path.join(src, "include"), "-o", out] + \
      sorted(glob.glob(os.path.join(csrc, "*.hip"))) + [os.path.join(csrc, "wgrt_scene_build.cpp")]
r = subprocess.run(cmd, capture_output=True, text=True)
sys.exit(r.stderr if r.returncode else 0)
PY
rm -rf "$src"
echo "$name exp_libs/$name/libwgrt.so ($rev)"
