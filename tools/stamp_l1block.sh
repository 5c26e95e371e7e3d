# Stamps build of libsad: only l1block.o rebuilt, with the Makefile's own
# CXXFLAGS (NOPK included: the same device code as the library's) plus
# -DSAD_STAMPS=1; the other objects from the normal build (run make first).
#   bash tools/stamp_l1block.sh [OUT]      (default abl/libsad_l1stamps.so)
# Then, on the GPU:  SAD_LIB=OUT python tools/l1bench.py --n 256
# prints the per-tile phase cycles of waves 0 and 2 of workgroup 0 per launch,
# strip-start and continuation tiles apart.  Diagnostic only: never time it.
set -e
cd "$(dirname "$0")/.."
out=${1:-abl/libsad_l1stamps.so}
csrc=synthetic-audio-detection_amd/csrc
mkdir -p "$(dirname "$out")" build/csrc_stamps
flags=$(make -s --no-print-directory -C $csrc flags)
/opt/rocm/bin/hipcc $flags -DSAD_STAMPS=1 -c $csrc/l1block.hip -o build/csrc_stamps/l1block.o
objs=$(ls build/csrc/*.o | grep -v '/l1block\.o$')
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o "$out" $objs build/csrc_stamps/l1block.o
