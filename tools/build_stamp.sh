#!/bin/bash
# Diagnostic build of the library with in-kernel cycle stamps in nn.hip and train.hip (k_conv_t; train_net.hip shares the handle's layout) (-DDBAZ_STAMP), into build/stamp/ (not shipped,
# git-ignored; it travels to the GPU box with the snapshot).  Use with DBAZ_LIB=$PWD/build/stamp/libdbaz_hip.so.
# RING_P=2 tools/build_stamp.sh: the same with the two-slot weight ring alone (-DDBAZ_RING_P=2), into build/stamp_p2/.
# STAGGER=0 tools/build_stamp.sh: every step head behind its barrier (-DDBAZ_STAGGER=0; 2: waves 0-3 late), into build/stamp_s0/.
set -e
cd "$(dirname "$0")/.."
out=build/stamp${RING_P:+_p$RING_P}${STAGGER:+_s$STAGGER}
mkdir -p $out
python -m dotsboxesaz_amd.build > /dev/null
for f in engine nn train train_net; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -DDBAZ_STAMP ${RING_P:+-DDBAZ_RING_P=$RING_P} ${STAGGER:+-DDBAZ_STAGGER=$STAGGER} -c dotsboxesaz_amd/csrc/$f.hip -o $out/$f.o &
done
wait
c=dotsboxesaz_amd/csrc
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $out/libdbaz_hip.so $c/tree.o $out/engine.o $out/nn.o $c/replay.o $out/train.o $out/train_net.o $c/solver.o $c/endgame.o $c/buildinfo.o
echo $out/libdbaz_hip.so
