#!/bin/bash
# Statistics build of the blend kernels (-DTS2D_STATS) -> tools/bin/libts2d_stats.so: the lab library's objects with render_group
# recompiled with counters.  Used by tests/triage/blend_probe.py (TS2D_LIBRARY_PATH=tools/bin/libts2d_stats.so).
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
python $R/triangle-splatting_amd/build.py --lab > /dev/null
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -Wall -Wno-unused-function -Wno-unused-result -DNDEBUG -DTS2D_STATS -mllvm -amdgpu-atomic-optimizer-strategy=None -fno-slp-vectorize"
mkdir -p $R/tools/bin /tmp/ts2d_stats
C=$R/triangle-splatting_amd/csrc
/opt/rocm/bin/hipcc $F -DTSG_PART=1 -c $C/render_group.hip -o /tmp/ts2d_stats/render_group_fwd.o &   # (two translation units since round 6)
/opt/rocm/bin/hipcc $F -DTSG_PART=2 -c $C/render_group.hip -o /tmp/ts2d_stats/render_group_bwd.o &
wait
# exactly the objects build.py links into the lab library, not whatever else an old build left in its object directory
OBJS=""
for o in $(cd $R/triangle-splatting_amd && python -c "import build; print(*build.objects(lab=True))"); do
  case $(basename $o) in render_group_fwd.o|render_group_bwd.o) o=/tmp/ts2d_stats/$(basename $o);; esac
  OBJS="$OBJS $o"
done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o $R/tools/bin/libts2d_stats.so $OBJS
echo $R/tools/bin/libts2d_stats.so
