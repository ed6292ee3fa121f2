#!/bin/bash
# Attribution builds of conv_wr.hip (each deletes one ingredient of the phase; results are wrong, timings are the point):
# libhdf_hip_wr_<tag>.so = the product objects with conv_wr.o rebuilt under -DWR_DBG_<tag>.  Then tools/wr_attrib.sh on the GPU box.
# (There is no NOSTORE build any more: its switch sat in an epilogue branch the routed form never compiled -- whole tiles
# leave through the deferred pieces --, so it measured the product kernel.)
cd "$(dirname "$0")/../h-denseformer_amd"
python build.py > /dev/null
VARS=${VARS:-"NOSTAGE NOMFMA STAMPS"}
for v in $VARS; do
  mkdir -p build/wr_$v
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize -mllvm -amdgpu-mfma-vgpr-form -mllvm -pragma-unroll-threshold=1000000 -DWR_DBG_$v -c csrc/conv_wr.hip -o build/wr_$v/conv_wr.o &
done
wait
# every product object except conv_wr.o (the list follows build.py's SOURCES: a source added there is linked here too)
objs=$(python -c "import build; print(' '.join('build/' + s[:-4] + '.o' for s in build.SOURCES if s != 'conv_wr.hip'))")
for v in $VARS; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o lib/libhdf_hip_wr_$v.so $objs build/wr_$v/conv_wr.o
done
ls -la lib/
