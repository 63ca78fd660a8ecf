#!/bin/bash
# Build variants of the library (one per name, into tools/build/) and time the config-5 sweeps of each with a one-handle stream
# (kernel durations = HIP events, nothing else on the GPU).  Every variant computes valid results:
#   BASE                       the default build
#   RSH<k>                     path retirement evaluated every 2^k records instead of 256 (RSH4 makes the small graphs of the tests
#                              and of tools/fuzz_parity.py retire paths)
#   RETSTAT                    statistics build for tools/probes/retire_stat.py
#   STALLSTAT, STALL2, STALL3  statistics builds for tools/probes/stall_stat.py (levels 1, 2, 3)
#   BANDLOOPS                  the band of the POA kernels as the reference's three loops (tests/test_band_check.py)
# Names are joined with _ (RSH4_RETSTAT).  The timing-only builds of rounds 2-6 (profiles/r0*_sweep_variants_*.txt) were taken out
# with their switches; they can be rebuilt from the history of this file and of rg_sweep16.hip.
#   without a GPU:   tools/sweep_variants.sh build
#   on the GPU box:  tools/sweep_variants.sh run > gpurun_out/sweep_variants.txt
cd "$(dirname "$0")/.." || exit 1
VARIANTS="${VARIANTS:-BASE RSH4}"
if [ "$1" = build ]; then
  mkdir -p tools/build
  for v in $VARIANTS; do
    flags=""; [ $v != BASE ] && for f in ${v//_/ }; do
      case $f in
        RSH[0-9]*) flags="$flags -DRG_SWEEP16_RETIRE_SHIFT=${f#RSH}";;
        RETSTAT) flags="$flags -DRG_SWEEP16_RETSTAT";;
        STALLSTAT) flags="$flags -DRG_SWEEP16_STALLSTAT";;
        STALL2) flags="$flags -DRG_SWEEP16_STALLSTAT=2";;
        STALL3) flags="$flags -DRG_SWEEP16_STALLSTAT=3";;
        BANDLOOPS) flags="$flags -DRG_BAND_SIMD_LOOPS";;
        *) echo "unknown variant '$f' in '$v'" >&2; exit 1;;
      esac; done
    rm -rf /tmp/rgvar_$v; mkdir -p /tmp/rgvar_$v
    cp -r recgraph_amd/csrc /tmp/rgvar_$v/csrc; mkdir -p /tmp/rgvar_$v/include; cp include/recgraph_hip.h /tmp/rgvar_$v/include/
    mkdir -p /tmp/rgvar_$v/x; mv /tmp/rgvar_$v/csrc /tmp/rgvar_$v/x/csrc; mkdir -p /tmp/rgvar_$v/include
    ( cd /tmp/rgvar_$v/x/csrc && rm -rf build && make -j16 CXXFLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wno-unused-function $flags" > /dev/null 2>&1 ) || { echo "build $v failed"; exit 1; }
    cp /tmp/rgvar_$v/x/librecgraph_hip.so tools/build/librecgraph_hip_$v.so
    echo "built $v ($flags)"
  done
  exit 0
fi
# (RG_NO_SPEC=1: every read takes the sweeps without the speculative bound; SPEC=1 keeps the speculative bound)
for v in $VARIANTS; do
  RG_NO_SPEC=$([ "$SPEC" = 1 ] && echo 0 || echo 1) RG_LIB_PATH=$PWD/tools/build/librecgraph_hip_$v.so python3 bench.py --config ${CFG:-C5} --steps 4 --warmup 1 --no-cpu --no-strong --no-probe --handles 1 2>/dev/null |
    python3 -c "import sys,json; d=json.loads(sys.stdin.read()); k=d['kernel_ms_per_step']; print('$v', 'fwd', k.get('k_sweep16_fwd'), 'rev', k.get('k_sweep16_rev'), 'step', d['ms_per_step'])"
done
