#!/bin/bash
# Build libhpvpinn.so for gfx950 in-tree (hipcc cross-compiles without a GPU), every stale object in parallel.
#   ../libhpvpinn.so            the product
#   ../libhpvpinn_testhooks.so  the same sources with -DHPV_TEST_HOOKS: the fault-injection knobs of the tests (HPV_DEBUG_SPLIT_SKIP:
#                               a partner workgroup stays away from an in-kernel exchange; HPV_TEST_RCCL_*), the A/B switches between
#                               product paths (HPV_NO_INKERNEL_FINALIZE, HPV_PJ_WG_SMALL) and the dispatch trace (HPV_TRACE_DISPATCH)
#                               exist ONLY there -- the product library does not read those variables (tests/test_cabi.py greps the
#                               binary)
# What keeps the build short: one compilation instead of two for the AGPR-guarded files (the guard reads the assembly -save-temps
# leaves behind), the width-generic kernels as one translation unit per width AND input dimension (the 64-wide unit alone was 94 s),
# longest jobs started first, and only the sources whose text depends on HPV_TEST_HOOKS compiled a second time.
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $HPV_EXTRA_FLAGS"   # e.g. HPV_EXTRA_FLAGS=-DHPV_FZ_TIMING
SRCS="kernels_mfma kernels_fused kernels_fused_gen kernels_project kernels_tile kernels_tall kernels_generic kernels_validate kernels_adapt kernels_linadapt kernels_linop kernels_nonlin kernels_ident kernels_moment kernels_ansatz kernels_lbfgs hpv_api hpv_pass hpv_exchange hpv_bench hpv_lbfgs"
ELEM_SHAPES="20,20,10,10 16,16,8,8 12,12,6,6"             # kernels_elem.hip: one object per element shape (= HPV_ELEM_SHAPES of hpv_mfma_dev.h)
WIDE_WIDTHS="64 32 48 24 40"                            # kernels_wide.hip: one object per hidden width and dimension (= HPV_WIDE_WIDTHS of hpv_mfma.h)
# the sources whose text depends on HPV_TEST_HOOKS, their own or through HPV_XDEBUG_SKIP of hpv_mfma_dev.h (built twice)
HOOKED="kernels_fused kernels_fused_gen kernels_tile kernels_tall hpv_api hpv_pass hpv_exchange hpv_lbfgs"
TH_FLAGS="-DHPV_TEST_HOOKS"
CHK="python3 ../../scripts/check_agpr.py"
# objects are cached by mtime; a change of flags must invalidate them (.flags remembers what the objects were built with)
if [ "$(cat .flags 2>/dev/null)" != "$FLAGS|$HPV_FUSED_EXTRA|v3" ]; then rm -f *.o; echo "$FLAGS|$HPV_FUSED_EXTRA|v3" > .flags; fi

stale() {   # stale <object> <source>: the object is missing or older than its source / any header
  [ ! -f "$1" ] && return 0
  local d
  [ "$2" = kernels_fused_gen.hip ] && [ kernels_fused.hip -nt "$1" ] && return 0      # (that unit IS kernels_fused.hip, its other instantiations)
  for d in "$2" *.h ../../include/hpvpinn.h; do
    [ -f "$d" ] && [ "$d" -nt "$1" ] && return 0
  done
  return 1
}

# Three sources park live values in hand-chosen AGPRs.  They are compiled ONCE with -save-temps: scripts/check_agpr.py reads, from the
# device assembly the object was made from and for every instantiation in it, where the hand-managed range starts and how high the
# compiler's own registers reach.  If a compiler release ever needs more, the check names the flags that compile the offending
# instantiations out (the table in that script: the launch functions decline, the callers fall back; hpv_build_info() reports it,
# bench.py prints it) and the file is compiled again with them -- and the build says so loudly.  If the check cannot run at all
# (symbol not found after a rename, no assembly) or a guarded kernel spills to scratch memory, the build FAILS.
guarded_compile() {   # guarded_compile <source stem> <object> <extra flags> <file-only flags>
  local f=$1 obj=$2 extra=$3 XF=$4 asm=${2%.o}.s tmp=.tmp_${2%.o} add
  rm -rf $tmp; mkdir -p $tmp
  $HIPCC $FLAGS $XF $extra -save-temps=obj -c $f.hip -o $tmp/$f.o 2>$asm.err || { cat $asm.err >&2; rm -rf $tmp; return 1; }
  cp $tmp/$f-hip-amdgcn-amd-amdhsa-gfx950.s $asm || { echo "build.sh: ERROR -- no device assembly behind $f.hip" >&2; rm -rf $tmp; return 1; }
  add=$($CHK --plan $f $asm) || { echo "build.sh: ERROR -- the AGPR guard could not check $f.hip" >&2; rm -rf $tmp; return 1; }
  if [ -z "$add" ]; then mv $tmp/$f.o $obj; rm -rf $tmp; return 0; fi
  rm -rf $tmp
  $HIPCC $FLAGS $XF $add $extra -c $f.hip -o $obj      # (the guard tripped: once more, without the offending instantiations)
}

# The reducing kernels of the L-BFGS stage run 1024 threads on 128 registers each: the same check, on their assembly, that none of
# them spills (no hand-managed registers there: base 256).
spill_checked_compile() {   # spill_checked_compile <source stem> <object> <extra flags> <kernel-name substring>
  local f=$1 obj=$2 extra=$3 key=$4 tmp=.tmp_${2%.o}
  rm -rf $tmp; mkdir -p $tmp
  $HIPCC $FLAGS $extra -save-temps=obj -c $f.hip -o $tmp/$f.o || { rm -rf $tmp; return 1; }
  cp $tmp/$f-hip-amdgcn-amd-amdhsa-gfx950.s ${obj%.o}.s || { echo "build.sh: ERROR -- no device assembly behind $f.hip" >&2; rm -rf $tmp; return 1; }
  $CHK ${obj%.o}.s $key 256 >/dev/null || { echo "build.sh: ERROR -- a kernel of $f.hip spills to scratch memory (or could not be checked)" >&2; rm -rf $tmp; return 1; }
  mv $tmp/$f.o $obj; rm -rf $tmp
}

compile_one() {   # compile_one <source stem> <object> <extra flags>
  local f=$1 obj=$2 extra=$3
  if [ $f = kernels_fused ]; then guarded_compile $f $obj "$extra" "$HPV_FUSED_EXTRA"      # (A/B builds: flags for this file only, scripts/build_variant.sh --fused-only)
  elif [ $f = kernels_fused_gen ]; then guarded_compile $f $obj "$extra" "$HPV_FUSED_EXTRA"
  elif [ $f = kernels_tall ]; then guarded_compile $f $obj "$extra" ""
  elif [ $f = kernels_lbfgs ]; then spill_checked_compile $f $obj "$extra" k_lbfgs
  else $HIPCC $FLAGS $extra -c $f.hip -o $obj; fi
}

# job pool: at most NJ compilers at a time (27 at once on 8 cores cost 30 % more CPU time than 8 at a time), longest jobs first;
# a job that fails leaves a marker (wait -n consumes exit statuses)
NJ=${HPV_BUILD_JOBS:-${MAX_JOBS:-$(nproc)}}
rm -f .fail_*
spawn() {   # spawn <object name> <command...>
  local name=$1; shift
  while [ "$(jobs -rp | wc -l)" -ge "$NJ" ]; do wait -n || true; done
  ( "$@" || { echo "build.sh: ERROR -- $name failed" >&2; rm -f $name; touch .fail_$name; } ) &
}
# the longest jobs first (they set the wall clock): the width-generic and the generic element-resident kernels
for w in $WIDE_WIDTHS; do
  for d in 2 1; do
    o=kernels_wide_${w}_d$d.o
    if stale $o kernels_wide.hip; then
      spawn $o $HIPCC $FLAGS -DHPV_WIDE_H=$w -DHPV_WIDE_D=$d -c kernels_wide.hip -o $o
    fi
  done
done
for sh in $ELEM_SHAPES; do
  IFS=, read qx qy ntx nty <<< "$sh"
  o=kernels_elem_${qx}_${qy}_${ntx}_${nty}.o
  if stale $o kernels_elem.hip; then
    spawn $o $HIPCC $FLAGS -DHPV_ELEM_QX=$qx -DHPV_ELEM_QY=$qy -DHPV_ELEM_NTX=$ntx -DHPV_ELEM_NTY=$nty -c kernels_elem.hip -o $o
  fi
done
for f in $SRCS; do
  [ -f $f.hip ] || continue
  if stale $f.o $f.hip; then spawn $f.o compile_one $f $f.o ""; fi
done
for f in $HOOKED; do
  if stale $f.th.o $f.hip; then spawn $f.th.o compile_one $f $f.th.o "$TH_FLAGS"; fi
done
wait
if ls .fail_* >/dev/null 2>&1; then rm -f .fail_*; exit 1; fi

OBJS=""; TOBJS=""
for f in $SRCS; do
  [ -f $f.hip ] || continue
  OBJS="$OBJS $f.o"
  case " $HOOKED " in *" $f "*) TOBJS="$TOBJS $f.th.o";; *) TOBJS="$TOBJS $f.o";; esac
done
for w in $WIDE_WIDTHS; do
  for d in 1 2; do
    OBJS="$OBJS kernels_wide_${w}_d$d.o"; TOBJS="$TOBJS kernels_wide_${w}_d$d.o"
  done
done
for sh in $ELEM_SHAPES; do o=kernels_elem_${sh//,/_}.o; OBJS="$OBJS $o"; TOBJS="$TOBJS $o"; done
# -Bsymbolic: the two libraries may live in one process (the tests load both); each must bind its internal calls to itself
$HIPCC --offload-arch=gfx950 -shared -fPIC -Wl,-Bsymbolic -o ../libhpvpinn.so $OBJS & l1=$!
$HIPCC --offload-arch=gfx950 -shared -fPIC -Wl,-Bsymbolic -o ../libhpvpinn_testhooks.so $TOBJS & l2=$!
wait $l1; wait $l2
echo "built $(cd .. && pwd)/libhpvpinn.so (+ libhpvpinn_testhooks.so)"
