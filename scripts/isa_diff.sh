#!/bin/bash
# Are the existing kernels instruction-identical in two builds of the library, and do they use the same resources?
#   bash scripts/isa_diff.sh <csrc/build of the parent commit> <csrc/build of this tree>
# For every object the parent's build directory holds, per record build (std, ext, big; the hot-kernel variants first, then
# the other objects by name), and every one only this tree's holds (not compared: printed as NEW with its resources): the
# gfx950 code object is taken out of the host object (llvm-objdump --offloading), disassembled, and compared with the kernel-name suffix of the anonymous
# namespace and the __hip_cuid_ symbol normalised.  Prints SAME / DIFFERENT per object, and next to it what decides the
# waves per SIMD, old -> new: per kernel the VGPR count, the private segment (scratch) and the static LDS of the code-object
# metadata, and the number of scratch_* instructions of the object.  Exit status 1 if any object differs, 2 if a kernel
# uses more VGPRs, its scratch or LDS size differs, or the scratch_* count grew.
LLVM=${LLVM:-/opt/rocm/lib/llvm/bin}
old=$1; new=$2; rc=0
unpack() {   # $1 = host object -> prints the directory holding x.co
  tmp=$(mktemp -d); cp "$1" $tmp/x.o
  (cd $tmp && $LLVM/llvm-objdump --offloading x.o > /dev/null && mv x.o.0.hipv4-amdgcn-amd-amdhsa--gfx950 x.co)
  echo $tmp
}
dis() {
  $LLVM/llvm-objdump -d --no-show-raw-insn --no-leading-addr $1/x.co |
    sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g; s/_GLOBAL__N_[0-9]+/_GLOBAL__N_/g' | grep -v 'file format'
}
res() {   # "vgpr V scratch S lds L" per kernel, in symbol order, then the scratch_* instructions of the object
  $LLVM/llvm-readelf --notes $1/x.co | awk '
    /\.group_segment_fixed_size:/ {l = $2} /\.private_segment_fixed_size:/ {s = $2} /\.vgpr_count:/ {v = $2}
    /\.wavefront_size:/ {printf "vgpr %s scratch %s lds %s; ", v, s, l}'
  echo "scratch_* $(dis $1 | grep -c '^[[:space:]]*scratch_')"
}
for b in std ext big; do
  names=$(for o in $old/$b/variant_*.o $old/$b/*.o; do basename $o; done | awk '!seen[$0]++'
          for o in $new/$b/*.o; do [ -f $old/$b/$(basename $o) ] || basename $o; done)
  for n in $names; do
    o=$old/$b/$n; f=$b/$n
    if [ ! -f $o ]; then
      if [ -f $new/$f ]; then tn=$(unpack $new/$f); echo "NEW       $f ($(dis $tn | wc -l) lines)  $(res $tn)"; rm -rf $tn; fi
      continue
    fi
    to=$(unpack $o); tn=$(unpack $new/$f)
    ro=$(res $to); rn=$(res $tn)
    if cmp -s <(dis $to) <(dis $tn); then echo "SAME      $f ($(dis $to | wc -l) lines)  $rn"; else echo "DIFFERENT $f  $ro -> $rn"; [ $rc = 0 ] && rc=1; fi
    # a kernel may use fewer VGPRs than the parent's (never fewer waves per SIMD); more VGPRs, another scratch or LDS size
    # or more scratch_* instructions fail
    if ! python3 - "$ro" "$rn" <<'PY'
import re, sys
f = lambda t: ([tuple(map(int, m)) for m in re.findall(r"vgpr (\d+) scratch (\d+) lds (\d+)", t)], int(t.split()[-1]))
(ko, so), (kn, sn) = f(sys.argv[1]), f(sys.argv[2])
ok = len(ko) == len(kn) and sn <= so and all(n[0] <= o[0] and n[1:] == o[1:] for o, n in zip(ko, kn))
sys.exit(0 if ok else 1)
PY
    then echo "  RESOURCES DIFFER $f"; rc=2; fi
    rm -rf $to $tn
  done
done
exit $rc
