#!/bin/bash
# Are the existing kernels instruction-identical in two builds of the library?
#   bash scripts/isa_diff.sh <csrc/build of the parent commit> <csrc/build of this tree>
# For every hot-kernel variant object, env_opp.o, vs_expert.o and env_after.o of the three record builds: the gfx950 code object is taken out of the
# host object (llvm-objdump --offloading), disassembled, and compared with the kernel-name suffix of the anonymous
# namespace and the __hip_cuid_ symbol normalised.  Prints SAME / DIFFERENT per object; exit status 1 if any differs.
LLVM=${LLVM:-/opt/rocm/lib/llvm/bin}
old=$1; new=$2; rc=0
dis() {
  tmp=$(mktemp -d); cp "$1" $tmp/x.o
  (cd $tmp && $LLVM/llvm-objdump --offloading x.o > /dev/null)
  $LLVM/llvm-objdump -d --no-show-raw-insn --no-leading-addr $tmp/x.o.0.hipv4-amdgcn-amd-amdhsa--gfx950 |
    sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g; s/_GLOBAL__N_[0-9]+/_GLOBAL__N_/g' | grep -v 'file format'
  rm -rf $tmp
}
for b in std ext big; do
  for o in $old/$b/variant_*.o $old/$b/env_opp.o $old/$b/vs_expert.o $old/$b/env_after.o; do
    f=$b/$(basename $o)
    if cmp -s <(dis $o) <(dis $new/$f); then echo "SAME      $f ($(dis $o | wc -l) lines)"; else echo "DIFFERENT $f"; rc=1; fi
  done
done
exit $rc
