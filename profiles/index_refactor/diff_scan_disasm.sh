#!/bin/bash
# diff_scan_disasm.sh PARENT_OBJ BRANCH_OBJ -- per scan kernel (k_ivf_scan*, every
# instantiation), whether the gfx950 instruction text of two builds of
# kernels_ivf.o is the same: the disassembly of each kernel's symbol with the
# addresses and encodings stripped (branch targets stay as label names).
set -e
BIN=/opt/rocm/lib/llvm/bin
tmp=$(mktemp -d)
i=0
for obj in "$1" "$2"; do
  i=$((i + 1))
  $BIN/llvm-objcopy --dump-section .hip_fatbin=$tmp/fb$i "$obj" $tmp/copy$i.o
  $BIN/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$tmp/fb$i --output=$tmp/co$i --unbundle
  # "<symbol>:" lines start a function; instruction lines: text before the "//" encoding comment
  $BIN/llvm-objdump -d $tmp/co$i | awk -v out=$tmp/k$i '
    /^[0-9a-f]+ <.*>:$/ { name = $2; gsub(/[<>:]/, "", name); f = (name ~ /k_ivf_scan/) ? out "_" name : ""; next }
    f != "" && NF { sub(/[ \t]*\/\/.*$/, ""); print > f }'
done
for f in $tmp/k1_*; do
  n=${f#$tmp/k1_}
  lines=$(wc -l < $f)
  if cmp -s $f $tmp/k2_$n; then echo "same      $lines instructions  $(echo $n | c++filt)"
  else echo "DIFFERENT $lines vs $(wc -l < $tmp/k2_$n)  $(echo $n | c++filt)"; fi
done
rm -rf $tmp
