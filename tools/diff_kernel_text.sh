#!/bin/bash
# diff_kernel_text.sh [-r] [-p PATTERN] PARENT_OBJ... -- BRANCH_OBJ...
#
# Whether two builds hold the same gfx950 kernels.  Each side is a list of
# object files (or code objects' hosts: anything with a .hip_fatbin section);
# the kernels of a side are the union over its objects, so a source file split
# into several compares against its unsplit parent.  Per mangled kernel name
# (those matching the awk regex PATTERN; default: every kernel):
#   same / DIFFERENT  the instruction text (disassembly with addresses,
#                     encodings and the branch-target comments stripped) and
#                     the four resource notes: vgpr, sgpr, lds (group segment)
#                     and scratch (private segment) bytes
#   MISSING           present on one side only
#   reordered         (with -r, instead of DIFFERENT) the same instruction lines
#                     in another order: equal resource notes and identical text
#                     once both sides' lines are sorted -- a schedule change
#                     only; not counted as a failure
# Padding after a kernel's last s_endpgm is not compared when it is only
# `s_nop 0`, `s_code_end` or `...` lines (it depends on which kernel comes last
# in an object); anything else there stays in and shows as a difference.
# Exit status 1 on any DIFFERENT or MISSING.
set -e -o pipefail
BIN=${ROCM_PATH:-/opt/rocm}/lib/llvm/bin
pat=.
reorder=0
while [ "$1" = "-p" ] || [ "$1" = "-r" ]; do
  if [ "$1" = "-r" ]; then
    reorder=1
    shift
  else
    pat=$2
    shift 2
  fi
done
tmp=$(mktemp -d)
trap 'rm -rf $tmp' EXIT
mkdir $tmp/1 $tmp/2
touch $tmp/1/notes $tmp/2/notes
side=1
for obj; do
  if [ "$obj" = "--" ]; then
    side=2
    continue
  fi
  if ! $BIN/llvm-objcopy --dump-section .hip_fatbin=$tmp/fb "$obj" $tmp/copy.o 2> /dev/null; then
    echo "(no device code: $obj)" >&2
    continue
  fi
  $BIN/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$tmp/fb --output=$tmp/co --unbundle
  # the kernels' entries of amdhsa.kernels (keys at 4 columns; the arguments' are deeper)
  $BIN/llvm-readelf --notes $tmp/co | awk -v pat="$pat" '
    function flush() { if (name != "" && name ~ pat) print name, "vgpr", v, "sgpr", s, "lds", g, "scratch", p; name = "" }
    /^  - / { flush() }
    /^amdhsa\.[a-z]+:/ && !/^amdhsa\.kernels:/ { flush() }
    /^    \.name:/ { name = $2 }
    /^    \.vgpr_count:/ { v = $2 }
    /^    \.sgpr_count:/ { s = $2 }
    /^    \.group_segment_fixed_size:/ { g = $2 }
    /^    \.private_segment_fixed_size:/ { p = $2 }
    END { flush() }' > $tmp/notes
  # "<symbol>:" lines start a function; instruction lines: text before the "//" encoding comment
  $BIN/llvm-objdump -d $tmp/co | awk -v out=$tmp/$side/ -v notes=$tmp/notes '
    BEGIN { while ((getline line < notes) > 0) { split(line, a, " "); want[a[1]] = 1 } }
    /^[0-9a-f]+ <.*>:$/ { name = $2; gsub(/[<>:]/, "", name); f = (name in want) ? out name ".txt" : ""; next }
    f != "" && NF { sub(/[ \t]*\/\/.*$/, ""); print > f }'
  cat $tmp/notes >> $tmp/$side/notes
done
if [ $side = 1 ]; then
  echo "usage: $0 [-r] [-p PATTERN] PARENT_OBJ... -- BRANCH_OBJ..." >&2
  exit 2
fi
# the text up to the last s_endpgm, when only padding follows it
strip_padding() {
  awk '{ l[NR] = $0; t = $0; gsub(/^[ \t]+|[ \t]+$/, "", t); if (t == "s_endpgm") last = NR }
       END { n = last ? last : NR
             for (i = last + 1; last && i <= NR; i++) {
               t = l[i]; gsub(/^[ \t]+|[ \t]+$/, "", t)
               if (t != "s_nop 0" && t != "s_code_end" && t != "...") n = NR
             }
             for (i = 1; i <= n; i++) print l[i] }' "$1"
}
same=0
diff=0
missing=0
reordered=0
for name in $(cat $tmp/1/notes $tmp/2/notes | cut -d' ' -f1 | sort -u); do
  pretty=$(echo $name | c++filt)
  n1=$(grep -m1 "^$name " $tmp/1/notes | cut -d' ' -f2- || true)
  n2=$(grep -m1 "^$name " $tmp/2/notes | cut -d' ' -f2- || true)
  if [ -z "$n1" ] || [ -z "$n2" ]; then
    echo "MISSING   in $([ -z "$n1" ] && echo parent || echo branch)  $pretty"
    missing=$((missing + 1))
    continue
  fi
  strip_padding $tmp/1/$name.txt > $tmp/a
  strip_padding $tmp/2/$name.txt > $tmp/b
  if cmp -s $tmp/a $tmp/b && [ "$n1" = "$n2" ]; then
    echo "same      $(wc -l < $tmp/a) instructions  $n1  $pretty"
    same=$((same + 1))
  elif [ $reorder = 1 ] && [ "$n1" = "$n2" ] && sort $tmp/a | cmp -s - <(sort $tmp/b); then
    echo "reordered $(wc -l < $tmp/a) instructions  $n1  $pretty"
    reordered=$((reordered + 1))
  else
    echo "DIFFERENT $(wc -l < $tmp/a) vs $(wc -l < $tmp/b) instructions  $n1 | $n2  $pretty"
    diff=$((diff + 1))
  fi
done
echo "$((same + reordered + diff + missing)) kernels: $same same, $([ $reorder = 1 ] && echo "$reordered reordered, ")$diff DIFFERENT, $missing MISSING"
[ $((diff + missing)) = 0 ]
