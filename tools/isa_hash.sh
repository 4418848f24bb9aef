#!/bin/bash
# ISA fingerprint of the device code of every object of the library: sha256 of the gfx950 disassembly (llvm-objdump -d) of
# each csrc/build/*.o.  Two builds whose fingerprints agree run the same machine code (the fat binary itself carries a
# per-compilation id and cannot be compared directly).  Usage: tools/isa_hash.sh [object-dir] > file; diff two files.
#
# tools/isa_hash.sh --kernels [object-dir] prints one line per kernel instead: object, kernel symbol, sha256 of the kernel's
# instructions -- mnemonic and operands of each, in order.  The address, the raw encoding and the absolute address of a branch's
# target (llvm-objdump's comment behind each instruction; the operand of a branch is relative) are left out, and so is the
# padding between the kernel's last s_endpgm and the next aligned symbol, so a kernel's hash does not depend on where it stands in
# its object or in which object: `sort -k2` of two trees' lists shows a kernel that moved between units as the same (symbol,
# hash) under another object.
set -e
MODE=objects
if [ "$1" = --kernels ]; then MODE=kernels; shift; fi
DIR=${1:-bayesian-inference-trpl_amd/csrc/build}
BIN=/opt/rocm/lib/llvm/bin
TMP=$(mktemp -d)

# the kernels of $TMP/$1.elf (the symbols with a kernel descriptor <symbol>.kd), each hashed alone
kernels() {
    mkdir "$TMP/k"
    nm "$TMP/$1.elf" | sed -n 's/^.* \([^ ]*\)\.kd$/\1/p' > "$TMP/k/kd"
    [ -s "$TMP/k/kd" ] || { rm -rf "$TMP/k"; return 0; }           # device code without a kernel
    $BIN/llvm-objdump -d "$TMP/$1.elf" | awk -v dir="$TMP/k" '
        function flush(   i, f) {
            if (sym == "" || !(sym in kd)) return
            while (n > 0 && (line[n] == "s_nop 0" || line[n] == "s_code_end")) n--
            f = dir "/" (++count)
            print sym > (dir "/names")
            for (i = 1; i <= n; i++) print line[i] > f
            close(f)
        }
        FNR == NR { kd[$1] = 1; next }
        /^[0-9a-f]+ <.*>:$/ { flush(); sym = substr($2, 2, length($2) - 3); n = 0; next }
        sym != "" && /^[ \t]+[a-z]/ { sub(/[ \t]*\/\/.*$/, ""); gsub(/[ \t]+/, " "); sub(/^ /, ""); line[++n] = $0 }
        END { flush() }' "$TMP/k/kd" -
    i=0
    while read -r sym; do
        i=$((i + 1))
        echo "$1 $sym $(sha256sum < "$TMP/k/$i" | cut -c1-32)"
    done < "$TMP/k/names"
    rm -rf "$TMP/k"
}

for o in "$DIR"/*.o; do
    n=$(basename "$o" .o)
    objcopy --dump-section .hip_fatbin="$TMP/$n.fatbin" "$o" 2>/dev/null || true
    [ -s "$TMP/$n.fatbin" ] || { [ $MODE = kernels ] || echo "$n host-only"; continue; }
    $BIN/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$TMP/$n.fatbin" --output="$TMP/$n.elf" --unbundle
    if [ $MODE = kernels ]; then kernels "$n"
    else $BIN/llvm-objdump -d "$TMP/$n.elf" | grep -v "file format" | sha256sum | cut -c1-32 | sed "s/^/$n /"
    fi
done
rm -rf "$TMP"
