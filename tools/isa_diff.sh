#!/bin/bash
# Device-ISA comparison of two builds, kernel by kernel: unbundles the gfx950 code object of every dprf_kernels_*.o in
# OBJ_A and OBJ_B, cuts the disassembly at the kernel symbols and compares each kernel of A with the kernel of the same
# name in B, whichever object it lives in -- so a kernel that moved to another source file still lines up.  Addresses
# and encodings are dropped (branch targets are relative, so the instruction text is comparable) and so is the padding
# after a kernel's last instruction (s_code_end, trailing s_nop).  One line per kernel; exit 0 only when every kernel
# of either build has an equal twin in the other: then a source change cannot have moved a bench number.
#   usage: tools/isa_diff.sh OBJ_A OBJ_B
set -euo pipefail
A=${1:?object dir A}; B=${2:?object dir B}
L=${LLVM_BIN:-/opt/rocm/lib/llvm/bin}
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
FILT=$(command -v "$L/llvm-cxxfilt" || command -v c++filt || command -v cat)   # readable names where a demangler is at hand

# kernels DIR OUT: one file OUT/<mangled name> per kernel, one instruction per line
kernels() {
    mkdir -p "$2"
    for f in "$1"/dprf_kernels_*.o; do
        "$L/llvm-objcopy" --dump-section .hip_fatbin="$T/fb" "$f" "$T/junk.o"
        tgt=$("$L/clang-offload-bundler" --list --type=o --input="$T/fb" | grep gfx950)
        "$L/clang-offload-bundler" --type=o --targets="$tgt" --input="$T/fb" --output="$T/co" --unbundle
        "$L/llvm-objdump" -d --no-show-raw-insn "$T/co" | awk -v out="$2" '
            function flush(   i) {
                if (name == "") return
                # padding: s_nop and s_code_end behind the last instruction, "..." where objdump elides zero bytes
                while (n > 0 && ins[n] ~ /^(s_nop|s_code_end|[ \t]*\.\.\.[ \t]*$)/) n--
                for (i = 1; i <= n; i++) print ins[i] > (out "/" name)
                close(out "/" name)
            }
            /^[0-9a-f]+ <.*>:$/ { flush(); name = $2; gsub(/[<>:]/, "", name); n = 0; next }
            /^\t/ { sub(/[ \t]*\/\/.*$/, ""); sub(/^\t/, ""); ins[++n] = $0 }
            END { flush() }'
    done
}
kernels "$A" "$T/A"
kernels "$B" "$T/B"

rc=0
for k in $( (ls "$T/A"; ls "$T/B") | sort -u ); do
    name=$(echo "$k" | "$FILT" | sed 's/(.*//; s/^void //')
    if [ ! -f "$T/A/$k" ] || [ ! -f "$T/B/$k" ]; then
        echo "$name: only in $([ -f "$T/A/$k" ] && echo A || echo B)"; rc=1; continue
    fi
    na=$(wc -l < "$T/A/$k"); nb=$(wc -l < "$T/B/$k")
    if cmp -s "$T/A/$k" "$T/B/$k"; then
        echo "$name: equal, $na instructions"
    else
        n=$(diff "$T/A/$k" "$T/B/$k" | grep -c '^[<>]' || true)
        echo "$name: DIFFERENT, $na / $nb instructions, $n differing lines"; rc=1
    fi
done
exit $rc
