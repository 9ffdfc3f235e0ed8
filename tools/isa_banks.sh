#!/bin/bash
# isa_banks.sh <outdir|file.s> <kernel-symbol-regex> [hipcc -D flags...]: VGPR source banks in the hot loops of count kernel instances.
# With a directory, qs_count.hip and qs_count_fused.hip are compiled for gfx950 with the given flags (two to three minutes) and the .s
# files kept there; with a .s file, that file is read as it is. For every kernel whose symbol matches the regex, e.g.
#   tools/isa_banks.sh /tmp/isa 'count_bitslice3_kernelILi4ELi0EjLi2E'      (4 bits, binary_full, u32 cells, the six-wave order)
# it prints the instance's VGPRs, spills, scratch, LDS and occupancy, and for every innermost loop (label .. backward branch to it)
# that holds more than MIN_BITOP3 v_bitop3 (environment, default 64: the smallest step loop, one a-column with a cut d-block, holds ~100,
# and an edit moves it by a few either way):
#   v_bitop3 count, and how many have src0 and src1 (both VGPRs) in ONE bank (bank = register number mod 4; src2 is free:
#   profiles/r03_experiments.md 7); v_bcnt count, and how many have both sources in one bank; the other VALU instructions.
# A report for reading, not a gate: which registers the allocator picks may change with any edit or compiler.
set -e
T=${1:?outdir or file.s}; K=${2:?kernel regex}; shift 2
if [ -d "$T" ] || [ "${T%.s}" = "$T" ]; then
    mkdir -p "$T"
    OUT=$(cd "$T" && pwd)
    cd "$(dirname "$0")/../quartetscores_amd/csrc"
    for f in qs_count qs_count_fused; do
        /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 "$@" -save-temps=obj -c $f.hip -o "$OUT/$f.o" 2>/dev/null
    done
    FILES="$OUT/qs_count-hip-amdgcn-amd-amdhsa-gfx950.s $OUT/qs_count_fused-hip-amdgcn-amd-amdhsa-gfx950.s"
else
    FILES=$T
fi
for S in $FILES; do
awk -v K="$K" -v MIN="${MIN_BITOP3:-64}" '
function bank(r) { return (substr(r, 2) + 0) % 4 }
function isv(r) { return r ~ /^v[0-9]+$/ }
function flush(   i, j) {
    if (!name) return
    ++nk; kname[nk] = name
    rep[nk] = sprintf("  vgpr %s spill @ scratch %s lds %s occupancy %s\n", vg, sc, lds, occ)
    # a loop that holds another hot loop well inside it is an outer loop: not reported. Of loops that overlap otherwise (the entry
    # ladder of an instance whose d-rows are conditional, a loop header two lines further down) the one with the most v_bitop3 is.
    for (i = 1; i <= nl; ++i) {
        keep[i] = lb3[i] > MIN
        for (j = 1; j <= nl; ++j) if (j != i && lb3[j] > MIN && llo[j] >= llo[i] + 8 && lhi[j] <= lhi[i] - 8) keep[i] = 0
    }
    for (i = 1; i <= nl; ++i) {
        if (!keep[i]) continue
        for (j = 1; j <= nl; ++j)
            if (j != i && keep[j] && llo[j] <= lhi[i] && lhi[j] >= llo[i] && (lb3[j] > lb3[i] || (lb3[j] == lb3[i] && j < i))) keep[i] = 2
    }
    for (i = 1; i <= nl; ++i) {
        if (keep[i] != 1) continue
        rep[nk] = rep[nk] sprintf("  loop %s (lines %d..%d): v_bitop3 %d, src0/src1 in one bank %d; v_bcnt %d, both sources in one bank %d; other VALU %d\n",
               llab[i], llo[i], lhi[i], lb3[i], lb3c[i], lbc[i], lbcc[i], lov[i])
    }
    name = ""
}
# the code of a kernel: from its label to .Lfunc_end; the resource lines follow as comments
/^_Z[A-Za-z0-9_]*:/ { flush(); sym = $1; sub(/:$/, "", sym); if (sym ~ K) { name = sym; code = 1; n = 0; nl = 0; delete lab; vg = sc = lds = occ = "?" } else code = 0; next }
name && code {
    ++n
    if ($1 ~ /^\.LBB[0-9_]+:/) { l = $1; sub(/:$/, "", l); lab[l] = n }
    op[n] = $1; a1[n] = $3; a2[n] = $4; gsub(/,/, "", a1[n]); gsub(/,/, "", a2[n])
    if ($1 ~ /^s_cbranch|^s_branch/ && ($2 in lab)) {   # backward branch: a loop
        ++nl; llab[nl] = $2; llo[nl] = lab[$2]; lhi[nl] = n
        lb3[nl] = lb3c[nl] = lbc[nl] = lbcc[nl] = lov[nl] = 0
        for (i = lab[$2]; i <= n; ++i) {
            if (op[i] ~ /^v_bitop3_b32/) { ++lb3[nl]; if (isv(a1[i]) && isv(a2[i]) && bank(a1[i]) == bank(a2[i])) ++lb3c[nl] }
            else if (op[i] ~ /^v_bcnt_u32_b32/) { ++lbc[nl]; if (isv(a1[i]) && isv(a2[i]) && bank(a1[i]) == bank(a2[i])) ++lbcc[nl] }
            else if (op[i] ~ /^v_/) ++lov[nl]
        }
    }
    if ($1 ~ /^\.Lfunc_end/) code = 0
    next
}
name && /^; NumVgprs:/ { vg = $3 }
name && /^; ScratchSize:/ { sc = $3 }
name && /^; Occupancy:/ { occ = $3 }
name && /^; LDSByteSize:/ { lds = $3 }
# the spill counts stand in the metadata at the end of the file
/^ +\.name: / { flush(); mname = $2 }
/^ +\.vgpr_spill_count: / { spill[mname] = $2 }
END { flush(); for (i = 1; i <= nk; ++i) { r = rep[i]; sub(/@/, (kname[i] in spill) ? spill[kname[i]] : "?", r); printf("%s\n%s", kname[i], r) } }' "$S"
done
