#!/bin/bash
# One line per kernel of a HIP source, sorted by name: the .amdhsa_ resource numbers tools/kernel_regs.sh prints and the sha256 of the
# kernel's instruction text -- to show that a change of the source text left the device code alone: run it over both trees and diff.
#   tools/kernel_isa.sh eppm_amd/csrc/k_pm_sweep.hip [extra hipcc flags, e.g. -DEPPM_TOL=1]
# Compiles the device code to gfx950 assembly with the Makefile's FLAGS.  Hashed per kernel: the lines from the kernel's label to its
# .Lfunc_end, without the .amdhsa_kernel block (printed as numbers), without comments, and with what depends only on the kernel's
# position in the translation unit normalised: the function index of local labels (.LBB<n>_, .LJTI<n>_, .Lfunc_end<n>) is dropped,
# .Ltmp<n> is renumbered from 0 inside each kernel.
src=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
flags=$(make -s -C "$root/eppm_amd/csrc" --eval='print-flags: ; @echo $(FLAGS)' print-flags) || exit 1
tmp=$(mktemp -d /tmp/kisa.XXXXXX)
trap 'rm -rf "$tmp"' EXIT
/opt/rocm/bin/hipcc $flags --cuda-device-only -S -o "$tmp/dev.s" "$@" "$src" 2>"$tmp/err" || { cat "$tmp/err" >&2; exit 1; }
awk -v dir="$tmp" '
    NR == FNR { if ($1 == ".amdhsa_kernel") kernel[$2 ":"] = 1; next }          # first pass: which labels are kernels
    !cur && ($1 in kernel) { cur = $1; sub(/:$/, "", cur); n++; body = dir "/k" n; ntmp = 0; split("", tmpno); next }
    !cur { next }
    $1 == ".amdhsa_kernel" { meta = 1; next }
    $1 == ".end_amdhsa_kernel" {
        meta = 0
        res[n] = sprintf("%s vgpr %s (arch %s) sgpr %s lds %s scratch %s", cur, v, a, s, l, p)
        next
    }
    meta {
        if ($1 == ".amdhsa_next_free_vgpr") v = $2; else if ($1 == ".amdhsa_next_free_sgpr") s = $2
        else if ($1 == ".amdhsa_group_segment_fixed_size") l = $2; else if ($1 == ".amdhsa_private_segment_fixed_size") p = $2
        else if ($1 == ".amdhsa_accum_offset") a = $2
        next
    }
    {
        line = $0
        sub(/[ \t]*;.*$/, "", line)
        if (line ~ /^[ \t]*$/) next
        gsub(/\.LBB[0-9]+_/, ".LBB_", line); gsub(/\.LJTI[0-9]+_/, ".LJTI_", line); gsub(/\.Lfunc_end[0-9]+/, ".Lfunc_end", line)
        while (match(line, /\.Ltmp[0-9]+/)) {
            t = substr(line, RSTART, RLENGTH)
            if (!(t in tmpno)) tmpno[t] = ntmp++
            line = substr(line, 1, RSTART - 1) ".LT" tmpno[t] substr(line, RSTART + RLENGTH)
        }
        print line > body
        if (line ~ /^\.Lfunc_end:/) { close(body); print res[n] > (dir "/r" n); close(dir "/r" n); cur = "" }
    }
' "$tmp/dev.s" "$tmp/dev.s"
for r in "$tmp"/r*; do
    [ -e "$r" ] || continue
    echo "$(cat "$r") sha256 $(sha256sum < "${r%/r*}/k${r##*/r}" | cut -d' ' -f1)"
done | c++filt | sed 's/eppm:://g; s/(eppm::PmBatch.*)//; s/(PmBatch[^)]*)//' | LC_ALL=C sort
