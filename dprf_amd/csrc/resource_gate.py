#!/usr/bin/env python3
"""Build gate on the compiler's kernel resource report (hipcc -Rpass-analysis=kernel-resource-usage).

The Makefile compiles every kernel object with that remark enabled, writes the remarks to <obj>.res and runs
this script on them.  It fails the build when a kernel spills to scratch beyond its stated bound, so a
compiler-flag or source change that starts spilling cannot ship silently (round 2 shipped k_odt_kdf with
20 B/lane of scratch under the max-ilp scheduler: 1.46x its algorithmic HBM writes).

Usage: resource_gate.py [--expect k1,k2,...] <file.res>...   (one line per kernel; exit 1 on a violation)

The gate fails closed (round 4): a remark block without a ScratchSize line, a report with no kernel in
it, or an expected kernel (--expect, the Makefile passes each object's kernel families) missing from the report
all fail the build -- a changed remark format or a dropped -Rpass-analysis flag must not read as "0 B of scratch".
"""
import re
import subprocess
import sys

# Kernel name (demangled; an entry with template arguments wins over the bare name) -> the most scratch it may
# use, bytes/lane.  Every kernel must appear here: an unknown kernel fails the gate too.
SCRATCH_LIMIT = {
    # every kernel at 0 B/lane since round 3 (list-mode R6 had 16 until the persistent loop stopped holding its lane
    # index and the watchdog's 64-bit timestamp in registers: dprf_kernels_r6.hip opaque_lane, idle_t0 in LDS)
    "k_office_kdf": 0,
    "k_office_check": 0,
    "k_odt_kdf": 0,
    "k_odt_check": 0,
    "k_pdf_r5": 0,
    "k_pdf_r24": 0,
    "k_pdf_r6": 0,
    "k_long_prehash": 0,      # round 4: candidates longer than a list slot
    "k_spell_symbols": 0,     # the device spellers (dprf_kernels_spell.hip): symbol windows (dprf_search_symbols)
    "k_spell_mask": 0,        # ... mask windows (dprf_search_mask)
    "k_pdf_r24_owner": 0,     # owner-password search (dprf_ctx_set_pdf_password)
    "k_pdf_r5_owner": 0,
    "k_pdf_r6_owner": 0,
    "k_agile_kdf": 0,         # Office 2010 / 2013 Agile Encryption (dprf_kernels_agile.hip)
    "k_agile_check": 0,
    "k_spell_hybrid": 0,      # ... hybrid windows (dprf_search_hybrid)
    "k_spell_rules": 0,       # ... rule windows (dprf_search_rules / dprf_spell_rules)
    "k_spell_combine": 0,     # ... combinator windows (dprf_search_combine / dprf_spell_combine)
    "k_oldoffice": 0,         # Office 97-2003 RC4 / RC4 CryptoAPI (dprf_kernels_oldoffice.hip)
    "k_odf_bf_kdf": 0,        # ODF 1.0 / 1.1 Blowfish-CFB (dprf_kernels_odf.hip)
    "k_odf_bf_check": 0,
    "k_key40_pdf": 0,         # 40-bit key search (dprf_search_key40): PDF R2-R4, Office 97-2003
    "k_key40_oldoffice": 0,
    "k_collide_pdf": 0,       # password for a known 40-bit key (dprf_ctx_set_key40): PDF R2-R4, Office 97-2003
    "k_collide_oldoffice": 0,
    "k_odf_aes_kdf": 0,       # ODF 1.2 at the manifest's iteration count (dprf_kernels_odfaes.hip); its check is k_odt_check
}


def parse(text):
    rows, cur = {}, None
    for ln in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z /\[\]]*?): (\S+) \[-Rpass-analysis", ln)
        if m and cur:
            rows[cur][m.group(1).strip()] = m.group(2)
    return rows


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    except OSError:
        return {n: n for n in names}
    return {n: (out[i] if i < len(out) and out[i] else n) for i, n in enumerate(names)}


def main(argv):
    bad, expect, paths = [], set(), []
    it = iter(argv)
    for a in it:
        if a == "--expect":
            expect |= {x for x in next(it, "").split(",") if x}
        else:
            paths.append(a)
    seen = set()
    for path in paths:
        rows = parse(open(path).read())
        if not rows:
            bad.append("%s: no kernel in the resource report" % path)
        dem = demangle(list(rows))
        for mangled, r in rows.items():
            name = dem[mangled].split("(")[0]
            full = re.sub(r"^void ", "", name)
            seen.add(full.split("<")[0])
            if "ScratchSize [bytes/lane]" not in r:
                bad.append("%s (no ScratchSize remark)" % name)
                continue
            scratch = int(r["ScratchSize [bytes/lane]"])
            limit = SCRATCH_LIMIT.get(full.replace(" ", ""), SCRATCH_LIMIT.get(full.split("<")[0]))
            ok = limit is not None and scratch <= limit
            print("%-6s %-44s VGPRs %-4s scratch %-3d (limit %s) occupancy %s" % (
                "ok" if ok else "FAIL", name[:44], r.get("VGPRs"), scratch, "unknown kernel" if limit is None else limit,
                r.get("Occupancy [waves/SIMD]")))
            if not ok:
                bad.append(name)
    for k in sorted(expect - seen):
        bad.append("%s (expected, not in the report)" % k)
    if bad:
        sys.stderr.write("resource_gate: scratch above the stated bound, unknown or missing kernel, or no report: %s\n" % ", ".join(bad))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
