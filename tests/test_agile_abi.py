"""The host-visible surface of Office 2010 / 2013 Agile Encryption support, without a GPU: the chunk policy knows both
kernel families (how a caller detects the support, include/dprf.h "Agile"), the header documents them, and the build's
resource gate holds the new kernels at 0 B of scratch."""
import os
import re
import sys

import pytest

from conftest import REPO

FAMILIES = ["office_agile_sha1", "office_agile_sha512"]
CSRC = os.path.join(REPO, "dprf_amd", "csrc")
HUGE = 1 << 40


@pytest.mark.parametrize("family", FAMILIES)
def test_plan_chunk_knows_the_agile_families(family):
    from dprf_amd import _lib
    first = _lib.plan_chunk(family, 0.0, HUGE, HUGE, 1)
    assert first != 0, "dprf_plan_chunk does not know %s" % family
    assert first % 256 == 0 and first <= 1 << 19
    # a measured rate never sizes a chunk below one resident generation, nor above Office's largest chunk
    for rate in (0.05, 1.0, 100.0, 1e5):
        n = _lib.plan_chunk(family, rate, HUGE, HUGE, 1)
        assert n % 256 == 0 and 1 << 18 <= n <= 1 << 20, (rate, n)
    assert _lib.plan_chunk(family, 0.0, 1000, HUGE, 1) == 1000
    assert _lib.plan_chunk("office_std", 0.0, HUGE, HUGE, 1) == 1 << 19           # the 2007 family as before
    assert _lib.lib().dprf_abi_version() == 9                                     # no export or struct changed


def test_header_documents_the_agile_stream():
    text = open(os.path.join(REPO, "include", "dprf.h")).read()
    for family in FAMILIES:
        assert '"%s"' % family in text
    assert "fe a7 d2 76 3b 4b 9e 79" in text and "d7 aa 0f 6d 30 61 34 4e" in text
    assert re.search(r"#define DPRF_ABI_VERSION 9\b", text)
    assert "DPRF_E_PWLEN" in text and "32 UTF-16 units" in text


def test_resource_gate_holds_the_agile_kernels_at_zero():
    sys.path.insert(0, CSRC)
    try:
        import resource_gate
    finally:
        sys.path.remove(CSRC)
    for k in ("k_agile_kdf", "k_agile_check"):
        assert resource_gate.SCRATCH_LIMIT.get(k) == 0, k


def test_built_object_reports_no_scratch():
    gate = os.path.join(REPO, "build", "obj", "dprf_kernels_agile.o.gate")
    assert os.path.exists(gate), "no gate report of the Agile object: run build() first"
    rows = [ln.split() for ln in open(gate).read().splitlines() if ln.strip()]
    seen = set()
    for r in rows:
        assert r[0] == "ok", r
        name = " ".join(r[1:r.index("VGPRs")])
        assert r[r.index("scratch") + 1] == "0", r
        seen.add(re.sub(r"^void ", "", name).split("<")[0])
    assert seen == {"k_agile_kdf", "k_agile_check"}
    # two candidate sources x two hashes, two hashes x two key sizes
    assert len(rows) == 8
