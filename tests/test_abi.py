"""The C-ABI library loads and exports every symbol include/dprf.h declares (no compute without a GPU)."""
import ctypes
import os
import re

import pytest

from conftest import REPO


def declared_symbols():
    hdr = open(os.path.join(REPO, "include", "dprf.h")).read()
    return sorted(set(re.findall(r"\b(dprf_[a-z_]+)\s*\(", hdr)))


def test_header_and_python_binding_agree():
    from dprf_amd import _lib
    assert declared_symbols() == sorted(_lib.EXPORTS)


def test_library_exports_every_declared_symbol():
    from dprf_amd import _lib
    L = _lib.lib()
    for name in declared_symbols():
        assert hasattr(L, name), name
    assert L.dprf_abi_version() == _lib.ABI_VERSION


def test_constants_match_header():
    from dprf_amd import _lib
    hdr = open(os.path.join(REPO, "include", "dprf.h")).read()
    consts = dict((k, int(v)) for k, v in re.findall(r"#define (DPRF_\w+) \(?(-?\d+)\)?", hdr))
    assert consts["DPRF_ABI_VERSION"] == _lib.ABI_VERSION
    assert consts["DPRF_E_DOMAIN"] == _lib.E_DOMAIN and consts["DPRF_E_NODEVICE"] == _lib.E_NODEVICE
    assert consts["DPRF_MAX_PW"] == _lib.MAX_PW and consts["DPRF_MAX_PW_RANGE"] == _lib.MAX_PW_RANGE
    assert consts["DPRF_FLAG_NEVER_MATCHES"] == _lib.FLAG_NEVER_MATCHES


def test_no_device_is_an_error_not_a_fallback():
    """Without a GPU, creating a context must fail loudly (DPRF_E_NODEVICE) -- there is no CPU path."""
    from dprf_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_lib.DprfError) as ei:
        _lib.Context(["pdf", "1", "2", "40", "-64", "1", "16", "11" * 16, "32", "22" * 32, "32", "33" * 32])
    assert ei.value.code == _lib.E_NODEVICE


def test_product_does_not_import_the_oracle():
    """Nothing under dprf_amd/ may import, load or execute oracle/ (it is the checker)."""
    for root, _, files in os.walk(os.path.join(REPO, "dprf_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                src = open(os.path.join(root, f), errors="replace").read()
                assert "pyoracle" not in src and "liboracle" not in src and "oracle.h" not in src, f


def test_makefile_tracks_every_local_header():
    """Every header a kernel or host source includes is a make dependency and part of the build fingerprint
    (HDRS): round 3 once shipped a stale object because the generated rc4_ksa_asm.h was missing there, so the
    library -- and its dprf_build_id() -- did not change when the header did."""
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dprf_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    hdrs = set(re.search(r"^HDRS\s*:=\s*(.*)$", mk, re.M).group(1).split())
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".cpp", ".h")):
            for inc in re.findall(r'^#include "([^"]+)"', open(os.path.join(csrc, f)).read(), re.M):
                if inc == "build_id.h":
                    continue                      # generated into OBJDIR by the Makefile itself
                assert inc in hdrs, (f, inc)


def test_candidate_source_is_defined_once():
    """dprf_cand.h is the only definition of the candidate source and the block prologue: the enumeration order, the
    lowest-hit rule and the full-slot terminator were each a bug once, and four hand-kept copies had drifted."""
    csrc = os.path.join(REPO, "dprf_amd", "csrc")
    text = dict((f, open(os.path.join(csrc, f)).read()) for f in sorted(os.listdir(csrc))
                if f.endswith((".hip", ".cpp", ".h")))
    assert "dprf_cand.h" in text
    # a definition: `struct cand {`, or the name after a return type at the start of a line (a call is indented)
    defs = {"struct cand": r"^\s*struct\s+cand\b[^;]*\{"}
    for name in ("range_candidate", "list_candidate", "block_prologue"):
        defs[name] = r"^(?:DEVI|__device__|static|inline)[^;(]*\b%s\s*\(" % name
    for what, pat in defs.items():
        where = [(f, len(re.findall(pat, src, re.M))) for f, src in text.items() if re.search(pat, src, re.M)]
        assert where == [("dprf_cand.h", 1)], (what, where)
    for f, src in text.items():
        if not f.endswith(".hip"):
            continue
        for gone in ("block_runs", "be_append_salted"):      # the renamed copies: neither defined nor called
            assert not re.search(r"\b%s\s*[<(]" % gone, src), (f, gone)
        if re.search(r"\bget_candidate\s*<", src):
            assert re.search(r'^#include "dprf_cand\.h"', src, re.M), f


def test_r24_shared_definitions():
    """What PDF R2-R4's two kernels share has one definition: the padded-password builder and the user-key chain
    (r24_key is the two in a row; it used to restate both), the PAD tail and the verdict check as functions, and the
    workgroup frame of the user kernel in rc4_wg.h, whose driver the user kernel runs on.  k_pdf_r24_owner and
    k_oldoffice keep the frame -- and the owner kernel the check stage -- written out, because on the shared code
    they measured slower (HISTORY.md): the copies that remain are counted here, so a further one shows."""
    csrc = os.path.join(REPO, "dprf_amd", "csrc")
    text = dict((f, open(os.path.join(csrc, f)).read()) for f in sorted(os.listdir(csrc))
                if f.endswith((".hip", ".cpp", ".h")))
    assert "rc4_wg.h" in text

    def defined(pat):
        return [(f, len(re.findall(pat, src, re.M))) for f, src in text.items() if re.search(pat, src, re.M)]
    func = r"^(?:DEVI|__device__|static|inline)[^;(]*\b%s\s*\("
    for name in ("r24_check", "r24_padded_pw", "r24_user_key", "r24_key", "r24_padtail"):
        assert defined(func % name) == [("dprf_kernels.hip", 1)], name
    for name in ("rc4_wg_geometry", "rc4_wg_put", "rc4_wg_get", "rc4_wg_sbox_base", "rc4_wg_lane_id", "rc4_wg_run"):
        assert defined(func % name) == [("rc4_wg.h", 1)], name
    kern = text["dprf_kernels.hip"]
    # r24_key composes the two builders and holds no MD5 of its own
    body = re.search(r"\bDEVI void r24_key\s*\([^{]*\{(.*?)\n\}", kern, re.S).group(1)
    assert "r24_padded_pw<" in body and "r24_user_key<" in body and "md5_compress" not in body
    # the user-key chain and the list-mode padding have no second copy: both kernels call the shared ones
    assert len(re.findall(r"\br24_user_key\s*<", kern)) == 2 and len(re.findall(r"\br24_padded_pw\s*<", kern)) == 2
    # the user kernel runs on the driver
    assert re.search(r"\brc4_wg_run<", kern) and re.search(r'^#include "rc4_wg\.h"', kern, re.M)
    # the remaining hand copies: the verdict stage (r24_check and the owner kernel's stage C) and the lane-id asm
    # (rc4_wg.h, the owner kernel, k_oldoffice; dprf_kernels_r6.hip has a v_mbcnt of its own, for another purpose)
    assert defined(r"\brc4_prga_span\s*<\s*1\s*,\s*4\s*>\s*\(") == [("dprf_kernels.hip", 2)]
    assert [d for d in defined(r"v_mbcnt_lo_u32_b32") if d[0] != "dprf_kernels_r6.hip"] == \
        [("dprf_kernels.hip", 1), ("dprf_kernels_oldoffice.hip", 1), ("rc4_wg.h", 1)]


def test_family_table_is_the_one_place_that_knows_a_family():
    """What the host knows of a kernel family is one row of FAMILIES in dprf_doc.cpp: every family name is written once
    in the host sources, the per-family refusal sentences live in the document unit only, and that unit is free of
    HIP, so a plain C++ compiler builds it (tests/test_doc_layer.py does)."""
    csrc = os.path.join(REPO, "dprf_amd", "csrc")
    text = dict((f, open(os.path.join(csrc, f)).read()) for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".h")))
    names = ["office_std", "odf_aes256", "odf_bf_sha1", "office_agile_sha1", "office_agile_sha512", "office_rc4_md5",
             "office_rc4_sha1", "pdf_r24", "pdf_r5", "pdf_r6", "pdf_r24_owner", "pdf_r5_owner", "pdf_r6_owner"]
    for name in names:
        where = [(f, src.count('"%s"' % name)) for f, src in text.items() if '"%s"' % name in src]
        assert where == [("dprf_doc.cpp", 1)], (name, where)
    for f in ("dprf_doc.cpp", "dprf_doc.h"):
        assert not re.search(r"\bhip", text[f], re.I), f                # hipMalloc, hip_runtime.h, HIPCHK, "HIP"
    assert [f for f, src in text.items() if "not supported yet" in src] == ["dprf_doc.cpp"]
    # the per-kind helpers are gone from the device half, which asks status_text for a sentence and holds none
    for gone in ("is_agile", "is_oldoffice", "slot_trunc", "two_kernels", "key_words(", "*status_text", "*kind_name"):
        assert gone not in text["dprf_host.cpp"], gone


def test_ctypes_structs_match_the_header_layout(tmp_path):
    """dprf_stats / dprf_device_stats as a C compiler lays them out (include/dprf.h) == the ctypes mirrors (ABI 6
    appended hit_ms and evaluated): sizes and every field offset."""
    import subprocess
    from dprf_amd import _lib
    src = tmp_path / "layout.c"
    fields = {"dprf_stats": [f for f, _ in _lib.Stats._fields_],
              "dprf_device_stats": [f for f, _ in _lib.DeviceStats._fields_]}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dprf.h"', "int main(void) {"]
    for t, fs in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (t, t))
        for f in fs:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (t, f, t, f))
    lines.append("return 0; }")
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if ln)
    for t, cls in (("dprf_stats", _lib.Stats), ("dprf_device_stats", _lib.DeviceStats)):
        assert int(got[t]) == ctypes.sizeof(cls), t
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (t, f)]) == getattr(cls, f).offset, (t, f)
