"""Owner-password search (ABI 9) without a GPU: the header and the library carry the two entry points, the chunk policy
knows the three owner families, the CLI refuses --owner for a document that is not a PDF before any device work, and
a checkpoint of one password kind is not loaded by a search for the other."""
import contextlib
import io
import json
import os
import re

import pytest

from conftest import REPO


def _header():
    with open(os.path.join(REPO, "include", "dprf.h")) as f:
        return f.read()


def test_header_declares_and_library_exports():
    from dprf_amd import _lib
    h = _header()
    assert re.search(r"#define\s+DPRF_PDF_USER\s+0\b", h) and re.search(r"#define\s+DPRF_PDF_OWNER\s+1\b", h)
    assert re.search(r"int\s+dprf_ctx_set_pdf_password\s*\(\s*dprf_ctx\s*\*\s*ctx\s*,\s*int\s+which\s*\)\s*;", h)
    assert re.search(r"int\s+dprf_ctx_pdf_password\s*\(\s*const\s+dprf_ctx\s*\*\s*ctx\s*\)\s*;", h)
    assert re.search(r"#define\s+DPRF_ABI_VERSION\s+9\b", h)
    L = _lib.lib()
    for name in ("dprf_ctx_set_pdf_password", "dprf_ctx_pdf_password"):
        assert name in _lib.EXPORTS
        assert getattr(L, name) is not None


def test_abi_version_is_9():
    from dprf_amd import _lib
    assert _lib.ABI_VERSION == 9
    assert _lib.lib().dprf_abi_version() == 9


@pytest.mark.parametrize("family", ["pdf_r24", "pdf_r5", "pdf_r6"])
def test_plan_chunk_knows_the_owner_families(family):
    from dprf_amd import _lib
    n = 1 << 30
    user = _lib.plan_chunk(family, 0.0, n, n, 1)
    owner = _lib.plan_chunk(family + "_owner", 0.0, n, n, 1)
    assert owner > 0
    assert owner <= user
    # a measured rate sizes the later chunks as it does for the user family
    assert _lib.plan_chunk(family + "_owner", 1e4, n, n, 1) == _lib.plan_chunk(family, 1e4, n, n, 1)


def test_null_context_is_invalid():
    from dprf_amd import _lib
    L = _lib.lib()
    assert L.dprf_ctx_set_pdf_password(None, 1) == _lib.E_INVALID
    assert L.dprf_ctx_pdf_password(None) == _lib.E_INVALID


def test_cli_refuses_owner_for_a_non_pdf(monkeypatch, capsys):
    from dprf_amd import brute_force as bf

    def no_device_work(*a, **k):
        raise AssertionError("the refusal must come before the document is parsed or a device is opened")

    monkeypatch.setattr(bf, "get_verification_data", no_device_work)
    monkeypatch.setattr(bf, "_context", no_device_work)
    with pytest.raises(SystemExit) as ei:
        bf.main(["1", "x.docx", "--owner", "-pr", "3"])
    assert ei.value.code not in (0, None)
    err = capsys.readouterr().err
    assert "--owner" in err and "PDF" in err


def test_init_refuses_owner_for_a_non_pdf_stream(streams, monkeypatch):
    from dprf_amd import brute_force as bf
    monkeypatch.setattr(bf, "_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError):
            bf.init(streams["office_testdoc"]["stream"], 3, None, owner=True)


def test_checkpoints_of_the_two_password_kinds_do_not_mix(tmp_path):
    from dprf_amd import brute_force as bf
    fields = ["pdf", "4", "4", "128", "-3904", "1", "16", "00" * 16, "32", "11" * 32, "32", "22" * 32]
    user_file, owner_file, old_file = (os.path.join(str(tmp_path), n) for n in ("u.json", "o.json", "old.json"))
    user = bf.Checkpoint(user_file, fields, "abc", 3)
    owner = bf.Checkpoint(owner_file, fields, "abc", 3, target="owner")
    user.save(17)
    owner.save(23)
    # a user search's key is what it was before owner mode existed
    with open(user_file) as f:
        assert "target" not in json.load(f)
    with open(owner_file) as f:
        assert json.load(f)["target"] == "owner"
    assert user.load() == (17, None) and owner.load() == (23, None)
    with pytest.raises(ValueError):
        bf.Checkpoint(owner_file, fields, "abc", 3).load()                    # user search, owner file
    with pytest.raises(ValueError):
        bf.Checkpoint(user_file, fields, "abc", 3, target="owner").load()     # owner search, user file
    # a file written before the target existed counts as a user search's
    with open(old_file, "w") as f:
        json.dump(dict(user.key, next_index=5, found=None), f)
    assert bf.Checkpoint(old_file, fields, "abc", 3).load() == (5, None)
    with pytest.raises(ValueError):
        bf.Checkpoint(old_file, fields, "abc", 3, target="owner").load()
    # the mask form carries the target too
    m = bf.Checkpoint(owner_file, fields, mask="?l?l", custom=(), target="owner")
    assert m.key["target"] == "owner" and "target" not in bf.Checkpoint(owner_file, fields, mask="?l?l").key
