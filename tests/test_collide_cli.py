"""The password search for a known key without a device: the exports, how a key is spelled, the CLI's flag rules, the
checkpoint's identity and the hint a key search ends with."""
import contextlib
import io
import json

import pytest

import key40_model as km
from dprf_amd import _lib, brute_force, key40


def test_library_exports_the_setter_and_the_getter():
    L = _lib.lib()
    for name in ("dprf_ctx_set_key40", "dprf_ctx_key40"):
        assert hasattr(L, name) and name in _lib.ADDITIVE_EXPORTS
    assert L.dprf_abi_version() == 9 == _lib.ABI_VERSION          # additive: the ABI version stays
    for name in ("set_key40", "key40"):
        assert hasattr(_lib.Context, name)
    # null contexts are refused, not dereferenced
    assert L.dprf_ctx_set_key40(None, b"\0" * 5) == _lib.E_INVALID
    assert L.dprf_ctx_key40(None, None) == _lib.E_INVALID


GOOD = [("91b2e062b9", "91b2e062b9"), ("91B2E062B9", "91b2e062b9"), (bytes.fromhex("00000000ff"), "00000000ff"),
        (bytearray(5), "0000000000")]
BAD = ["91b2e062b", "91b2e062b9a", "zzzzzzzzzz", "0x91b2e062", " 91b2e062b9", "", b"\0" * 4, b"\0" * 6, 5, 0x91b2e062b9,
       None, ["91b2e062b9"], (1, 2, 3, 4, 5)]


@pytest.mark.parametrize("key,want", GOOD, ids=repr)
def test_key_spelling(key, want):
    assert key40.known_key(key).hex() == want == _lib._key40_bytes(key).hex()


@pytest.mark.parametrize("key", BAD, ids=repr)
def test_anything_else_is_a_value_error_before_ctypes(key):
    """Context.set_key40 and Context(key40=...) judge the key before they touch the handle or the fields (so this runs
    without a context); None clears in set_key40, but is no key elsewhere."""
    with pytest.raises(ValueError):
        key40.known_key(key)
    if key is None:
        return
    with pytest.raises(ValueError):
        _lib._key40_bytes(key)
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._h = None
    with pytest.raises(ValueError):
        ctx.set_key40(key)
    with pytest.raises(ValueError):
        _lib.Context(None, key40=key)
    with pytest.raises(ValueError):
        brute_force.init("no stream is parsed", 3, None, key=key)


@pytest.mark.parametrize("extra,named", [(["--owner"], "--owner"), (["--key40"], "--key40"),
                                         (["--key40", "0000000000-00000000ff"], "--key40")], ids=" ".join)
@pytest.mark.parametrize("source", [["-pr", "3"], ["--mask", "?d?d"], ["--wordlist", "w.txt"]], ids=" ".join)
def test_key_with_owner_or_key40_is_a_usage_error(extra, named, source, capsys):
    """argparse's usage error: exit status 2 and a message that names both flags, before the document is opened (the
    file does not exist).  --key40 refuses every candidate source too, so it is tried bare as well."""
    for argv in (source + ["--key", "91b2e062b9"] + extra, ["--key", "91b2e062b9"] + extra):
        with pytest.raises(SystemExit) as ei:
            brute_force.main(["3", "/nonexistent/none.pdf"] + argv)
        assert ei.value.code == 2
        err = capsys.readouterr().err
        assert "--key" in err and named in err and "cannot be combined" in err


@pytest.mark.parametrize("bad", ["91b2e062b", "91b2e062b9a", "zzzzzzzzzz", ""])
def test_a_malformed_key_is_a_usage_error(bad, capsys):
    with pytest.raises(SystemExit) as ei:
        brute_force.main(["3", "/nonexistent/none.pdf", "-pr", "3", "--key", bad])
    assert ei.value.code == 2
    assert "--key" in capsys.readouterr().err


def test_init_refuses_owner_with_a_key_before_the_stream_is_parsed():
    with pytest.raises(ValueError, match="--owner"):
        brute_force.init("no stream is parsed", 3, None, owner=True, key="91b2e062b9")


def test_checkpoint_identity_includes_the_key(tmp_path):
    """A known-key search's cursor belongs to its key: another key's file, a document search's, an owner search's and a
    key search's are each refused, in both directions; range, mask, hybrid and rule searches alike."""
    f = km.base_documents()["pdf_r2"]
    k1, k2 = bytes.fromhex("91b2e062b9"), bytes.fromhex("91b2e062ba")
    assert brute_force._target(False, None) == "user" and brute_force._target(True, None) == "owner"
    assert brute_force._target(False, k1) == "key40:91b2e062b9"
    shapes = [dict(charset="abc", pwlen=3), dict(mask="?d?d"), dict(mask="?w?d", wordlist=("00" * 32, 7)),
              dict(mask="?w", wordlist=("00" * 32, 7), rules=("11" * 32, 3))]
    for n, shape in enumerate(shapes):
        path = str(tmp_path / ("cursor%d.json" % n))

        def cp(target):
            return brute_force.Checkpoint(path, f, target=target, **shape)

        mine = cp(brute_force._target(False, k1))
        assert mine.load() == (0, None)
        mine.save(40)
        assert json.load(open(path))["target"] == "key40:91b2e062b9"
        assert cp("key40:91b2e062b9").load() == (40, None)
        for other in (cp("key40:" + k2.hex()), cp("user"), cp("owner"),
                      brute_force.Checkpoint(path, f, key_window=(0, 0xfff))):
            with pytest.raises(ValueError, match="different search"):
                other.load()
        for target in ("user", "owner", "key40:" + k2.hex()):
            cp(target).save(5)
            with pytest.raises(ValueError, match="different search"):
                mine.load()
        mine.save(50, "found")
        assert mine.load() == (50, "found")


def test_a_finished_checkpoint_answers_without_a_device(tmp_path):
    """init(..., key=...) loads the cursor first: a finished one answers, another key's raises, both without a context."""
    f = km.base_documents()["office_md5"]
    stream = km.stream_of(f)
    with contextlib.redirect_stdout(io.StringIO()):
        fields = brute_force.parse_verification_data(stream)
    path = str(tmp_path / "cursor.json")
    brute_force.Checkpoint(path, fields, "abc", 3, target="key40:91b2e062b9").save(9, "cab")
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert brute_force.init(stream, 3, None, charset="abc", checkpoint=path, key="91B2E062B9") == (1, "cab")
    assert "already finished" in out.getvalue()
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(ValueError, match="different search"):
        brute_force.init(stream, 3, None, charset="abc", checkpoint=path, key="91b2e062ba")
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(ValueError, match="different search"):
        brute_force.init(stream, 3, None, charset="abc", checkpoint=path)


def test_the_hint_after_a_key_search(tmp_path):
    """A key search that has found its key says how the key becomes a password: the command-line flag and the key.  The
    finished checkpoint answers without a device."""
    f = km.base_documents()["pdf_r34"]
    path = str(tmp_path / "cursor.json")
    brute_force.Checkpoint(path, f, key_window=(0, 0xfff)).save(0x800, "00000007ff")
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert brute_force.init_key40_brute_force(f, (0, 0xfff), checkpoint=path) == (1, "00000007ff")
    assert "--key 00000007ff" in out.getvalue()
    assert "--key %s" in key40.KEY_HINT and "%s" in key40.COLLISION_NOTE
    note = key40.COLLISION_NOTE % "00000007ff"
    assert "00000007ff" in note and "not necessarily" in note


def test_report_adds_the_collision_note_only_with_a_key(capsys):
    brute_force._report("cab", 10, 0.0)
    assert "not necessarily" not in capsys.readouterr().out
    brute_force._report("cab", 10, 0.0, False, bytes.fromhex("16d00f0376"))
    out = capsys.readouterr().out
    assert "Correct password is 'cab'" in out and "16d00f0376" in out and "not necessarily" in out
    brute_force._report(None, 10, 0.0, False, bytes.fromhex("16d00f0376"))
    assert "not necessarily" not in capsys.readouterr().out
