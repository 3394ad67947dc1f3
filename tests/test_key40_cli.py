"""The 40-bit key search without a device: the export, the chunk planner's names, the window grammar, the CLI's flag
rules and the checkpoint's identity."""
import json

import pytest

import key40_model as km
from dprf_amd import _lib, brute_force, key40


def test_library_exports_the_key_search():
    L = _lib.lib()
    assert hasattr(L, "dprf_search_key40")
    assert L.dprf_abi_version() == 9 == _lib.ABI_VERSION          # additive: the ABI version stays
    assert _lib.KEY40_SPACE == 1 << 40 == key40.SPACE
    assert hasattr(_lib.Context, "search_key40")


@pytest.mark.parametrize("name,parent", [("pdf_r24_key40", "pdf_r24"), ("office_rc4_md5_key40", "office_rc4_md5"),
                                         ("office_rc4_sha1_key40", "office_rc4_sha1")])
def test_plan_chunk_knows_the_key_search_families(name, parent):
    assert _lib.plan_chunk(name, 0.0, 1 << 40, 1 << 40, 1) != 0
    for rate, remaining, total, ndev, inflight in ((0.0, 1 << 40, 1 << 40, 1, 0), (8e6, 1 << 40, 1 << 40, 8, 0),
                                                   (8e6, 1 << 21, 1 << 30, 8, 1)):
        assert _lib.plan_chunk(name, rate, remaining, total, ndev, inflight) == \
            _lib.plan_chunk(parent, rate, remaining, total, ndev, inflight)
    assert _lib.plan_chunk("pdf_r5_key40", 0.0, 1, 1, 1) == 0


def test_parse_window():
    assert key40.parse_window(None) == key40.parse_window("") == (0, (1 << 40) - 1)
    assert key40.parse_window("0000000000-3fffffffff") == (0, (1 << 38) - 1)
    assert key40.parse_window("91B2E062B9-91b2e062b9") == (0x91b2e062b9, 0x91b2e062b9)
    assert key40.parse_window("00ffffffff-0100000000") == (0xffffffff, 0x100000000)
    for bad in ("0-1", "000000000-0000000001", "0000000000", "0000000001-0000000000", "000000000g-0000000001",
                "0000000000-00000000011", "0000000000 - 0000000001", "0000000000-0000000001-0000000002"):
        with pytest.raises(ValueError):
            key40.parse_window(bad)


def test_key_index_and_bytes():
    assert key40.key_index("91b2e062b9") == 0x91b2e062b9 == key40.key_index(bytes.fromhex("91b2e062b9"))
    for bad in ("91b2e062b", "91b2e062b9a", "zzzzzzzzzz", b"\0" * 4, b"\0" * 6):
        with pytest.raises(ValueError):
            key40.key_index(bad)


def test_a_sentence_per_family():
    docs = km.base_documents()
    got = {fam: key40.family(f) for fam, f in docs.items()}
    assert got == {"pdf_r2": "pdf_r2", "pdf_r34": "pdf_r34", "office_md5": "office_rc4_md5",
                   "office_sha1": "office_rc4_sha1"}
    assert set(key40.SENTENCES) == set(got.values())
    for s in key40.SENTENCES.values():
        assert s.startswith("The five bytes are ")
    assert key40.family(["pdf", "4", "4", "128", "-4", "1", "16", "00" * 16, "32", "00" * 32, "32", "00" * 32]) is None
    assert key40.family(["oldoffice", "4", "", "", ""]) is None and key40.family(["odt"]) is None


FORBIDDEN = [["-pr", "3"], ["--charset", "abc"], ["--mask", "?d?d"], ["--wordlist", "w.txt"],
             ["--wordlist", "w.txt", "--rules", "r.rule"], ["--wordlist", "w.txt", "--rules", "r.rule", "--stdout"],
             ["--stdout"], ["--owner"], ["-1", "abc"]]


@pytest.mark.parametrize("extra", FORBIDDEN, ids=lambda e: " ".join(e))
@pytest.mark.parametrize("key40_arg", [["--key40"], ["--key40", "0000000000-00000000ff"]], ids=["all", "window"])
def test_forbidden_flag_combinations_are_usage_errors(extra, key40_arg, capsys):
    """argparse's usage error: exit status 2 and a message that names --key40, before the document is opened (the file
    does not exist)."""
    with pytest.raises(SystemExit) as ei:
        brute_force.main(["3", "/nonexistent/none.pdf"] + key40_arg + extra)
    assert ei.value.code == 2
    err = capsys.readouterr().err
    assert "--key40" in err and "cannot be combined" in err


@pytest.mark.parametrize("bad", ["0-1", "0000000001-0000000000", "xyz"])
def test_a_malformed_window_is_a_usage_error(bad, capsys):
    with pytest.raises(SystemExit) as ei:
        brute_force.main(["3", "/nonexistent/none.pdf", "--key40", bad])
    assert ei.value.code == 2
    assert "--key40" in capsys.readouterr().err


def test_checkpoint_identity(tmp_path):
    """The cursor belongs to "key40", the stream and the window: another window's file, another stream's and a password
    search's are each refused, in both directions."""
    docs = km.base_documents()
    f = docs["pdf_r2"]
    path = str(tmp_path / "cursor.json")
    cp = brute_force.Checkpoint(path, f, key_window=(0x1000, 0x1fff))
    assert cp.load() == (0, None)
    cp.save(0x1400)
    rec = json.load(open(path))
    assert rec["search"] == "key40" and rec["window"] == [0x1000, 0x1fff] and rec["next_index"] == 0x1400
    assert brute_force.Checkpoint(path, f, key_window=(0x1000, 0x1fff)).load() == (0x1400, None)
    for other in (brute_force.Checkpoint(path, f, key_window=(0x1000, 0x2fff)),
                  brute_force.Checkpoint(path, f, key_window=(0, 0x1fff)),
                  brute_force.Checkpoint(path, docs["pdf_r34"], key_window=(0x1000, 0x1fff)),
                  brute_force.Checkpoint(path, f, "abc", 3),
                  brute_force.Checkpoint(path, f, mask="?d?d")):
        with pytest.raises(ValueError, match="different search"):
            other.load()
    # a password search's file is not a key search's
    brute_force.Checkpoint(path, f, "abc", 3).save(5)
    with pytest.raises(ValueError, match="different search"):
        brute_force.Checkpoint(path, f, key_window=(0x1000, 0x1fff)).load()
    # a finished search answers from the file
    cp.save(0x1500, "0000001499")
    assert cp.load() == (0x1500, "0000001499")


def test_resuming_another_window_is_refused_before_any_device_work(tmp_path):
    """init_key40_brute_force loads the cursor first: a file written for another window raises without a context (no
    GPU is needed to see it)."""
    f = km.base_documents()["office_md5"]
    path = str(tmp_path / "cursor.json")
    brute_force.Checkpoint(path, f, key_window=(0, 0xfff)).save(0x800)
    with pytest.raises(ValueError, match="different search"):
        brute_force.init_key40_brute_force(f, "0000000000-0000001fff", checkpoint=path)
    with pytest.raises(ValueError):
        brute_force.init_key40_brute_force(f, (5, 1 << 40))


def test_python_checks_the_window_before_ctypes():
    """ctypes takes an oversized int modulo 2^64 silently: Context.search_key40 refuses the window itself, before it
    touches the handle (so this runs without a context)."""
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._h = None
    for start, count in ((0, (1 << 40) + 1), (1, 1 << 40), (1 << 64, 1), (0, (1 << 64) + 5), (-1, 2), (0, -1)):
        with pytest.raises(_lib.DprfError) as ei:
            ctx.search_key40(start, count)
        assert ei.value.code == _lib.E_INVALID
