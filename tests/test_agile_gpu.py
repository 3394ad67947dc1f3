"""Office 2010 / 2013 Agile Encryption on the device (k_agile_kdf + k_agile_check, kernel families "office_agile_sha1"
and "office_agile_sha512") against tests/agile_model.py, the Python statement of the definition, which
tests/test_agile_model.py pins on the CPU (public vectors included).  Streams come from agile_model.make_stream with a
small spinCount except in (a); the shapes are the smallest at which these kernels can go wrong.

  (a) the two public vectors at spinCount 100000 (the only place the loop counter passes 65535), one wave
  (b) every (version, keyBits) pair x spinCount {0, 1, 3, 1000}: a 125-candidate range window (no multiple of 64), the
      whole hit set, and stop_on_first
  (c) window edges: 1, 63, 65, 257 and 513 candidates from a non-zero start, the password at either end
  (d) planted lengths in list mode: SHA-1's first message crosses from one block to two at 20 characters, 32 fill the slot
  (e) non-ASCII candidates: list, symbol window, mask
  (f) two and four lanes on one device
  (g) the refusals, after each of which the context or the library still serves
  (h) the family names; the 2007 stream is served as before
  (i) end to end from a document written by agile_docgen: --mask, list mode, -pr / --charset with --checkpoint
  (j) the server and the GPU client on an Agile stream"""
import contextlib
import functools
import io
import json
import os
import zlib

import pytest

import agile_model as M
from conftest import load_golden

pytestmark = pytest.mark.gpu

PAIRS = [("2010", 128), ("2010", 256), ("2013", 128), ("2013", 256)]
FAMILY = {"2010": "office_agile_sha1", "2013": "office_agile_sha512"}
CS5 = "678Ux"
PW = "Ux7"
PW_IDX = M.index_of(PW, CS5)
assert PW_IDX == 96 and M.word(PW_IDX, CS5, 3) == PW


@pytest.fixture(scope="module")
def dprf():
    from dprf_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device: GPU tests need the MI355X box"
    return _lib


def _fields(stream):
    from dprf_amd.brute_force import parse_verification_data
    with contextlib.redirect_stdout(io.StringIO()):
        return parse_verification_data(stream)


@functools.lru_cache(maxsize=None)
def _stream(pw, version, bits, spin):
    """One stream per (password, version, keyBits, spinCount), made once and shared."""
    s = M.make_stream(pw, version, bits, spin, seed=zlib.crc32(repr((pw, version, bits, spin)).encode()))
    assert M.verifies(s, pw)
    return s


# ---------------------------------------------------------------- (a) public vectors, spinCount 100000
@pytest.mark.parametrize("name", ["office_2010_hashcat", "office_2013_hashcat"])
def test_public_vectors(dprf, name):
    v = load_golden("agile_vectors.json")[name]
    f = _fields("hashcat:" + v["stream"])
    assert f[2] == "100000"
    with dprf.Context(f, device=0) as ctx:
        assert ctx.kernel == FAMILY[f[1]] and ctx.flags == 0
        hits, n, st = ctx.verify_list(["hashca", "hashcat", "hashcatx", "Hashcat"])
        assert hits == [1] and n == 1 and st["candidates"] == 4


# ---------------------------------------------------------------- (b) range windows, every pair x spin
@pytest.mark.parametrize("version,bits", PAIRS)
@pytest.mark.parametrize("spin", [0, 1, 3, 1000])
def test_range_window(dprf, version, bits, spin):
    s = _stream(PW, version, bits, spin)
    assert M.verifies(s, M.word(PW_IDX, CS5, 3))
    assert not M.verifies(s, M.word(PW_IDX - 1, CS5, 3)) and not M.verifies(s, M.word(PW_IDX + 1, CS5, 3))
    with dprf.Context(_fields(s), device=0) as ctx:
        assert ctx.kernel == FAMILY[version]
        hits, n, st = ctx.search_range(CS5, 3, 0, 125)
        assert hits == [PW_IDX] and n == 1 and st["candidates"] == 125
        first, n1, _ = ctx.search_range(CS5, 3, 0, 125, stop_on_first=True, cap=1)
        assert first == [PW_IDX] and n1 >= 1


# ---------------------------------------------------------------- (c) window edges
@pytest.mark.parametrize("version,bits", [("2013", 256), ("2010", 128)])
@pytest.mark.parametrize("count", [1, 63, 65, 257, 513])
def test_window_edges(dprf, version, bits, count):
    start = 1009                                            # 5^5 = 3125 candidates; 1009 + 513 stays inside
    for idx in sorted({start, start + count - 1}):
        pw = M.word(idx, CS5, 5)
        s = _stream(pw, version, bits, 3)
        with dprf.Context(_fields(s), device=0) as ctx:
            hits, n, st = ctx.search_range(CS5, 5, start, count)
            assert hits == [idx] and n == 1 and st["candidates"] == count, (idx, hits)
            first, _, _ = ctx.search_range(CS5, 5, start, count, stop_on_first=True, cap=1)
            assert first == [idx]
            # one candidate to either side of the password and the window misses it
            if idx == start and count > 1:
                assert ctx.search_range(CS5, 5, start + 1, count - 1)[0] == []
            if idx == start + count - 1 and count > 1:
                assert ctx.search_range(CS5, 5, start, count - 1)[0] == []


# ---------------------------------------------------------------- (d) planted lengths, list mode
def _planted(L):
    return "".join(chr(33 + (7 * k + 5 * L + k * k) % 90) for k in range(L))


@pytest.mark.parametrize("version,bits", [("2010", 128), ("2013", 256)])
@pytest.mark.parametrize("L", [1, 19, 20, 27, 28, 31, 32])
def test_planted_lengths(dprf, version, bits, L):
    pw = _planted(L)
    s = _stream(pw, version, bits, 3)
    # decoys one character shorter and longer; the empty candidate (below 1) and a 33-character one (above the slot)
    # are refusals, tested in (g) -- at those ends a decoy of the same length with its last character changed stands in
    shorter = pw[:-1] if L > 1 else "~"
    longer = pw + "x" if L < 32 else pw[:-1] + "~"
    words = [shorter, longer, pw, pw[:-1] + "}"]
    assert [k for k, w in enumerate(words) if M.verifies(s, w)] == [2]
    total = M.first_message_len(pw)
    assert total == 16 + 2 * L
    if version == "2010":
        assert (total > 55) == (L >= 20)                    # SHA-1: one block below 20 characters, two from there on
    else:
        assert total + 17 <= 128                            # SHA-512: one block throughout
    with dprf.Context(_fields(s), device=0) as ctx:
        hits, n, _ = ctx.verify_list(words)
        assert hits == [2] and n == 1


# ---------------------------------------------------------------- (e) non-ASCII candidates
@pytest.mark.parametrize("version,bits", [("2010", 256), ("2013", 128)])
def test_non_ascii_list(dprf, version, bits):
    words = ["été", "日本語", "\U0001F600ok", "ete", "日本", "ok"]
    for k in range(3):
        s = _stream(words[k], version, bits, 3)
        assert [j for j, w in enumerate(words) if M.verifies(s, w)] == [k]
        with dprf.Context(_fields(s), device=0) as ctx:
            assert ctx.verify_list(words)[0] == [k]
            assert ctx.verify_list([w.encode("utf-8") for w in words])[0] == [k]


@pytest.mark.parametrize("version,bits", [("2010", 128), ("2013", 256)])
def test_symbol_window_and_mask(dprf, version, bits):
    from dprf_amd import mask as masks
    charset = "aé"
    pw = "éaé"
    idx = M.index_of(pw, charset)
    s = _stream(pw, version, bits, 3)
    assert [k for k in range(8) if M.verifies(s, M.word(k, charset, 3))] == [idx]
    with dprf.Context(_fields(s), device=0) as ctx:
        assert ctx.search_symbols(charset, 3, 0, 8)[0] == [idx]
        assert ctx.search_symbols(charset, 3, idx, 1, stop_on_first=True, cap=1)[0] == [idx]
        assert ctx.search_symbols(charset, 3, 0, idx)[0] == []
    positions = masks.parse_mask("U?1?d", ("xé",))
    assert masks.space(positions) == 20
    mpw = "Ué7"
    midx = masks.index_of(positions, mpw)
    assert midx == 17 and masks.word(positions, midx) == mpw
    s = _stream(mpw, version, bits, 3)
    assert [k for k in range(20) if M.verifies(s, masks.word(positions, k))] == [midx]
    with dprf.Context(_fields(s), device=0) as ctx:
        assert ctx.search_mask(positions, 0, 20)[0] == [midx]


# ---------------------------------------------------------------- (f) lanes on one device
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]])
def test_lanes_on_one_device(dprf, devices):
    s = _stream(PW, "2013", 256, 1000)
    with dprf.Context(_fields(s), devices=devices) as ctx:
        hits, n, st = ctx.search_range(CS5, 3, 0, 125)
        assert hits == [PW_IDX] and n == 1 and st["candidates"] == 125
        first, _, _ = ctx.search_range(CS5, 3, 0, 125, stop_on_first=True, cap=1)
        assert first == [PW_IDX]
        assert [d["device"] for d in ctx.last_call_devices()] == devices


# ---------------------------------------------------------------- (g) refusals
def _serves(dprf, s):
    with dprf.Context(_fields(s), device=0) as ctx:
        assert ctx.verify_list([PW, "Ux8"])[0] == [0]


def refusal_base():
    """The stream the refused ones are made from, and its fields."""
    good = _stream(PW, "2013", 256, 1000)
    return good, _fields(good)


def bad_streams(base):
    """What is refused, as changes to `base`: label -> (field index, value, the field name the message carries or
    None).  tests/test_doc_layer.py runs the same list through the document layer without a device."""
    return {
        "keyBits 192": (3, "192", "keyBits"),
        "saltSize 8": (4, "8", "saltSize"),
        "spinCount 10,000,001": (2, "10000001", "spinCount"),
        "30-digit verifier input": (6, base[6][:30], "encryptedVerifierHashInput"),
        # any version but "2010" / "2013" is read as the 2007 stream, where field 2 is the verifier hash size: 1000
        # lies outside it
        "version 2016": (1, "2016", None),
    }


def test_stream_refusals(dprf):
    good, base = refusal_base()
    bad = bad_streams(base)
    for what, (k, v, _) in bad.items():
        f = list(base)
        f[k] = v
        with pytest.raises(dprf.DprfError) as ei:
            dprf.Context(f, device=0)
        assert ei.value.code == dprf.E_DOMAIN, what
        _serves(dprf, good)
    for k, v, name in bad.values():
        if name is None:
            continue
        f = list(base)
        f[k] = v
        with pytest.raises(dprf.DprfError) as ei:
            dprf.Context(f, device=0)
        assert name in str(ei.value), (name, str(ei.value))      # the message names the field


@pytest.mark.parametrize("version,bits", [("2010", 128), ("2013", 256)])
def test_candidate_refusals(dprf, version, bits):
    import numpy as np
    s = _stream(PW, version, bits, 3)
    words = [PW.encode(), b"y" * 33, b"z" * 32, b""]
    blob = b"".join(words)
    offs = np.cumsum([0] + [len(w) for w in words]).astype(np.uint64)
    with dprf.Context(_fields(s), device=0) as ctx:
        with pytest.raises(dprf.DprfError) as ei:
            ctx.verify_list(words[:3])
        assert ei.value.code == dprf.E_PWLEN and "not supported yet" in str(ei.value)
        assert list(ctx.list_status(blob, offs)) == [0, dprf.E_PWLEN, 0, dprf.E_DOMAIN]
        assert ctx.verify_list([words[0], words[2]])[0] == [0]                 # the context still serves
        with pytest.raises(dprf.DprfError) as ei:
            ctx.verify_list([PW, ""])
        assert ei.value.code == dprf.E_DOMAIN
        with pytest.raises(dprf.DprfError) as ei:
            ctx.verify_list([PW.encode(), b"\xff\xfe"])                        # invalid UTF-8
        assert ei.value.code == dprf.E_DOMAIN
        with pytest.raises(dprf.DprfError) as ei:
            ctx.search_range("aé".encode("utf-8"), 2, 0, 4)                    # Office: ASCII-only range charset
        assert ei.value.code == dprf.E_CHARSET
        assert ctx.search_range(CS5, 3, 0, 125)[0] == [PW_IDX]


# ---------------------------------------------------------------- (h) family names; the 2007 stream as before
def test_family_names_and_the_2007_stream(dprf, streams, hitsets):
    for version, bits in PAIRS:
        with dprf.Context(_fields(_stream(PW, version, bits, 3)), device=0) as ctx:
            assert ctx.kernel == FAMILY[version] and ctx.flags == 0 and ctx.format == 1
    h = hitsets["office_synth_ok/lower^2"]
    with dprf.Context(_fields(streams["office_synth_ok"]["stream"]), device=0) as ctx:
        assert ctx.kernel == "office_std"
        hits, _, st = ctx.search_range(h["charset"], h["pwlen"], h["start"], h["count"])
        assert hits == h["hits"] == [374] and st["candidates"] == 676


# ---------------------------------------------------------------- (i) end to end from a document
def test_document_end_to_end(dprf, tmp_path):
    import agile_docgen
    from dprf_amd import brute_force
    path = os.path.join(str(tmp_path), "modern.docx")
    agile_docgen.write_docx_agile(path, PW, 0xD0C, version="2013", key_bits=256, spin=1000)
    with contextlib.redirect_stdout(io.StringIO()):
        assert brute_force.main(["1", path, "--mask", "U?l?d", "--devices", "0"]) == (1, PW)
        stream = brute_force.get_verification_data("1", path)
        fields = brute_force.parse_verification_data(stream)
        assert fields[1] == "2013" and M.verifies(stream, PW)
        assert brute_force.init_listbased_brute_force(fields, ["Ux6", "ux7", PW, "Ux8"], devices=[0]) == (1, PW)
        assert brute_force.init_listbased_brute_force(fields, ["Ux6", "ux7"], devices=[0])[0] == 0
        # -pr / --charset with a checkpoint: the cursor file records the search and its result
        cp = os.path.join(str(tmp_path), "cursor.json")
        argv = ["1", path, "-pr", "3", "--charset", CS5, "--devices", "0", "--checkpoint", cp]
        assert brute_force.main(argv) == (1, PW)
        assert json.load(open(cp))["found"] == PW
        assert brute_force.main(argv) == (1, PW)                                # answered from the checkpoint


def test_server_and_gpu_client(dprf):
    """The work-distribution pair on an Agile stream: the server's payloads, verified by the GPU client in list mode."""
    import socket
    import threading
    from dprf_amd import client as cl, server as sv
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    hb = s.getsockname()[1]
    s.close()
    stream = _stream("ok", "2013", 256, 3)
    srv = sv.Server(stream, password_range=2, payload_size=300, heartbeat_port=hb, quiet=True)
    out = {}
    th = threading.Thread(target=lambda: out.setdefault("pw", srv.run("127.0.0.1", 0)), daemon=True)
    th.start()
    assert srv.bound.wait(10)
    ver = cl.GpuVerifier([0])
    rc, pw = cl.connect_to_server("127.0.0.1", srv.address[1], "gpu", ver, quiet=True)
    ver.close()
    th.join(10)
    assert (rc, pw) == (0, "ok") and out["pw"] == "ok"
