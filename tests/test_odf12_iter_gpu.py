"""ODF 1.2 at the manifest's PBKDF2 iteration count on the device (k_odf_aes_kdf + k_odt_check, kernel family
"odf_aes_sha256") against tests/odf12_docgen.py's model, which tests/test_odf12_iter_model.py pins on the CPU, and at
1024 iterations against the "$odt$" stream of the same document (k_odt_kdf, the yardstick).  The shapes are the
smallest at which this kernel can go wrong: the loop's edges and the SHA-256 block edges of the start key.

  (a) iteration edges 1, 2, 3, 1024, 1025: every index of a 600-candidate list of the password hits, and none does on
      a document made with one iteration less or more; one case at 100000
  (b) candidate lengths 1, 55, 56, 64 and, through the long list, 65 and 200, planted at the edges of the workgroups
  (c) the rejecting direction: a bit in each checksum word, the salt, the iv, the first and the last content block
  (d) 1024 iterations: range, mask, symbols, hybrid and rules report what the "$odt$" context reports
  (e) two and four lanes on one device; stop_on_first reports the lower of two plantings
  (f) end to end from a package at 2000 iterations; the server and a GPU client
  (g) refusals, after each of which the library still serves"""
import contextlib
import functools
import io
import os
import time
import zlib

import pytest

import odf12_docgen as G
from odf_legacy_model import index_of, word

pytestmark = pytest.mark.gpu

FAMILY = "odf_aes_sha256"
PW = "Ux7"
N = 600                      # more than two 256-lane workgroups, no multiple of 64
LOWER = "abcdefghijklmnopqrstuvwxyz"


@pytest.fixture(scope="module")
def dprf():
    from dprf_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device: GPU tests need the MI355X box"
    return _lib


@functools.lru_cache(maxsize=None)
def _stream(pw, iterations=3):
    """One stream per (password, iterations), made once and shared."""
    s = G.make_stream(pw, iterations, seed=zlib.crc32(repr((pw, iterations)).encode()))
    assert G.verifies(s, pw)
    return s


@functools.lru_cache(maxsize=None)
def _verifies(s, w):
    return G.verifies(s, w)


def _model_hits(s, words):
    return [k for k, w in enumerate(words) if _verifies(s, w)]


# ---------------------------------------------------------------- (a) iteration edges
@pytest.mark.parametrize("c", [1, 2, 3, 1024, 1025])
def test_iteration_edges(dprf, c):
    s = _stream(PW, c)
    with dprf.Context(G.fields_of(s), device=0) as ctx:
        assert ctx.kernel == FAMILY and ctx.flags == 0 and ctx.format == dprf.FMT_ODT
        hits, n, st = ctx.verify_list([PW] * N)
        assert hits == list(range(N)) and n == N and st["candidates"] == N
    # a document made with one iteration less or more, under a stream that says c: the count is honoured, no constant
    for made_with in (c - 1, c + 1):
        if made_with < 1:
            continue
        f = G.fields_of(_stream(PW, made_with))
        f[3] = str(c)
        assert not G.verifies(f, PW)
        with dprf.Context(f, device=0) as ctx:
            hits, n, st = ctx.verify_list([PW] * N)
            assert hits == [] and n == 0 and st["candidates"] == N, (c, made_with)


def test_100000_iterations(dprf):
    s = _stream(PW, 100000)
    t0 = time.monotonic()
    with dprf.Context(G.fields_of(s), device=0) as ctx:
        hits, n, st = ctx.verify_list([PW] * N)
        assert hits == list(range(N)) and n == N and st["candidates"] == N
        assert ctx.verify_list(["Ux8"] * 70 + [PW])[0] == [70]
    assert time.monotonic() - t0 < 60.0


# ---------------------------------------------------------------- (b) start-key block edges, the long list
def _planted(L):
    return "".join(chr(33 + (7 * k + 5 * L + k * k) % 90) for k in range(L))


AT = (0, 63, 64, 255, 256, 299)


@pytest.mark.parametrize("L", [1, 55, 56, 64, 65, 200])
def test_planted_lengths(dprf, L):
    pw = _planted(L)
    assert len(pw.encode()) == L
    s = _stream(pw)
    # wrong candidates of the password's own length (so a long password's neighbours are on the long list too)
    decoy = (lambda k: pw[:-3] + "%03d" % k) if L >= 4 else (lambda k: "d%03dy" % k)
    near = [pw[:-1] if L > 1 else "~", pw + "x", pw, pw[:-1] + "}"]       # one byte less, one more, another last byte
    assert _model_hits(s, near) == [2] and not _verifies(s, decoy(7))
    with dprf.Context(G.fields_of(s), device=0) as ctx:
        for at in AT:
            words = [pw if k == at else decoy(k) for k in range(AT[-1] + 1)]
            assert words.count(pw) == 1
            hits, n, st = ctx.verify_list(words)
            assert hits == [at] and n == 1 and st["candidates"] == len(words), (L, at, hits)
        assert ctx.verify_list(near)[0] == [2]


def test_high_bytes_and_the_empty_candidate(dprf):
    words = ["pässwörd", "passwort", "日本語", b"\xff\xfe\x80", ""]
    for k in (0, 2, 3, 4):
        s = _stream(words[k])
        assert _model_hits(s, words) == [k]
        with dprf.Context(G.fields_of(s), device=0) as ctx:
            assert ctx.verify_list(words)[0] == [k]


# ---------------------------------------------------------------- (c) the rejecting direction
def _flip(hexfield, pos, bit):
    raw = bytearray(bytes.fromhex(hexfield))
    raw[pos] ^= 1 << bit
    return bytes(raw).hex()


def test_tampered_streams(dprf):
    base = G.fields_of(_stream(PW, 3))
    CK, IV, SALT, CONTENT = 5, 7, 9, 11
    cases = [(CK, 4 * w + w % 4, (3 * w + 1) % 8) for w in range(8)]          # one bit in each checksum word, in turn
    cases += [(SALT, 9, 4), (IV, 6, 2)]
    cases += [(CONTENT, 5, 1), (CONTENT, 16 * 63 + 11, 6)]                    # AES blocks 0 and 63
    for k, pos, bit in cases:
        f = list(base)
        f[k] = _flip(base[k], pos, bit)
        assert not G.verifies(f, PW), (k, pos, bit)
        with dprf.Context(f, device=0) as ctx:
            hits, nh, st = ctx.verify_list([PW, "Ux8"])
            assert hits == [] and nh == 0 and st["candidates"] == 2, (k, pos, bit)
    with dprf.Context(base, device=0) as ctx:
        assert ctx.verify_list([PW, "Ux8"])[0] == [0]


# ---------------------------------------------------------------- (d) 1024 iterations: the "$odt$" context's answers
PW4 = "nord"


@pytest.fixture(scope="module")
def pair(dprf, tmp_path_factory):
    """(the "$odf$*1*1*1024" context, the "$odt$" context) of one generated package's content.xml"""
    from dprf_amd.brute_force import parse_verification_data
    path = os.path.join(str(tmp_path_factory.mktemp("odf12")), "d.odt")
    e = G.write_odt12(path, PW4, seed=0x1024, iterations=1024)["content.xml"]
    odf = G.fields_of(G.odf_stream(e, 1024))
    with contextlib.redirect_stdout(io.StringIO()):
        odt = parse_verification_data(G.odt_stream(e))
    assert G.verifies(odf, PW4) and odt[0] == "odt"
    with dprf.Context(odf, device=0) as a, dprf.Context(odt, device=0) as b:
        assert (a.kernel, b.kernel) == (FAMILY, "odf_aes256")
        yield a, b


def _both(pair, call):
    got = [call(ctx) for ctx in pair]
    assert got[0][0] == got[1][0] and got[0][1] == got[1][1] == 1 and len(got[0][0]) == 1, got
    assert got[0][2]["candidates"] == got[1][2]["candidates"]
    return got[0][0][0]


def test_range_window_equals_the_odt_stream(pair):
    idx = index_of(PW4, LOWER)
    start, count = idx - 4001, 1 << 13
    assert start > 0 and start + count < 26 ** 4
    assert _both(pair, lambda c: c.search_range(LOWER, 4, start, count)) == idx
    assert _both(pair, lambda c: c.search_range(LOWER, 4, start, count, stop_on_first=True, cap=1)) == idx
    for ctx in pair:                                                            # one candidate short: the window misses
        assert ctx.search_range(LOWER, 4, start, idx - start)[0] == []


def test_mask_and_symbol_windows_equal_the_odt_stream(pair):
    from dprf_amd import mask as masks
    positions = masks.parse_mask("?l?l?l?l")
    idx = masks.index_of(positions, PW4)
    assert masks.word(positions, idx) == PW4
    assert _both(pair, lambda c: c.search_mask(positions, idx - 4001, 1 << 13)) == idx
    charset = "é" + LOWER                                                       # a two-byte character among the symbols
    sidx = index_of(PW4, charset)
    assert word(sidx, charset, 4) == PW4 and any("é" in word(k, charset, 4) for k in range(sidx - 4001, sidx + 4191))
    assert _both(pair, lambda c: c.search_symbols(charset, 4, sidx - 4001, 1 << 13)) == sidx


def test_hybrid_and_rules_equal_the_odt_stream(pair):
    from dprf_amd import hybrid, rules as rulemod
    words = [b"winter", "été".encode("utf-8"), b"no", b"x" * 62]
    positions, word_at = hybrid.parse_hybrid("?w?l?l")
    space = hybrid.space(len(words), positions)
    assert space == 4 * 676
    idx = hybrid.index_of(words, positions, word_at, PW4.encode())
    for ctx in pair:
        ctx.set_words(words)
    assert _both(pair, lambda c: c.search_hybrid(positions, word_at, 0, space)) == idx
    words = [b"winter", b"nor", "été".encode("utf-8"), b"summer"]
    rules = [rulemod.parse_rule(":"), rulemod.parse_rule("$d"), rulemod.parse_rule("u"), rulemod.parse_rule("c $1")]
    rspace = rulemod.space(len(words), len(rules))
    ridx = rulemod.index_of(words, rules, PW4.encode())
    cands = [rulemod.candidate(words, rules, k) for k in range(rspace)]
    assert cands.count(PW4.encode()) == 1 and cands[ridx] == PW4.encode()
    for ctx in pair:
        ctx.set_words(words)
    assert _both(pair, lambda c: c.search_rules(rules, 0, rspace)) == ridx
    a, b = pair
    assert a.spell_rules(rules, 0, rspace) == b.spell_rules(rules, 0, rspace) == cands    # raw bytes, rule unit = byte


# ---------------------------------------------------------------- (e) lanes on one device
DENSE = (0, 63, 64, 127, 128, 255, 256, 299)


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]])
def test_lanes_on_one_device(dprf, devices):
    s = _stream(PW, 3)
    words = [PW if k in DENSE else "d%03dy" % k for k in range(300)]
    two = [PW if k in (70, 200) else "d%03dy" % k for k in range(300)]
    assert not _verifies(s, "d001y")
    with dprf.Context(G.fields_of(s), devices=devices) as ctx:
        hits, n, st = ctx.verify_list(words)
        assert hits == list(DENSE) and n == len(DENSE) and st["candidates"] == 300
        assert ctx.verify_list(two, stop_on_first=True, cap=1)[0] == [70]      # the lower of two plantings
        assert ctx.verify_list(two)[0] == [70, 200]
        assert [d["device"] for d in ctx.last_call_devices()] == devices
        idx = index_of(PW, "678Ux")
        rhits, _, rst = ctx.search_range("678Ux", 3, 0, 125)
        assert rhits == [idx] and rst["candidates"] == 125


# ---------------------------------------------------------------- (f) end to end
def test_document_end_to_end(dprf, tmp_path):
    from dprf_amd import brute_force
    t = str(tmp_path)
    path = os.path.join(t, "new.odt")
    G.write_odt12(path, PW, seed=0x2000, iterations=2000)
    with contextlib.redirect_stdout(io.StringIO()):
        assert brute_force.main(["2", path, "--mask", "U?l?d", "--devices", "0"]) == (1, PW)
        stream = brute_force.get_verification_data("2", path)
        fields = brute_force.parse_verification_data(stream)
        assert fields[:5] == ["odf", "1", "1", "2000", "32"] and G.verifies(fields, PW)
        assert brute_force.init_listbased_brute_force(fields, ["Ux6", "ux7", PW, "Ux8"], devices=[0]) == (1, PW)
        assert brute_force.init_listbased_brute_force(fields, ["Ux6", "ux7"], devices=[0])[0] == 0
        wl = os.path.join(t, "words.txt")
        with open(wl, "w") as f:
            f.write("winter\nUx\nsummer\n")
        assert brute_force.main(["2", path, "--wordlist", wl, "--mask", "?w?d", "--devices", "0"]) == (1, PW)
        rl = os.path.join(t, "r.rule")
        with open(rl, "w") as f:
            f.write(":\nc $7\n")
        with open(wl, "w") as f:
            f.write("winter\nux\n")
        assert brute_force.main(["2", path, "--wordlist", wl, "--rules", rl, "--devices", "0"]) == (1, PW)


def test_server_and_gpu_client(dprf):
    """The work-distribution pair on a "$odf$*1*1*" stream: the server's payloads, verified by the GPU client."""
    import socket
    import threading
    from dprf_amd import client as cl, server as sv
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    hb = s.getsockname()[1]
    s.close()
    srv = sv.Server("new.odt:" + _stream("ok", 5), password_range=2, payload_size=300, heartbeat_port=hb, quiet=True)
    out = {}
    th = threading.Thread(target=lambda: out.setdefault("pw", srv.run("127.0.0.1", 0)), daemon=True)
    th.start()
    assert srv.bound.wait(10)
    ver = cl.GpuVerifier([0])
    rc, pw = cl.connect_to_server("127.0.0.1", srv.address[1], "gpu", ver, quiet=True)
    ver.close()
    th.join(10)
    assert (rc, pw) == (0, "ok") and out["pw"] == "ok"


# ---------------------------------------------------------------- (g) refusals
def test_stream_refusals(dprf):
    from test_odf12_iter_model import bad_streams
    good = _stream(PW, 3)
    base = G.fields_of(good)
    for name, k, v in bad_streams(base):
        f = list(base)
        f[k] = v
        with pytest.raises(dprf.DprfError) as ei:
            dprf.Context(f, device=0)
        assert ei.value.code == dprf.E_DOMAIN, (name, v[:12])
        assert name in str(ei.value) and "$odt$" in str(ei.value), (name, str(ei.value))
    for f in (base[:11], base + ["00"]):                                       # a wrong field count is no odf stream
        with pytest.raises(dprf.DprfError) as ei:
            dprf.Context(f, device=0)
        assert ei.value.code == dprf.E_INVALID
    with dprf.Context(base, device=0) as ctx:
        assert ctx.verify_list([PW, "Ux8"])[0] == [0]
        with pytest.raises(dprf.DprfError) as ei:
            ctx.set_pdf_password("owner")                                       # not a PDF context
        assert ei.value.code == dprf.E_INVALID
        assert ctx.verify_list([PW, "y" * 65])[0] == [0]                        # a long candidate is served, not refused
