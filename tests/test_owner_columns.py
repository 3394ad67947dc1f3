"""Owner-mode R6 period columns (dprf_amd/csrc/dprf_kernels_r6.hip r6_pat_words_owner): the period is
pw || K[0:bs] || U[0:48], 48 bytes longer than the user search's.  For every range length and every list maximum the
column holds every word a block read touches, every byte a block uses is a period byte or a wrap byte r6_store_k
writes, the first message's read-back in r6_begin (pw || O[32:40] || U[0:48] || 0x80) stays inside the column, and
the workgroup still holds at least one group of 64 slots beside the tables.  Restated from the source, which is
checked to still contain the statement."""
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "dprf_amd", "csrc", "dprf_kernels_r6.hip")


def pat_words_owner(mode, lmax):
    if mode != 0:
        return ((lmax + 48 + 63) >> 2) + 5
    mx = ((lmax + 16) >> 2) + 5
    for bs in (32, 48, 64):
        Lp = lmax + bs + 48
        g = 16
        while Lp % g:
            g >>= 1
        for o in range(0, Lp, g):
            mx = max(mx, (o >> 2) + (5 if o & 3 else 4))
    return mx


def test_source_still_matches_restatement():
    src = open(SRC).read()
    body = src[src.index("static uint32_t r6_pat_words_owner"):]
    body = body[:body.index("\n}\n")]
    for frag in ("((lmax + 48u + 63u) >> 2) + 5u", "((lmax + 16u) >> 2) + 5u", "bs <= 64; bs += 16",
                 "const uint32_t Lp = lmax + bs + 48u;", "while (Lp % g) g >>= 1",
                 "(o >> 2) + ((o & 3u) ? 5u : 4u)"):
        assert frag in body, frag
    assert "const uint32_t Lp = len + bs + (OWNER ? 48u : 0u);" in src
    assert "if (at < colbytes) *L8(S.pat + pat_addr(at, S.lanebase))" in src


def _check(words, lmax, full_wrap):
    assert words >= 16                                      # r6_begin writes the 16 password words
    assert ((lmax + 16) >> 2) + 5 <= words                   # r6_load_k's second 5-word read
    assert ((lmax + 56) >> 2) + 1 <= words                   # r6_begin reads the first message back up to its 0x80
    for bs in (32, 48, 64):
        Lp = lmax + bs + 48
        assert Lp <= 4 * words                               # K and U[0:48] are stored whole
        written = set(range(Lp)) | {Lp + k for k in range(16) if Lp + k < 4 * words}
        if full_wrap:
            assert Lp + 16 <= 4 * words
        o = 0
        for _ in range(4 * Lp):
            nwords = 5 if (o & 3 or full_wrap) else 4         # list mode always reads five words
            assert (o >> 2) + nwords <= words, (lmax, bs, o)
            assert all(b in written for b in range(o, o + 16)), (lmax, bs, o)
            o = (o + 16) % Lp


def test_every_read_fits_and_every_used_byte_is_written():
    for lmax in range(1, 33):
        _check(pat_words_owner(0, lmax), lmax, False)
    for lmax in range(1, 65):
        _check(pat_words_owner(1, lmax), lmax, True)


def test_a_workgroup_keeps_at_least_one_group():
    # 160 KiB less the 64 KiB of tables, the charset, the shared block (under 16 KiB) and the 64 reserved bytes
    free = 160 * 1024 - 64 * 1024 - 256 - 16 * 1024 - 64
    assert free // (pat_words_owner(1, 64) * 256) >= 1
    assert free // (pat_words_owner(0, 32) * 256) >= 1
