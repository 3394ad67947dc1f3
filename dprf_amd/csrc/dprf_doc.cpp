/* dprf_doc.cpp -- the device-free half of libdprf.so (dprf_doc.h): the error text, the document parsers, the family
 * table, chunk planning, and the checks of candidates, words, masks and rules.  Nothing here includes or calls the
 * device runtime. */
#include "dprf_doc.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

/* ------------------------------------------------------------------ errors */
static thread_local std::string g_err;
extern "C" const char *dprf_last_error(void) { return g_err.c_str(); }

namespace dprf_internal __attribute__((visibility("hidden"))) {

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

/* ------------------------------------------------------------------ AES tables (FIPS 197 5.1.1) */
static uint8_t gmul(uint8_t a, uint8_t b) {
    uint8_t p = 0;
    while (b) {
        if (b & 1) p ^= a;
        a = (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0));
        b >>= 1;
    }
    return p;
}
static dprf_aes_tables make_tables() {
    dprf_aes_tables t;
    for (int x = 0; x < 256; x++) {
        uint8_t inv = 0;
        if (x)
            for (int y = 1; y < 256; y++)
                if (gmul((uint8_t)x, (uint8_t)y) == 1) { inv = (uint8_t)y; break; }
        uint8_t s = inv, r = inv;
        for (int i = 0; i < 4; i++) { r = (uint8_t)((r << 1) | (r >> 7)); s ^= r; }
        s ^= 0x63;
        t.sbox[x] = s;
        t.inv_sbox[s] = (uint8_t)x;
    }
    for (int x = 0; x < 256; x++) {
        uint8_t s = t.sbox[x], i = t.inv_sbox[x];
        t.te0[x] = ((uint32_t)gmul(s, 2) << 24) | ((uint32_t)s << 16) | ((uint32_t)s << 8) | gmul(s, 3);
        t.td0[x] = ((uint32_t)gmul(i, 14) << 24) | ((uint32_t)gmul(i, 9) << 16) | ((uint32_t)gmul(i, 13) << 8) |
                   gmul(i, 11);
    }
    return t;
}
const dprf_aes_tables &aes_tables() {
    static const dprf_aes_tables t = make_tables();
    return t;
}

/* ------------------------------------------------------------------ host MD5 (RFC 1321), for the
 * document constant MD5(PAD || ID) only */
static void md5_host(const uint8_t *msg, size_t n, uint8_t out[16]) {
    static const uint32_t K[64] = {
        0xd76aa478u,0xe8c7b756u,0x242070dbu,0xc1bdceeeu,0xf57c0fafu,0x4787c62au,0xa8304613u,0xfd469501u,
        0x698098d8u,0x8b44f7afu,0xffff5bb1u,0x895cd7beu,0x6b901122u,0xfd987193u,0xa679438eu,0x49b40821u,
        0xf61e2562u,0xc040b340u,0x265e5a51u,0xe9b6c7aau,0xd62f105du,0x02441453u,0xd8a1e681u,0xe7d3fbc8u,
        0x21e1cde6u,0xc33707d6u,0xf4d50d87u,0x455a14edu,0xa9e3e905u,0xfcefa3f8u,0x676f02d9u,0x8d2a4c8au,
        0xfffa3942u,0x8771f681u,0x6d9d6122u,0xfde5380cu,0xa4beea44u,0x4bdecfa9u,0xf6bb4b60u,0xbebfbc70u,
        0x289b7ec6u,0xeaa127fau,0xd4ef3085u,0x04881d05u,0xd9d4d039u,0xe6db99e5u,0x1fa27cf8u,0xc4ac5665u,
        0xf4292244u,0x432aff97u,0xab9423a7u,0xfc93a039u,0x655b59c3u,0x8f0ccc92u,0xffeff47du,0x85845dd1u,
        0x6fa87e4fu,0xfe2ce6e0u,0xa3014314u,0x4e0811a1u,0xf7537e82u,0xbd3af235u,0x2ad7d2bbu,0xeb86d391u};
    static const int S[16] = {7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21};
    std::vector<uint8_t> m(msg, msg + n);
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    uint64_t bits = (uint64_t)n * 8;
    for (int i = 0; i < 8; i++) m.push_back((uint8_t)(bits >> (8 * i)));
    uint32_t h[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    for (size_t off = 0; off < m.size(); off += 64) {
        uint32_t w[16];
        for (int i = 0; i < 16; i++)
            w[i] = (uint32_t)m[off + 4 * i] | ((uint32_t)m[off + 4 * i + 1] << 8) |
                   ((uint32_t)m[off + 4 * i + 2] << 16) | ((uint32_t)m[off + 4 * i + 3] << 24);
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
        for (int i = 0; i < 64; i++) {
            uint32_t f;
            int g;
            if (i < 16) { f = (b & c) | (~b & d); g = i; }
            else if (i < 32) { f = (d & b) | (~d & c); g = (5 * i + 1) & 15; }
            else if (i < 48) { f = b ^ c ^ d; g = (3 * i + 5) & 15; }
            else { f = c ^ (b | ~d); g = (7 * i) & 15; }
            uint32_t tmp = d;
            d = c;
            c = b;
            uint32_t x = a + f + K[i] + w[g];
            int s = S[(i >> 4) * 4 + (i & 3)];
            b = b + ((x << s) | (x >> (32 - s)));
            a = tmp;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d;
    }
    for (int i = 0; i < 4; i++)
        for (int k = 0; k < 4; k++) out[4 * i + k] = (uint8_t)(h[i] >> (8 * k));
}

/* ------------------------------------------------------------------ field decoding */
static int hexval(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}
/* the 2 * n hex digits at s (the caller has checked the length) as n bytes; false at the first non-digit */
static bool hex_bytes(const char *s, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; i++) {
        const int hi = hexval((unsigned char)s[2 * i]), lo = hexval((unsigned char)s[2 * i + 1]);
        if (hi < 0 || lo < 0) return false;
        out[i] = (uint8_t)(hi << 4 | lo);
    }
    return true;
}
/* The reference decodes with str_to_uchar (BN_hex2bn + BN_bn2bin, msoffcrypto...c:340-349) into a
 * buffer of the length its argv declares.  Inside the parity domain the string is exactly 2*declared
 * hex digits; a leading 00 byte makes the reference decode short (flagged, decoded in full here). */
static int decode_hex(const char *s, int declared, std::vector<uint8_t> &out, int &flags, const char *what) {
    size_t n = strlen(s);
    if (declared < 0 || n != (size_t)declared * 2)
        return fail(DPRF_E_DOMAIN, "%s: %zu hex digits for a declared length of %d bytes", what, n, declared);
    out.resize((size_t)declared);
    if (!hex_bytes(s, out.size(), out.data())) return fail(DPRF_E_DOMAIN, "%s: not a hex string", what);
    if (declared > 0 && out[0] == 0) flags |= DPRF_FLAG_REF_NONDETERMINISTIC;
    return DPRF_OK;
}
/* The streams no reference verifier reads (Agile, Office 97-2003, ODF 1.0 / 1.1): a field of exactly nbytes, decoded
 * in full, nothing flagged. */
static int decode_hex_exact(const char *s, size_t nbytes, uint8_t *out, const char *what,
                            const char *who = "office agile") {
    const size_t n = strlen(s);
    if (n != 2 * nbytes)
        return fail(DPRF_E_DOMAIN, "%s: %s has %zu hex digits (%zu expected)", who, what, n, 2 * nbytes);
    if (!hex_bytes(s, nbytes, out)) return fail(DPRF_E_DOMAIN, "%s: %s is not a hex string", who, what);
    return DPRF_OK;
}
/* a decimal field: 1..max_digits digits and nothing else, with a value in lo..hi */
static bool read_decimal(const char *s, size_t max_digits, uint64_t lo, uint64_t hi, uint64_t &v) {
    const size_t nd = strlen(s);
    if (nd < 1 || nd > max_digits) return false;
    v = 0;
    for (size_t i = 0; i < nd; i++) {
        if (s[i] < '0' || s[i] > '9') return false;
        v = v * 10 + (uint64_t)(s[i] - '0');
    }
    return v >= lo && v <= hi;
}
static uint32_t be_word(const uint8_t *p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}
static uint32_t le_word(const uint8_t *p) {
    return ((uint32_t)p[3] << 24) | ((uint32_t)p[2] << 16) | ((uint32_t)p[1] << 8) | p[0];
}
static const uint8_t PDF_PAD[32] = {0x28, 0xBF, 0x4E, 0x5E, 0x4E, 0x75, 0x8A, 0x41, 0x64, 0x00, 0x4E,
                                    0x56, 0xFF, 0xFA, 0x01, 0x08, 0x2E, 0x2E, 0x00, 0xB6, 0xD0, 0x68,
                                    0x3E, 0x80, 0x2F, 0x0C, 0xA9, 0xFE, 0x64, 0x53, 0x69, 0x7A};

/* ------------------------------------------------------------------ the family table */
#ifndef DPRF_R24_HI_LOG2
#define DPRF_R24_HI_LOG2 30
#endif
#ifndef DPRF_R24_TARGET_MS
#define DPRF_R24_TARGET_MS 100.0
#endif
/* R6: every launch of the persistent kernel ends in a drain (the last candidates' ~35 remaining rounds with
 * fewer live slots than lanes, ~70 ms), so its launches are long: same 2^23-candidate steps measured 2.79 / 2.92 /
 * 3.00 M cand/s with 2^21 / 2^22 / 2^23 per launch (tools/ab_r6_chunk.sh, round 2).  Round 4: the start and the drain of
 * a launch are also what leaves class batches part-filled (61.7 of 64 lanes on 2^22-candidate launches, a per-wave timing build, HISTORY.md;
 * a flow simulation of the claim gives 62.2 / 63.0 / 63.5 / 63.8 at 2^22 / 2^23 / 2^24 / 2^25 per launch and 64.0 in
 * the steady state); 2^23 / 2^24 / 2^25 per launch measured 3.685 / 3.725 / 3.746 M cand/s (tools/sessions/session_d.sh, three
 * alternating runs each), so launches now take ~9 s (2^25 at the measured rate) */
#ifndef DPRF_R6_LO_LOG2
#define DPRF_R6_LO_LOG2 21
#endif
#ifndef DPRF_R6_HI_LOG2
#define DPRF_R6_HI_LOG2 25
#endif
#ifndef DPRF_R6_TARGET_MS
#define DPRF_R6_TARGET_MS 12000.0
#endif
#ifndef DPRF_ODT_INIT_LOG2
#define DPRF_ODT_INIT_LOG2 22
#endif
#ifndef DPRF_ODT_HI_LOG2
#define DPRF_ODT_HI_LOG2 23
#endif
#ifndef DPRF_ODT_TARGET_MS
#define DPRF_ODT_TARGET_MS 300.0
#endif
#ifndef DPRF_OFFICE_HI_LOG2
#define DPRF_OFFICE_HI_LOG2 20
#endif
#ifndef DPRF_OFFICE_TARGET_MS
#define DPRF_OFFICE_TARGET_MS 400.0
#endif
/* the chunk policies more than one family takes (chunk_policy in dprf_doc.h: init, lo, hi, target_ms, tail, gran) */
#define POLICY_OFFICE {1u << 19, 1u << 19, 1u << DPRF_OFFICE_HI_LOG2, DPRF_OFFICE_TARGET_MS, 1u << 18, 256}
#define POLICY_R24 {1u << 24, 1u << 20, 1u << DPRF_R24_HI_LOG2, DPRF_R24_TARGET_MS, 1u << 20, 4096}
#define POLICY_ODT {1u << DPRF_ODT_INIT_LOG2, 1u << 19, 1u << DPRF_ODT_HI_LOG2, DPRF_ODT_TARGET_MS, 1u << 19, 512}
static const uint32_t NO_CUT = ~0u;
#define NO_LONG_AGILE "longer than 32 UTF-16 units: long Office Agile candidates are not supported yet"
#define NO_LONG_OLDOFFICE "longer than 32 UTF-16 units: long Office 97-2003 candidates are not supported yet"
/* One row per kernel_kind, in the enum's order (the static_assert below holds the build to it).  Columns: the kind,
 * its name, owner-mode name, key-search name and known-key (collider) name, chunk policy, the verifier's cut, key
 * words handed from the KDF to the check, long-list prehash and whether it writes keys, the refusal without a
 * long-list mode, streams per device. */
constexpr family FAMILIES[K_COUNT] = {
    /* a never-matching context launches nothing */
    {K_NONE, "none", nullptr, nullptr, nullptr, {1u << 24, 1u << 20, 1u << 24, 100.0, 1u << 20, 256}, NO_CUT, 0, 0, false, nullptr, 1},
    {K_OFFICE, "office_std", nullptr, nullptr, nullptr, POLICY_OFFICE, NO_CUT, 8, DPRF_LONG_SHA1_SALT16, true, nullptr, 1},
    {K_ODT, "odf_aes256", nullptr, nullptr, nullptr, POLICY_ODT, NO_CUT, 8, DPRF_LONG_SHA256, true, nullptr, 1},
    /* R2-R4 truncate at 32 bytes: never long */
    {K_PDF_R24, "pdf_r24", "pdf_r24_owner", "pdf_r24_key40", "pdf_r24_collide", POLICY_R24, 32, 0, 0, false, nullptr,
     DPRF_R24_STREAMS},
    /* R5: the prehash is the whole check */
    {K_PDF_R5, "pdf_r5", "pdf_r5_owner", nullptr, nullptr, {1u << 27, 1u << 22, 1u << 31, 100.0, 1u << 22, 2048}, 127, 0, DPRF_LONG_R5,
     false, nullptr, 1},
    {K_PDF_R6, "pdf_r6", "pdf_r6_owner", nullptr, nullptr,
     {1u << 22, 1u << DPRF_R6_LO_LOG2, 1u << DPRF_R6_HI_LOG2, DPRF_R6_TARGET_MS, 1u << 20, 64}, NO_CUT, 0,
     DPRF_LONG_SHA256_SALT8, true, nullptr, 1},
    /* Agile: Office's target and granularity; init / lo / tail are one resident generation of k_agile_kdf at the
     * occupancy it builds with (256 CUs x 4 SIMDs x waves x 64 lanes: 2^19 at 8 waves per SIMD for SHA-1, 2^18 at
     * 4 for SHA-512).  It hands over two keys of up to 8 words. */
    {K_AGILE_SHA1, "office_agile_sha1", nullptr, nullptr, nullptr, POLICY_OFFICE, NO_CUT, 16, 0, false, NO_LONG_AGILE, 1},
    {K_AGILE_SHA512, "office_agile_sha512", nullptr, nullptr, nullptr,
     {1u << 18, 1u << 18, 1u << DPRF_OFFICE_HI_LOG2, DPRF_OFFICE_TARGET_MS, 1u << 18, 256}, NO_CUT, 16, 0, false,
     NO_LONG_AGILE, 1},
    /* Office 97-2003 RC4 (types 0 / 1) and RC4 CryptoAPI (types 3 / 4): one kernel, fast hashes between R2 and R4 in
     * cost -- pdf_r24's row, on one stream */
    {K_OLDOFFICE_MD5, "office_rc4_md5", nullptr, "office_rc4_md5_key40", "office_rc4_md5_collide",
     POLICY_R24, NO_CUT, 0, 0, false, NO_LONG_OLDOFFICE, 1},
    {K_OLDOFFICE_SHA1, "office_rc4_sha1", nullptr, "office_rc4_sha1_key40", "office_rc4_sha1_collide",
     POLICY_R24, NO_CUT, 0, 0, false, NO_LONG_OLDOFFICE, 1},
    /* ODF 1.0 / 1.1: half of ODF 1.2's KDF and a check of about the same time again -- its row */
    {K_ODF_BF, "odf_bf_sha1", nullptr, nullptr, nullptr, POLICY_ODT, NO_CUT, 8, 0, false,
     "longer than 64 bytes: long ODF 1.0/1.1 candidates are not supported yet", DPRF_ODF_STREAMS},
    /* ODF 1.2 at the manifest's iteration count: ODF 1.2's row, which describes 1024 iterations; policy() scales it
     * by the document's count */
    {K_ODF_AES, "odf_aes_sha256", nullptr, nullptr, nullptr, POLICY_ODT, NO_CUT, 8, DPRF_LONG_SHA256, true, nullptr, 1},
};
constexpr bool rows_in_order(int k = 0) { return k == K_COUNT || (FAMILIES[k].kind == k && rows_in_order(k + 1)); }
static_assert(rows_in_order(), "FAMILIES needs one row per kernel_kind, in the enum's order");

const char *kind_name(kernel_kind k, bool owner, bool collide) {
    const family &f = fam(k);
    if (collide && f.collide_name) return f.collide_name;
    return owner && f.owner_name ? f.owner_name : f.name;
}
chunk_policy policy(kernel_kind k, bool owner, bool collide, uint32_t iterations) {
    chunk_policy p = fam(k).policy;
    if (k == K_ODF_AES && iterations && iterations != 1024u) {
        /* the row is sized for 1024 iterations; a candidate costs iterations / 1024 of that.  Never above hi (the key
         * buffer holds hi candidates), never below one resident generation of the KDF kernel */
        auto scale = [&](uint32_t v) {
            const uint64_t w = round_up(((uint64_t)v * 1024u + iterations - 1) / iterations, p.gran);
            return (uint32_t)std::min<uint64_t>(p.hi, std::max<uint64_t>(w, ODF_AES_GENERATION));
        };
        p.init = scale(p.init);
        p.lo = scale(p.lo);
        p.tail = scale(p.tail);
    }
    if (owner && fam(k).owner_name) p.init = std::max(p.init / 2, p.lo);
    /* a known key: hashing alone, 2 to 5 times the password family's rate (PDF R2 56 G cand/s, type 3
     * 30 G), so the password family's ceiling of 2^30 would hold a launch at 19 to 36 ms of its own 100 ms target.
     * 2^31 is the most a launch's 32-bit count and block offsets take (PDF R5's ceiling) */
    if (collide && fam(k).collide_name) p.hi = std::max(p.hi, 1u << 31);
    return p;
}
uint64_t round_up(uint64_t v, uint64_t g) { return (v + g - 1) / g * g; }
uint64_t plan_chunk(kernel_kind k, bool owner, double rate, uint64_t remaining, uint64_t total, int ndev, int inflight,
                    bool collide, uint32_t iterations) {
    const chunk_policy p = policy(k, owner, collide, iterations);
    uint64_t want = p.init;
    if (rate > 0) {
        const double t = rate * p.target_ms;
        want = p.lo;
        while (want < p.hi && 2.0 * (double)want <= t) want <<= 1;
        want = std::min<uint64_t>(want, p.hi);   /* a scaled floor is no power of two: the doubling may pass hi */
    }
    if (ndev > 1) {
        const uint64_t nd = (uint64_t)ndev;
        const uint64_t raw = (remaining + 4 * nd - 1) / (4 * nd);
        const uint64_t guided = round_up(raw, raw >= 8ull * p.gran ? p.gran : 64);   /* whole workgroups when large */
        /* a small call's fair share rounds to whole waves only, so every device gets one */
        const uint64_t floor_ = std::min<uint64_t>(p.tail, round_up((total + nd - 1) / nd, 64));
        want = std::min(want, std::max(guided, floor_));
        /* no taking ahead when work is scarce: a device that still has a launch in flight waits for it unless
         * every device could get a chunk this size (else the first device to act takes a small call twice) */
        if (inflight > 0 && remaining < nd * want) return 0;
    }
    return std::min(want, remaining);
}

/* ------------------------------------------------------------------ the parsers */
/* Office 2010 / 2013 Agile Encryption (include/dprf.h "Agile"): ["office", "2010" | "2013", spinCount, keyBits,
 * saltSize, salt, encryptedVerifierHashInput, encryptedVerifierHashValue[0:32]].  No reference verifier reads this
 * stream, so nothing here is flagged DPRF_FLAG_REF_NONDETERMINISTIC: the hex fields are decoded in full. */
static int parse_agile(dprf_doc *c, const char *const *f) {
    const bool sha512 = !strcmp(f[1], "2013");
    uint64_t spin = 0;
    if (!read_decimal(f[2], 9, 0, DPRF_AGILE_MAX_SPIN, spin))
        return fail(DPRF_E_DOMAIN, "office agile: spinCount '%s' (decimal, 0..%d)", f[2], DPRF_AGILE_MAX_SPIN);
    if (strcmp(f[3], "128") && strcmp(f[3], "256"))
        return fail(DPRF_E_DOMAIN, "office agile: keyBits '%s' (128 or 256; AES-192 is not supported)", f[3]);
    if (strcmp(f[4], "16")) return fail(DPRF_E_DOMAIN, "office agile: saltSize '%s' (16)", f[4]);
    uint8_t salt[16], evi[16], evh[32];
    int r;
    if ((r = decode_hex_exact(f[5], 16, salt, "salt"))) return r;
    if ((r = decode_hex_exact(f[6], 16, evi, "encryptedVerifierHashInput"))) return r;
    if ((r = decode_hex_exact(f[7], 32, evh, "encryptedVerifierHashValue"))) return r;
    dprf_agile_params &p = c->agile;
    for (int i = 0; i < 4; i++) p.salt[i] = be_word(&salt[4 * i]);
    for (int i = 0; i < 4; i++) p.evi[i] = be_word(&evi[4 * i]);
    for (int i = 0; i < 8; i++) p.evh[i] = be_word(&evh[4 * i]);
    p.spin = (uint32_t)spin;
    p.sha512 = sha512 ? 1u : 0u;
    p.key_words = !strcmp(f[3], "256") ? 8u : 4u;
    c->kind = sha512 ? K_AGILE_SHA512 : K_AGILE_SHA1;
    return DPRF_OK;
}

/* Office 97-2003 RC4 / RC4 CryptoAPI (include/dprf.h "Office 97-2003"): ["oldoffice", type, salt, encryptedVerifier,
 * encryptedVerifierHash].  No reference verifier reads this stream: the hex fields are decoded in full and nothing is
 * flagged. */
static int parse_oldoffice(dprf_doc *c, const char *const *f) {
    static const char *who = "oldoffice";
    const bool one = f[1][0] != 0 && f[1][1] == 0;
    if (!one || (f[1][0] != '0' && f[1][0] != '1' && f[1][0] != '3' && f[1][0] != '4'))
        return fail(DPRF_E_DOMAIN, "oldoffice: type '%s' (0 or 1: RC4; 3 or 4: RC4 CryptoAPI)", f[1]);
    const int type = f[1][0] - '0';
    const bool sha1 = type >= 3;
    uint8_t salt[16], ev[16], evh[20] = {0};
    int r;
    if ((r = decode_hex_exact(f[2], 16, salt, "salt", who))) return r;
    if ((r = decode_hex_exact(f[3], 16, ev, "encryptedVerifier", who))) return r;
    if ((r = decode_hex_exact(f[4], sha1 ? 20 : 16, evh, "encryptedVerifierHash", who))) return r;
    dprf_oldoffice_params &p = c->oldoffice;
    p.sha1 = sha1 ? 1u : 0u;
    p.key_bytes = type == 3 ? 5u : 16u;
    for (int i = 0; i < 4; i++) p.salt[i] = be_word(&salt[4 * i]);
    for (int i = 0; i < 4; i++) p.ev[i] = le_word(&ev[4 * i]);
    for (int i = 0; i < 5; i++) p.evh[i] = le_word(&evh[4 * i]);
    /* types 0 / 1: the padded message (h[0:5] || salt) x 16 -- 336 bytes, six MD5 blocks -- with zeros where the kernel
     * places the five hash bytes of each 21-byte copy */
    uint8_t msg[4 * DPRF_OLDOFFICE_REP_WORDS] = {0};
    for (int k = 0; k < 16; k++) memcpy(msg + 21 * k + 5, salt, 16);
    msg[336] = 0x80;
    const uint64_t bits = 336 * 8;
    for (int i = 0; i < 8; i++) msg[sizeof msg - 8 + i] = (uint8_t)(bits >> (8 * i));
    for (int i = 0; i < DPRF_OLDOFFICE_REP_WORDS; i++) p.rep[i] = le_word(msg + 4 * i);
    c->kind = sha1 ? K_OLDOFFICE_SHA1 : K_OLDOFFICE_MD5;
    return DPRF_OK;
}

static int parse_office(dprf_doc *c, const char *const *f) {
    /* the version field selects Agile Encryption; every other stream is Office 2007 Standard Encryption as before */
    if (!strcmp(f[1], "2010") || !strcmp(f[1], "2013")) return parse_agile(c, f);
    /* argv mapping brute_force.py:163-173 */
    int salt_len = atoi(f[4]);
    int ev_len = (int)(strlen(f[6]) / 2), evh_len = (int)(strlen(f[7]) / 2);
    int key_bits = atoi(f[3]), hash_size = atoi(f[2]);
    if (salt_len != 16) return fail(DPRF_E_DOMAIN, "office: salt_len %d (office2john asserts 16)", salt_len);
    if (ev_len % 16 || evh_len % 16 || ev_len > 128 || evh_len > 128)
        return fail(DPRF_E_DOMAIN, "office: verifier lengths %d/%d abort the reference's EVP decrypt", ev_len, evh_len);
    if (key_bits < 128) return fail(DPRF_E_DOMAIN, "office: key_bits %d < 128", key_bits);
    std::vector<uint8_t> salt, ev, evh;
    int r;
    if ((r = decode_hex(f[5], salt_len, salt, c->flags, "office salt"))) return r;
    if ((r = decode_hex(f[6], ev_len, ev, c->flags, "office encrypted verifier"))) return r;
    if ((r = decode_hex(f[7], evh_len, evh, c->flags, "office encrypted verifier hash"))) return r;
    if (ev_len != 16 || evh_len != 32) {
        c->flags |= DPRF_FLAG_NEVER_MATCHES;   /* msoffcrypto...c:163,168 */
        return DPRF_OK;
    }
    if (hash_size < 0 || hash_size >= 32)
        return fail(DPRF_E_DOMAIN, "office: verifier_hash_size %d reads past the decrypted hash", hash_size);
    for (int i = 0; i < 4; i++) c->office.salt[i] = be_word(&salt[4 * i]);
    for (int i = 0; i < 4; i++) c->office.ev[i] = be_word(&ev[4 * i]);
    for (int i = 0; i < 8; i++) c->office.evh[i] = be_word(&evh[4 * i]);
    c->office.hash_size = (uint32_t)hash_size;
    c->kind = K_OFFICE;
    return DPRF_OK;
}

static int parse_odt(dprf_doc *c, const char *const *f) {
    /* argv mapping brute_force.py:175-182 */
    int enc_len = atoi(f[6]);
    if (enc_len < 0 || enc_len % 16)
        return fail(DPRF_E_DOMAIN, "odt: encrypted length %d is not a multiple of 16 (reference aborts)", enc_len);
    std::vector<uint8_t> ck, iv, salt, enc;
    int r;
    if ((r = decode_hex(f[2], 32, ck, c->flags, "odt checksum"))) return r;
    if ((r = decode_hex(f[3], 16, iv, c->flags, "odt iv"))) return r;
    if ((r = decode_hex(f[4], 16, salt, c->flags, "odt salt"))) return r;
    if ((r = decode_hex(f[5], enc_len, enc, c->flags, "odt encrypted file"))) return r;
    for (int i = 0; i < 8; i++) c->odt.checksum[i] = be_word(&ck[4 * i]);
    for (int i = 0; i < 4; i++) c->odt.iv[i] = be_word(&iv[4 * i]);
    for (int i = 0; i < 4; i++) c->odt.salt[i] = be_word(&salt[4 * i]);
    c->odt.enc_len = (uint32_t)enc_len;
    c->odt.hash_len = (uint32_t)std::min(enc_len, 1024);
    const uint32_t nw = std::max<uint32_t>(4u, c->odt.hash_len / 4);
    c->odt_words.assign(nw, 0u);
    for (uint32_t i = 0; i < c->odt.hash_len / 4; i++) c->odt_words[i] = be_word(&enc[4 * i]);
    c->kind = K_ODT;
    return DPRF_OK;
}

/* ODF 1.0 / 1.1, Blowfish-CFB with SHA-1 (include/dprf.h "ODF 1.0/1.1"): ["odf", cipher "0", checksum type "0",
 * iterations, key size "16", checksum, iv length "8", iv, salt length "16", salt, inplace "0", content].  No reference
 * verifier reads this stream: the hex fields are decoded in full and nothing is flagged. */
/* ODF 1.2 at the manifest's iteration count (include/dprf.h "$odf$*1*1*"): ["odf", cipher "1", checksum type "1",
 * iterations, key size "32", checksum, iv length "16", iv, salt length "16", salt, inplace "0", content].  The
 * reference's own spelling of such a document is the $odt$ stream, which has no field for the count: every refusal
 * here says so.  Decoded in full, nothing flagged. */
#define ODF_AES_HINT "; at 1024 iterations the reference's spelling of an ODF 1.2 document is the $odt$ stream (odt2hashes)"
static int parse_odf_aes(dprf_doc *c, const char *const *f) {
    static const char *who = "odf (AES-256-CBC, SHA-256)";
    if (strcmp(f[4], "32")) return fail(DPRF_E_DOMAIN, "%s: key size '%s' (32)" ODF_AES_HINT, who, f[4]);
    if (strcmp(f[6], "16")) return fail(DPRF_E_DOMAIN, "%s: iv length '%s' (16)" ODF_AES_HINT, who, f[6]);
    if (strcmp(f[8], "16")) return fail(DPRF_E_DOMAIN, "%s: salt length '%s' (16)" ODF_AES_HINT, who, f[8]);
    if (strcmp(f[10], "0")) return fail(DPRF_E_DOMAIN, "%s: inplace flag '%s' (0)" ODF_AES_HINT, who, f[10]);
    uint64_t iter = 0;
    if (!read_decimal(f[3], 9, 1, DPRF_ODF_MAX_ITER, iter))
        return fail(DPRF_E_DOMAIN, "%s: iterations '%s' (a decimal in 1..%d)" ODF_AES_HINT, who, f[3], DPRF_ODF_MAX_ITER);
    uint8_t ck[32], iv[16], salt[16];
    std::vector<uint8_t> content(4 * DPRF_ODF_CONTENT_WORDS);
    const struct { int at; size_t n; uint8_t *out; const char *what; } hex[4] = {
        {5, 32, ck, "checksum"}, {7, 16, iv, "iv"}, {9, 16, salt, "salt"}, {11, content.size(), content.data(), "content"}};
    for (const auto &h : hex)
        if (const int r = decode_hex_exact(f[h.at], h.n, h.out, h.what, who))
            return fail(r, "%s" ODF_AES_HINT, std::string(dprf_last_error()).c_str());
    for (int i = 0; i < 8; i++) c->odt.checksum[i] = be_word(&ck[4 * i]);
    for (int i = 0; i < 4; i++) c->odt.iv[i] = be_word(&iv[4 * i]);
    for (int i = 0; i < 4; i++) c->odt.salt[i] = c->odfaes.salt[i] = be_word(&salt[4 * i]);
    c->odt.enc_len = c->odt.hash_len = 4 * DPRF_ODF_CONTENT_WORDS;
    c->odfaes.iterations = (uint32_t)iter;
    c->odt_words.assign(DPRF_ODF_CONTENT_WORDS, 0u);
    for (int i = 0; i < DPRF_ODF_CONTENT_WORDS; i++) c->odt_words[i] = be_word(&content[4 * i]);
    c->kind = K_ODF_AES;
    return DPRF_OK;
}

static int parse_odf(dprf_doc *c, const char *const *f) {
    static const char *who = "odf";
    if (!strcmp(f[1], "1") && !strcmp(f[2], "1")) return parse_odf_aes(c, f);
    if (strcmp(f[1], "0")) return fail(DPRF_E_DOMAIN, "odf: cipher '%s' (0: Blowfish-CFB)", f[1]);
    if (strcmp(f[2], "0")) return fail(DPRF_E_DOMAIN, "odf: checksum type '%s' (0: SHA-1)", f[2]);
    if (strcmp(f[4], "16")) return fail(DPRF_E_DOMAIN, "odf: key size '%s' (16)", f[4]);
    if (strcmp(f[6], "8")) return fail(DPRF_E_DOMAIN, "odf: iv length '%s' (8)", f[6]);
    if (strcmp(f[8], "16")) return fail(DPRF_E_DOMAIN, "odf: salt length '%s' (16)", f[8]);
    if (strcmp(f[10], "0")) return fail(DPRF_E_DOMAIN, "odf: inplace flag '%s' (0)", f[10]);
    uint64_t iter = 0;
    if (!read_decimal(f[3], 9, 1, DPRF_ODF_MAX_ITER, iter))
        return fail(DPRF_E_DOMAIN, "odf: iterations '%s' (a decimal in 1..%d)", f[3], DPRF_ODF_MAX_ITER);
    uint8_t ck[20], iv[8], salt[16];
    std::vector<uint8_t> content(4 * DPRF_ODF_CONTENT_WORDS);
    int r;
    if ((r = decode_hex_exact(f[5], 20, ck, "checksum", who))) return r;
    if ((r = decode_hex_exact(f[7], 8, iv, "iv", who))) return r;
    if ((r = decode_hex_exact(f[9], 16, salt, "salt", who))) return r;
    if ((r = decode_hex_exact(f[11], content.size(), content.data(), "content", who))) return r;
    for (int i = 0; i < 5; i++) c->odf.checksum[i] = be_word(&ck[4 * i]);
    for (int i = 0; i < 4; i++) c->odf.salt[i] = be_word(&salt[4 * i]);
    c->odf.iterations = (uint32_t)iter;
    c->odf_words.assign(DPRF_ODF_X_WORDS, 0u);
    for (int i = 0; i < 2; i++) c->odf_words[i] = be_word(&iv[4 * i]);
    for (int i = 0; i < DPRF_ODF_CONTENT_WORDS; i++) c->odf_words[2 + i] = be_word(&content[4 * i]);
    c->kind = K_ODF_BF;
    return DPRF_OK;
}

static int parse_pdf(dprf_doc *c, const char *const *f) {
    /* argv mapping brute_force.py:184-197 */
    int V = atoi(f[1]), R = atoi(f[2]), Length = atoi(f[3]), P = atoi(f[4]), meta = atoi(f[5]);
    int id_len = atoi(f[6]), u_len = atoi(f[8]), o_len = atoi(f[10]);
    std::vector<uint8_t> id, u, o;
    int r;
    if ((r = decode_hex(f[7], id_len, id, c->flags, "pdf id"))) return r;
    if ((r = decode_hex(f[9], u_len, u, c->flags, "pdf U"))) return r;
    if ((r = decode_hex(f[11], o_len, o, c->flags, "pdf O"))) return r;
    c->pdf_o_len = (int)o.size();
    c->pdf_u_len = (int)u.size();
    /* (V,R) whitelist and Length % 8 (pdf...c:89-101) */
    if ((V != 1 && V != 2 && V != 4 && V != 5) || (V == 1 && R != 2) || (V == 2 && R != 3) ||
        (V == 4 && R != 4) || (V == 5 && (R != 5 && R != 6)) || Length % 8 != 0) {
        c->flags |= DPRF_FLAG_NEVER_MATCHES;
        return DPRF_OK;
    }
    dprf_pdf_params &p = c->pdf;
    p.R = (uint32_t)R;
    for (int i = 0; i < 8; i++) p.pad[i] = le_word(PDF_PAD + 4 * i);
    if (R >= 5) {
        if (u_len < 40) return fail(DPRF_E_DOMAIN, "pdf R%d: U shorter than 40 bytes", R);
        for (int i = 0; i < 8; i++) p.u[i] = be_word(&u[4 * i]);
        p.u[8] = le_word(&u[32]);
        p.u[9] = le_word(&u[36]);
        /* owner check: O[0:32] is the hash, O[32:40] || U[0:48] follow the candidate in its first message */
        if (o.size() >= 48 && u.size() >= 48) {
            for (int i = 0; i < 8; i++) p.o[i] = be_word(&o[4 * i]);
            p.osuf[0] = le_word(&o[32]);
            p.osuf[1] = le_word(&o[36]);
            for (int i = 0; i < 12; i++) p.osuf[2 + i] = le_word(&u[4 * i]);
        }
        c->kind = R == 5 ? K_PDF_R5 : K_PDF_R6;
        return DPRF_OK;
    }
    int n = Length / 8;
    if (R == 2 && (n < 5 || u_len < 32)) return fail(DPRF_E_DOMAIN, "pdf R2: Length %d / U length %d", Length, u_len);
    if (R >= 3 && ((n != 5 && n != 16) || u_len < 16))
        return fail(DPRF_E_DOMAIN, "pdf R%d: key length %d bytes (EVP_rc4 reads 16 key bytes)", R, n);
    p.n = (uint32_t)n;
    for (int i = 0; i < (R == 2 ? 8 : 4); i++) p.u[i] = le_word(&u[4 * i]);
    /* the document-constant tail of the initial MD5 message (get_initial_md5_hash :352-402) */
    std::vector<uint8_t> msg(PDF_PAD, PDF_PAD + 32);   /* placeholder for the 32 password bytes */
    msg.insert(msg.end(), o.begin(), o.end());
    uint32_t pb = (uint32_t)P;
    for (int i = 0; i < 4; i++) msg.push_back((uint8_t)(pb >> (8 * i)));
    msg.insert(msg.end(), id.begin(), id.end());
    if (R >= 4 && !meta)
        for (int i = 0; i < 4; i++) msg.push_back(0xff);
    uint64_t bits = (uint64_t)msg.size() * 8;
    msg.push_back(0x80);
    while (msg.size() % 64 != 56) msg.push_back(0);
    for (int i = 0; i < 8; i++) msg.push_back((uint8_t)(bits >> (8 * i)));
    size_t tail_words = (msg.size() - 32) / 4;
    if (tail_words > DPRF_PDF_TAIL_WORDS) return fail(DPRF_E_DOMAIN, "pdf: O/ID too long (%zu tail words)", tail_words);
    for (size_t i = 0; i < tail_words; i++) p.tail[i] = le_word(&msg[32 + 4 * i]);
    p.tail_blocks = (uint32_t)(msg.size() / 64 - 1);
    /* MD5(PAD || ID) (get_final_md5_hash :404-434) */
    std::vector<uint8_t> m2(PDF_PAD, PDF_PAD + 32);
    m2.insert(m2.end(), id.begin(), id.end());
    uint8_t h2[16];
    md5_host(m2.data(), m2.size(), h2);
    for (int i = 0; i < 4; i++) p.h2[i] = le_word(h2 + 4 * i);
    /* owner check: O[0:32] is the RC4 ciphertext of the padded user password */
    if (o.size() >= 32)
        for (int i = 0; i < 8; i++) p.o[i] = le_word(&o[4 * i]);
    c->kind = K_PDF_R24;
    return DPRF_OK;
}

/* The long-list prehash of each format (k_long_prehash): the first message of its verify().  The family's row names
 * the algorithm; what the algorithm reads of the document is filled here. */
static void set_long_params(dprf_doc *c) {
    dprf_long_params &lp = c->lp;
    memset(&lp, 0, sizeof lp);
    lp.alg = fam(c->kind).long_alg;
    switch (lp.alg) {
        case DPRF_LONG_SHA1_SALT16:
            for (int i = 0; i < 4; i++) lp.prefix[i] = c->office.salt[i];
            break;
        case DPRF_LONG_R5:
        case DPRF_LONG_SHA256_SALT8:
            lp.suffix[0] = c->pdf.u[8];
            lp.suffix[1] = c->pdf.u[9];
            for (int i = 0; i < 8; i++) lp.target[i] = c->pdf.u[i];
            break;
        default: break;
    }
}

int parse_document(dprf_doc *c, const char *const *fields, int nfields) {
    int r;
    const char *tag = fields[0];
    if (!strcmp(tag, "office") && nfields == 8) { c->fmt = DPRF_FMT_OFFICE; r = parse_office(c, fields); }
    else if (!strcmp(tag, "oldoffice") && nfields == 5) { c->fmt = DPRF_FMT_OFFICE; r = parse_oldoffice(c, fields); }
    else if (!strcmp(tag, "odt") && nfields == 7) { c->fmt = DPRF_FMT_ODT; r = parse_odt(c, fields); }
    else if (!strcmp(tag, "odf") && nfields == 12) { c->fmt = DPRF_FMT_ODT; r = parse_odf(c, fields); }
    else if (!strcmp(tag, "pdf") && nfields == 12) { c->fmt = DPRF_FMT_PDF; r = parse_pdf(c, fields); }
    else r = fail(DPRF_E_INVALID, "The input data is not supported (tag '%s', %d fields).", tag, nfields);
    if (r == DPRF_OK) set_long_params(c);
    return r;
}

/* What dprf_ctx_set_pdf_password refuses: a context that is no PDF, an unknown kind, and an owner check that would read
 * more of O and U than the stream holds. */
int check_pdf_password(const dprf_doc *c, int which) {
    if (c->fmt != DPRF_FMT_PDF) return fail(DPRF_E_INVALID, "dprf_ctx_set_pdf_password: not a PDF context");
    if (which != DPRF_PDF_USER && which != DPRF_PDF_OWNER)
        return fail(DPRF_E_INVALID, "dprf_ctx_set_pdf_password: unknown password kind %d", which);
    if (which == DPRF_PDF_OWNER) {
        if (c->has_key40)
            return fail(DPRF_E_INVALID, "dprf_ctx_set_pdf_password: a known key is set (dprf_ctx_set_key40), and a password "
                        "for a known key is a user password (clear the key first)");
        /* what the owner check reads (include/dprf.h); a never-matching context (kind none) reads nothing */
        if (c->kind == K_PDF_R24 && c->pdf_o_len < 32)
            return fail(DPRF_E_DOMAIN, "pdf R%u owner check: O shorter than 32 bytes (%d)", c->pdf.R, c->pdf_o_len);
        if ((c->kind == K_PDF_R5 || c->kind == K_PDF_R6) && (c->pdf_o_len < 48 || c->pdf_u_len < 48))
            return fail(DPRF_E_DOMAIN, "pdf R%u owner check: O (%d bytes) or U (%d bytes) shorter than 48 bytes", c->pdf.R,
                        c->pdf_o_len, c->pdf_u_len);
    }
    return DPRF_OK;
}

/* What dprf_search_key40 refuses (include/dprf.h "40-bit key search"): a window past 2^40, and every document whose
 * RC4 key is not 40 bits long.  A never-matching context (kind none) passes: it answers "no hit" as in every search. */
int check_key40(const dprf_doc *c, uint64_t start, uint64_t count) {
    if (start > DPRF_KEY40_SPACE || count > DPRF_KEY40_SPACE - start)
        return fail(DPRF_E_INVALID, "key window [%llu, +%llu) exceeds the 40-bit key space (2^40 keys)",
                    (unsigned long long)start, (unsigned long long)count);
    return check_key40_domain(c);
}
/* The domain half: dprf_search_key40's, and dprf_ctx_set_key40's -- a known key is a key of the same documents */
int check_key40_domain(const dprf_doc *c) {
    switch (c->kind) {
        case K_NONE: return DPRF_OK;
        case K_PDF_R24:
            /* R2: the reference takes a 5-byte key whatever Length says (pdf...c:161-163) */
            if (c->pdf.R == 2 || c->pdf.n == 5) return DPRF_OK;
            return fail(DPRF_E_DOMAIN, "40-bit key search: pdf R%u with a %u-bit RC4 key (Length %u), not a 40-bit document",
                        c->pdf.R, 8 * c->pdf.n, 8 * c->pdf.n);
        case K_PDF_R5:
        case K_PDF_R6:
            return fail(DPRF_E_DOMAIN, "40-bit key search: pdf R%u is AES-256 under a SHA-2 password hash, not a 40-bit "
                        "document", c->pdf.R);
        case K_OLDOFFICE_MD5: return DPRF_OK;
        case K_OLDOFFICE_SHA1:
            if (c->oldoffice.key_bytes == 5) return DPRF_OK;
            return fail(DPRF_E_DOMAIN, "40-bit key search: Office 97-2003 type 4 (RC4 CryptoAPI) has a 128-bit key, not a "
                        "40-bit document");
        case K_OFFICE:
            return fail(DPRF_E_DOMAIN, "40-bit key search: Office 2007 is AES-128 under 50,000 SHA-1 rounds, not a 40-bit "
                        "document");
        case K_AGILE_SHA1:
        case K_AGILE_SHA512:
            return fail(DPRF_E_DOMAIN, "40-bit key search: Office 2010/2013 Agile Encryption is AES under a spun hash, not "
                        "a 40-bit document");
        case K_ODT:
            return fail(DPRF_E_DOMAIN, "40-bit key search: ODF 1.2 is AES-256 under PBKDF2, not a 40-bit document");
        case K_ODF_AES:
            return fail(DPRF_E_DOMAIN, "40-bit key search: ODF 1.2 is AES-256 under PBKDF2, not a 40-bit document");
        case K_ODF_BF:
            return fail(DPRF_E_DOMAIN, "40-bit key search: ODF 1.0/1.1 is Blowfish with a 128-bit PBKDF2 key, not a 40-bit "
                        "document");
        default: return fail(DPRF_E_DOMAIN, "40-bit key search: not a 40-bit document");
    }
}
/* What dprf_ctx_set_key40 refuses (include/dprf.h "password for a known key"): a document that is not a 40-bit one,
 * and a PDF in owner mode.  Clearing is never refused. */
int check_set_key40(const dprf_doc *c, bool set) {
    if (!set) return DPRF_OK;
    if (const int rc = check_key40_domain(c)) return rc;
    if (c->fmt == DPRF_FMT_PDF && c->pdf.owner)
        return fail(DPRF_E_INVALID, "dprf_ctx_set_key40: the context searches the owner password; a password for a known "
                    "key is a user password (select DPRF_PDF_USER first)");
    return DPRF_OK;
}

/* ------------------------------------------------------------------ range mode and the spelled windows */
/* u32 division by d via multiply-high (round-up method): q = (mulhi(n,m) + ((n - mulhi) >> 1)) >> s */
void fastdiv_magic(uint32_t d, uint32_t &m, uint32_t &s) {
    if (d <= 1) { m = 0; s = 0; return; }
    uint32_t l = 0;
    while ((1ull << l) < d) l++;
    m = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    s = l - 1;
}

/* keyspace bound of range mode and symbol windows: start + count <= radix^pwlen */
int check_power_space(uint64_t start, uint64_t count, int radix, int pwlen) {
    long double space = 1;
    for (int i = 0; i < pwlen; i++) space *= radix;
    if ((long double)start + (long double)count > space)
        return fail(DPRF_E_INVALID, "range [%llu, +%llu) exceeds the keyspace %d^%d", (unsigned long long)start,
                    (unsigned long long)count, radix, pwlen);
    return DPRF_OK;
}

/* The longest candidate of a window, after the cut, must fit a list slot; `detail` ends the message. */
int check_slot(const char *what, uint64_t longest, const char *detail) {
    if (longest <= SLOT_BYTES) return DPRF_OK;
    return fail(DPRF_E_PWLEN, "%s candidates of up to %llu bytes exceed a %u-byte slot%s", what,
                (unsigned long long)longest, SLOT_BYTES, detail);
}

/* One symbol as the kernels read it: LE-packed bytes (Office: the character's UTF-16LE -- exactly one character: its
 * UTF-16LE is what iconv makes of it inside any password) and their count.  pos / k name the symbol in the message
 * (pos < 0: a symbol window, whose symbols belong to no position). */
static_assert(DPRF_MASK_POOL == DPRF_MAX_MASK_SYMBOLS && DPRF_MAX_RANGE_LEN == DPRF_MAX_PW_RANGE,
              "dprf_params.h and include/dprf.h disagree on the mask limits");
int mask_symbol(const dprf_doc *c, const uint8_t *b, size_t n, uint32_t &w, uint32_t &len, int pos, int k) {
    size_t m = n;
    /* the refusal: fmt takes the position prefix, k and m (nothing is formatted for a symbol that passes) */
    auto refuse = [&](const char *fmt) {
        char at[32] = "";
        if (pos >= 0) snprintf(at, sizeof at, "position %d: ", pos);
        return fail(DPRF_E_CHARSET, fmt, at, k, m);
    };
    if (n == 0) return refuse("%ssymbol %d is empty (or offsets not ascending)");
    if (memchr(b, 0, n)) return refuse("%ssymbol %d contains NUL (argv cannot carry it)");
    uint8_t u[8];
    if (c->fmt == DPRF_FMT_OFFICE) {
        const int r = n <= 4 ? utf8_to_utf16le(b, n, u, sizeof u) : -1;
        const bool one = n == 1 || (n == 2 && (b[0] & 0xE0) == 0xC0) || (n == 3 && (b[0] & 0xF0) == 0xE0) ||
                         (n == 4 && (b[0] & 0xF8) == 0xF0);
        if (r < 0 || !one) return refuse("%sOffice symbol %d is not one valid UTF-8 character");
        b = u;
        m = (size_t)r;
    }
    if (m > 4) return refuse("%ssymbol %d has %zu bytes (at most 4)");
    w = 0;
    for (size_t j = 0; j < m; j++) w |= (uint32_t)b[j] << (8 * j);
    len = (uint32_t)m;
    return DPRF_OK;
}

int build_mask_tab(const dprf_doc *c, const uint8_t *sym, const uint32_t *sym_off, const uint32_t *pos_off, int npos,
                   mask_tab &m) {
    /* the table the kernel reads (dprf_params.h): per position {radix, magic, shift, base}, then the pool.  A
     * position whose list equals an earlier one's shares its run of the pool ("?l?l?l?l" holds a-z once). */
    std::vector<uint32_t> &tab = m.tab;
    tab.assign(DPRF_MASK_TAB_WORDS, 0u);
    uint8_t *plen = (uint8_t *)&tab[DPRF_MASK_LENS_AT];
    std::vector<std::vector<uint64_t>> lists((size_t)npos);   /* per position: (count << 32 | word) per symbol */
    uint32_t *radix = m.radix, &npool = m.npool, &sum_longest = m.sum_longest;
    npool = sum_longest = 0;
    for (int p = 0; p < npos; p++) {
        if (pos_off[p + 1] <= pos_off[p]) return fail(DPRF_E_CHARSET, "position %d has no symbol", p);
        const uint32_t r = pos_off[p + 1] - pos_off[p];
        if (r > 256) return fail(DPRF_E_CHARSET, "position %d has %u symbols (at most 256)", p, r);
        std::vector<uint64_t> &li = lists[(size_t)p];
        uint32_t longest = 0;
        for (uint32_t k = 0; k < r; k++) {
            const uint32_t s0 = sym_off[pos_off[p] + k], s1 = sym_off[pos_off[p] + k + 1];
            uint32_t w, len;
            const int rc = mask_symbol(c, sym + s0, s1 > s0 ? s1 - s0 : 0, w, len, p, (int)k);
            if (rc) return rc;
            const uint64_t v = (uint64_t)len << 32 | w;
            for (uint32_t i = 0; i < k; i++)
                if (li[i] == v) return fail(DPRF_E_CHARSET, "position %d: symbols %u and %u are the same", p, i, k);
            li.push_back(v);
            longest = std::max(longest, len);
        }
        sum_longest += longest;
        radix[p] = r;
        int same = -1;
        for (int o = 0; o < p && same < 0; o++)
            if (lists[(size_t)o] == li) same = o;
        uint32_t *rec = &tab[DPRF_MASK_REC_WORDS * p];
        rec[0] = r;
        fastdiv_magic(r, rec[1], rec[2]);
        if (same >= 0) {
            rec[3] = tab[DPRF_MASK_REC_WORDS * same + 3];
            continue;
        }
        if (npool + r > DPRF_MAX_MASK_SYMBOLS)
            return fail(DPRF_E_CHARSET, "the mask's distinct symbol lists hold over %d symbols (at position %d)",
                        DPRF_MAX_MASK_SYMBOLS, p);
        rec[3] = npool;
        for (uint32_t k = 0; k < r; k++) {
            tab[DPRF_MASK_POOL_AT + npool + k] = (uint32_t)li[k];
            plen[npool + k] = (uint8_t)(li[k] >> 32);
        }
        npool += r;
    }
    return DPRF_OK;
}

/* The mask's keyspace, the product of the radices, exactly up to 2^66 where it saturates: above any start + count
 * (< 2^65), so a keyspace of 2^64 or more neither wraps nor refuses a window below 2^64. */
unsigned __int128 mask_space(const uint32_t *radix, int npos) {
    unsigned __int128 space = 1;
    for (int p = 0; p < npos; p++) space = std::min<unsigned __int128>(space * radix[p], (unsigned __int128)1 << 66);
    return space;
}

/* The mixed-radix digits of keyspace index v, the last position fastest, one byte per position packed into sdig
 * (zeroed by the caller).  Returns what is left over: 0 inside a mask's keyspace, the word index of a hybrid one. */
uint64_t start_digits(uint64_t v, const uint32_t *radix, int npos, uint32_t *sdig) {
    for (int p = npos - 1; p >= 0; p--) {
        sdig[p >> 2] |= (uint32_t)(v % radix[p]) << (8 * (p & 3));
        v /= radix[p];
    }
    return v;
}

/* ------------------------------------------------------------------ candidates and words */
/* UTF-8 -> UTF-16LE as iconv("UTF16LE","UTF8") (msoffcrypto...c:275-336); -1 on invalid input */
int utf8_to_utf16le(const uint8_t *s, size_t n, uint8_t *out, size_t cap) {
    size_t o = 0;
    for (size_t i = 0; i < n;) {
        uint32_t cp;
        int k;
        uint8_t b = s[i];
        if (b < 0x80) { cp = b; k = 1; }
        else if ((b & 0xE0) == 0xC0) { cp = b & 0x1F; k = 2; }
        else if ((b & 0xF0) == 0xE0) { cp = b & 0x0F; k = 3; }
        else if ((b & 0xF8) == 0xF0) { cp = b & 0x07; k = 4; }
        else return -1;
        if (i + k > n) return -1;
        for (int j = 1; j < k; j++) {
            if ((s[i + j] & 0xC0) != 0x80) return -1;
            cp = (cp << 6) | (s[i + j] & 0x3F);
        }
        if ((k == 2 && cp < 0x80) || (k == 3 && cp < 0x800) || (k == 4 && (cp < 0x10000 || cp > 0x10FFFF))) return -1;
        if (cp >= 0xD800 && cp <= 0xDFFF) return -1;
        if (cp >= 0x10000) {
            if (o + 4 > cap) return -2;
            uint32_t v = cp - 0x10000, hi = 0xD800 | (v >> 10), lo = 0xDC00 | (v & 0x3FF);
            out[o++] = (uint8_t)hi; out[o++] = (uint8_t)(hi >> 8); out[o++] = (uint8_t)lo; out[o++] = (uint8_t)(lo >> 8);
        } else {
            if (o + 2 > cap) return -2;
            out[o++] = (uint8_t)cp; out[o++] = (uint8_t)(cp >> 8);
        }
        i += k;
    }
    return (int)o;
}

/* A candidate as the reference's verifier hashes it: UTF-16LE (Office, iconv at msoffcrypto...c:80), truncated at 32
 * bytes (PDF R<=4, pdf...c:137) or 127 (PDF R5, :197-200), as given otherwise.  *out points into pw or tmp.
 * Returns 0 or the DPRF_E_* code of a candidate the reference cannot verify:
 *   NUL                         argv cannot carry it (the reference receives candidates as argv strings)
 *   > DPRF_MAX_PW bytes         no argv string can be that long (Linux MAX_ARG_STRLEN), the verifier never runs
 *   Office "" / invalid UTF-8   the iconv path leaves the length uninitialised / reads freed memory (:287-336)
 *   R6 > DPRF_MAX_PW_R6 bytes   64 x (pw || K) overflows data[(128 + 64 + 48) * 64] (pdf...c:228): the reference
 *                               aborts ("stack smashing detected", measured; tests/golden/long_verdicts.json) */
int convert_candidate(const dprf_doc *c, const uint8_t *pw, size_t len, const uint8_t **out, size_t *olen,
                      std::vector<uint8_t> &tmp) {
    if (memchr(pw, 0, len)) return DPRF_E_INVALID;
    if (len > DPRF_MAX_PW) return DPRF_E_PWLEN;
    const family &f = fam(c->kind);
    *out = pw;
    *olen = len;
    if (c->fmt == DPRF_FMT_OFFICE) {
        if (len == 0) return DPRF_E_DOMAIN;
        if (tmp.size() < 2 * len) tmp.resize(2 * len);
        const int u = utf8_to_utf16le(pw, len, tmp.data(), tmp.size());
        if (u < 0) return DPRF_E_DOMAIN;
        *out = tmp.data();
        *olen = (size_t)u;
    } else {
        *olen = std::min<size_t>(len, f.trunc);
    }
    /* a family without a long-list prehash yet (Agile, Office 97-2003, ODF 1.0 / 1.1): candidates over the slot (more
     * than 64 bytes, 32 UTF-16 units) are refused */
    if (f.no_long && *olen > SLOT_BYTES) return DPRF_E_PWLEN;
    if (c->kind == K_PDF_R6 && len > DPRF_MAX_PW_R6) return DPRF_E_DOMAIN;
    /* owner search, R5/R6 (the PDF families with a long list): the long-list prehash appends the 8 salt bytes only, not
     * salt || U[0:48] -- candidates longer than a slot are refused for now */
    if (c->pdf.owner && f.long_alg && *olen > SLOT_BYTES) return DPRF_E_PWLEN;
    return DPRF_OK;
}
const char *status_text(int code, const dprf_doc *c, size_t len) {
    if (code == DPRF_E_PWLEN && c && len <= DPRF_MAX_PW) {
        if (c->pdf.owner)
            return "longer than 64 bytes: long owner-password candidates (PDF R5/R6) are not supported yet";
        if (fam(c->kind).no_long) return fam(c->kind).no_long;
    }
    switch (code) {
        case DPRF_E_INVALID: return "contains NUL (argv cannot carry it)";
        case DPRF_E_DOMAIN:
            return "empty or invalid UTF-8 Office password (the reference's iconv path is undefined), or a PDF R6 "
                   "password over 176 bytes (the reference overflows its data buffer and aborts)";
        case DPRF_E_PWLEN: return "longer than 131,071 bytes (no argv string can carry it to the reference's verifier)";
        default: return "invalid";
    }
}

/* A word of the table as the kernels spell it: the bytes as given, for Office their UTF-16LE (any number of
 * characters).  0, or DPRF_E_DOMAIN for a word no candidate can contain: empty, with NUL, or (Office) invalid UTF-8. */
int convert_word(const dprf_doc *c, const uint8_t *w, size_t len, const uint8_t **out, size_t *olen,
                 std::vector<uint8_t> &tmp) {
    if (len == 0 || memchr(w, 0, len)) return DPRF_E_DOMAIN;
    *out = w;
    *olen = len;
    if (c->fmt != DPRF_FMT_OFFICE) return DPRF_OK;
    if (tmp.size() < 2 * len) tmp.resize(2 * len);
    const int u = utf8_to_utf16le(w, len, tmp.data(), tmp.size());
    if (u <= 0) return DPRF_E_DOMAIN;
    *out = tmp.data();
    *olen = (size_t)u;
    return DPRF_OK;
}
const char *word_text(const uint8_t *w, size_t len) {
    if (len == 0) return "is empty";
    if (memchr(w, 0, len)) return "contains NUL (argv cannot carry it)";
    return "is not valid UTF-8 (an Office password is converted to UTF-16LE)";
}

/* ------------------------------------------------------------------ rule windows */
static_assert(DPRF_RULE_FNS == DPRF_MAX_RULE_FNS, "dprf_params.h and include/dprf.h disagree on the rule limits");

/* The parameters of a rule function (include/dprf.h "rule mode"): N / M positions 0..35, X / Y units; null for a byte
 * that is no function of the language. */
static const char *rule_signature(uint32_t op) {
    switch (op) {
        case ':': case 'l': case 'u': case 'c': case 'C': case 't': case 'E': case 'r': case 'd': case 'f': case '{':
        case '}': case 'q': case 'k': case 'K': case '[': case ']':
            return "";
        case 'T': case 'p': case 'D': case '\'': case 'z': case 'Z': case 'y': case 'Y': case '.': case ',':
            return "N";
        case '*': case 'x': case 'O':
            return "NM";
        case '$': case '^': case '@':
            return "X";
        case 'i': case 'o':
            return "NX";
        case 's':
            return "XY";
        default:
            return nullptr;
    }
}

/* What dprf_search_rules and dprf_spell_rules refuse alike; `who` names the export. */
int check_rules(const dprf_doc *c, const char *who, const uint32_t *fns, const uint32_t *rule_off, int64_t nrules,
                uint64_t start, uint64_t count) {
    if (!fns || !rule_off) return fail(DPRF_E_INVALID, "%s: null argument", who);
    if (c->nwords == 0) return fail(DPRF_E_INVALID, "%s: the context has no word table (dprf_ctx_set_words)", who);
    if (nrules < 1 || nrules > DPRF_MAX_RULES)
        return fail(DPRF_E_INVALID, "%lld rules (1..%d)", (long long)nrules, DPRF_MAX_RULES);
    for (int64_t k = 0; k < nrules; k++) {
        if (rule_off[k + 1] < rule_off[k]) return fail(DPRF_E_INVALID, "rule offsets not ascending at rule %lld", (long long)k);
        const uint32_t nf = rule_off[k + 1] - rule_off[k];
        if (nf < 1 || nf > DPRF_MAX_RULE_FNS)
            return fail(DPRF_E_INVALID, "rule %lld has %u functions (1..%d)", (long long)k, nf, DPRF_MAX_RULE_FNS);
        if (rule_off[k + 1] > DPRF_MAX_RULE_WORDS)
            return fail(DPRF_E_INVALID, "the rule table holds over %d functions (at rule %lld)", DPRF_MAX_RULE_WORDS,
                        (long long)k);
    }
    const bool office = c->fmt == DPRF_FMT_OFFICE;
    for (int64_t k = 0; k < nrules; k++)
        for (uint32_t f = rule_off[k]; f < rule_off[k + 1]; f++) {
            const uint32_t w = fns[f], op = w & 0xffu, par[2] = {(w >> 8) & 0xffu, (w >> 16) & 0xffu};
            const int fi = (int)(f - rule_off[k]);
            const char *sig = rule_signature(op);
            if (!sig)
                return fail(DPRF_E_CHARSET, "rule %lld, function %d: byte 0x%02x is no function of the rule language",
                            (long long)k, fi, op);
            const size_t np = strlen(sig);
            for (size_t j = 0; j < 2; j++) {
                if (j >= np) {
                    if (par[j]) return fail(DPRF_E_CHARSET, "rule %lld, function %d ('%c'): unused parameter bits are set",
                                            (long long)k, fi, (int)op);
                } else if (sig[j] == 'N' || sig[j] == 'M') {
                    if (par[j] > 35)
                        return fail(DPRF_E_CHARSET, "rule %lld, function %d ('%c'): position %u (0..35)", (long long)k, fi,
                                    (int)op, par[j]);
                } else if (par[j] == 0) {
                    return fail(DPRF_E_CHARSET, "rule %lld, function %d ('%c'): NUL cannot be a unit", (long long)k, fi,
                                (int)op);
                } else if (office && par[j] >= 0x80) {
                    return fail(DPRF_E_CHARSET, "rule %lld, function %d ('%c'): Office takes the units 0x01..0x7F, not 0x%02x",
                                (long long)k, fi, (int)op, par[j]);
                }
            }
            if (w >> 24)
                return fail(DPRF_E_CHARSET, "rule %lld, function %d ('%c'): unused parameter bits are set", (long long)k, fi,
                            (int)op);
        }
    /* a rule may move a word's tail to the front, so the copy clipped to a slot that hybrid search tolerates for
     * R2-R4 is not enough here: every word must fit the slot whole */
    if (c->w_longest > SLOT_BYTES)
        return fail(DPRF_E_PWLEN, "word %llu takes %llu converted bytes: rules apply to words of at most %u",
                    (unsigned long long)c->w_longest_idx, (unsigned long long)c->w_longest, SLOT_BYTES);
    if ((unsigned __int128)start + count > (unsigned __int128)c->nwords * (uint64_t)nrules)
        return fail(DPRF_E_INVALID, "window [%llu, +%llu) exceeds the rule keyspace of %llu words times %lld rules",
                    (unsigned long long)start, (unsigned long long)count, (unsigned long long)c->nwords,
                    (long long)nrules);
    return DPRF_OK;
}

/* An upper bound, in bytes, of the candidates the validated rules make of the table's words: the list kernels take the
 * launch's longest candidate (R5 picks its message width by it, R6 its period lengths), so a bound tighter than the slot
 * keeps rule mode at the rate of the candidates it really makes.  Per rule, the longest word's length in units goes
 * through the functions that lengthen ($ ^ i by one, d f q twice, pN N + 1 times, z Z by N, y Y by N when N fits); a
 * function whose result would pass LIMIT leaves that word unchanged, but a shorter word may then reach LIMIT itself, so
 * the bound becomes LIMIT.  Everything else keeps or shortens. */
uint32_t rules_longest(const dprf_doc *c, const uint32_t *fns, const uint32_t *rule_off, int64_t nrules) {
    const uint32_t unit = c->fmt == DPRF_FMT_OFFICE ? 2u : 1u, limit = SLOT_BYTES / unit;
    const uint32_t n0 = std::max<uint32_t>(1u, (uint32_t)c->w_longest / unit);
    uint32_t best = n0;
    for (int64_t k = 0; k < nrules && best < limit; k++) {
        uint32_t n = n0;
        for (uint32_t f = rule_off[k]; f < rule_off[k + 1]; f++) {
            const uint32_t op = fns[f] & 0xffu, N = (fns[f] >> 8) & 0xffu;
            uint32_t m = n;
            switch (op) {
                case '$': case '^': case 'i': m = n + 1u; break;
                case 'd': case 'f': case 'q': m = 2u * n; break;
                case 'p': m = n * (N + 1u); break;
                case 'z': case 'Z': m = n + N; break;
                case 'y': case 'Y': m = N <= n ? n + N : n; break;
                default: break;
            }
            n = std::min(m, limit);
        }
        best = std::max(best, n);
    }
    return std::min<uint32_t>(best * unit, fam(c->kind).trunc);
}

/* ------------------------------------------------------------------ combinator windows */
int check_combine(const dprf_doc *c, const char *who, uint64_t start, uint64_t count) {
    if (c->nwords == 0) return fail(DPRF_E_INVALID, "%s: the context has no left word table (dprf_ctx_set_words)", who);
    if (c->nright == 0)
        return fail(DPRF_E_INVALID, "%s: the context has no right word table (dprf_ctx_set_right_words)", who);
    if ((unsigned __int128)start + count > (unsigned __int128)c->nwords * c->nright)
        return fail(DPRF_E_INVALID, "window [%llu, +%llu) exceeds the combinator keyspace of %llu left times %llu right words",
                    (unsigned long long)start, (unsigned long long)count, (unsigned long long)c->nwords,
                    (unsigned long long)c->nright);
    /* the sum cannot wrap: a table's converted bytes stay below 2^32 in all */
    const uint64_t longest = std::min<uint64_t>(c->w_longest + c->r_longest, fam(c->kind).trunc);
    if (longest > SLOT_BYTES) {
        char detail[160];
        snprintf(detail, sizeof detail, ": left word %llu takes %llu bytes, right word %llu takes %llu",
                 (unsigned long long)c->w_longest_idx, (unsigned long long)c->w_longest,
                 (unsigned long long)c->r_longest_idx, (unsigned long long)c->r_longest);
        return check_slot("combinator", longest, detail);
    }
    return DPRF_OK;
}

uint32_t combine_longest(const dprf_doc *c) {
    return (uint32_t)std::min<uint64_t>(std::min<uint64_t>(c->w_longest + c->r_longest, fam(c->kind).trunc), SLOT_BYTES);
}

}   // namespace dprf_internal

/* ------------------------------------------------------------------ ABI: chunk planning by family name */
extern "C" uint64_t dprf_plan_chunk(const char *kernel, double rate_per_ms, uint64_t remaining, uint64_t total,
                                    int ndev, int inflight) {
    using namespace dprf_internal;
    if (!kernel) return 0;
    for (int k = K_NONE + 1; k < K_COUNT; k++) {
        const family &f = FAMILIES[k];
        const bool owner = f.owner_name && !strcmp(kernel, f.owner_name);
        const bool collide = f.collide_name && !strcmp(kernel, f.collide_name);
        /* a key search plans with the password family's policy (dprf_doc.h key40_name) */
        if (owner || collide || !strcmp(kernel, f.name) || (f.key40_name && !strcmp(kernel, f.key40_name)))
            return plan_chunk((kernel_kind)k, owner, rate_per_ms, remaining, total, ndev, inflight, collide);
    }
    return 0;
}
