/* dprf_kernels_agile.hip -- Office 2010 / 2013 Agile Encryption, password key encryptor
 * (MS-OFFCRYPTO 2.3.4.11-2.3.4.13), one candidate per lane, two launches per batch as k_office_kdf +
 * k_office_check:
 *   k_agile_kdf<MODE, SHA512>     h = H(salt || UTF16LE(pw)); spinCount x h = H(LE32(i) || h);
 *                                 key1 = H(h || fe a7 d2 76 3b 4b 9e 79), key2 = H(h || d7 aa 0f 6d 30 61 34 4e),
 *                                 each cut (SHA-1 with 256 bits: padded with 0x36) to keyBits / 8 bytes
 *   k_agile_check<SHA512, KEY256> vin = AES-CBC-dec(key1, iv = salt, encryptedVerifierHashInput) (one block),
 *                                 vhv = AES-CBC-dec(key2, iv = salt, encryptedVerifierHashValue[0:32]) (two blocks);
 *                                 a hit when H(vin)[0:n] == vhv[0:n], n = 20 (SHA-1) or 32 (SHA-512)
 * H is SHA-1 for the "2010" stream and SHA-512 for "2013".  No reference verifier exists for this format: the
 * definition is pinned by tests/agile_model.py and the public vectors in tests/golden/agile_vectors.json.
 *
 * A translation unit of its own: the kernels measured by bench.py (dprf_kernels.hip, dprf_kernels_r6.hip) keep their
 * objects untouched.  The candidate source, the block prologue and be_append are dprf_cand.h's.
 */
#include "dev_crypto.h"
#include "dprf_params.h"
#include "dprf_launch.h"
#include "dprf_hits.h"
#include "dprf_cand.h"

namespace {
/* the two block keys of 2.3.4.13 as BE words */
constexpr uint32_t BK1_HI = 0xfea7d276u, BK1_LO = 0x3b4b9e79u;   /* verifier hash input */
constexpr uint32_t BK2_HI = 0xd7aa0f6du, BK2_LO = 0x3061344eu;   /* verifier hash value */

/* SHA-1 of h[0:20] || 8 block-key bytes (28 bytes, one block) */
DEVI void sha1_h_blockkey(const uint32_t h[5], uint32_t bhi, uint32_t blo, uint32_t out[5]) {
    uint32_t w[16] = {h[0], h[1], h[2], h[3], h[4], bhi, blo, 0x80000000u, 0, 0, 0, 0, 0, 0, 0, 224u};
    sha1_iv(out);
    sha1_compress(out, w);
}
/* SHA-512 of h[0:64] || 8 block-key bytes (72 bytes, one block) */
DEVI void sha512_h_blockkey(const uint64_t h[8], uint32_t bhi, uint32_t blo, uint64_t out[8]) {
    uint64_t w[16];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = h[k];
    w[8] = pack64(bhi, blo);
    w[9] = pack64(0x80000000u, 0u);
#pragma unroll
    for (int k = 10; k < 15; k++) w[k] = 0ull;
    w[15] = pack64(0u, 576u);
    sha512_iv(out, false);
    sha512_compress(out, w);
}

/* ------------------------------------------------------------------ SHA-512 with the constants folded
 * sha512_compress adds with inline assembly (dev_crypto.h add64: one v_lshl_add_u64), which the compiler cannot fold.
 * In the spin loop the compression starts from the constant initial state and seven of its 16 message words are
 * constants (six zeros and the bit length), so a good part of the first rounds and of the first schedule pass is
 * constant work.  This restatement of the same compression sums through ksum, which lets the compiler add the
 * compile-time constants of a sum and spends one instruction per variable term (the constant rides in an SGPR pair),
 * and takes the sigmas of constant words in plain C.  With no constant among the terms the sums keep
 * sha512_compress's tree shape. */
#ifndef AGILE_SHA512_FOLD
#define AGILE_SHA512_FOLD 1
#endif
struct ksum {
    uint64_t k = 0, v = 0;
    bool have = false;
};
DEVI void ks_add(ksum &s, uint64_t x) {
    if (CONSTP(x)) { s.k += x; return; }
    s.v = s.have ? add64(s.v, x) : x;
    s.have = true;
}
DEVI uint64_t ks_done(const ksum &s) {
    if (!s.have) return s.k;
    return s.k == 0 ? s.v : add64k(s.v, s.k);
}
/* a + b + c + d + k, k a compile-time constant */
DEVI uint64_t sum4k(uint64_t a, uint64_t b, uint64_t c, uint64_t d, uint64_t k) {
    if (!CONSTP(a) && !CONSTP(b) && !CONSTP(c) && !CONSTP(d))
        return add64(add64(a, b), add64(c, k == 0 ? d : add64k(d, k)));
    ksum s;
    s.k = k;
    ks_add(s, a); ks_add(s, b); ks_add(s, c); ks_add(s, d);
    return ks_done(s);
}
DEVI uint64_t sum2(uint64_t a, uint64_t b) {
    if (!CONSTP(a) && !CONSTP(b)) return add64(a, b);
    ksum s;
    ks_add(s, a); ks_add(s, b);
    return ks_done(s);
}
constexpr uint64_t rorc(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
DEVI uint64_t sig0_512(uint64_t x) {
    if (CONSTP(x)) return rorc(x, 1) ^ rorc(x, 8) ^ (x >> 7);
    return xor3_64(ror64(x, 1), ror64(x, 8), shr64(x, 7));
}
DEVI uint64_t sig1_512(uint64_t x) {
    if (CONSTP(x)) return rorc(x, 19) ^ rorc(x, 61) ^ (x >> 6);
    return xor3_64(ror64(x, 19), ror64(x, 61), shr64(x, 6));
}
DEVI uint64_t Sig0_512(uint64_t x) {
    if (CONSTP(x)) return rorc(x, 28) ^ rorc(x, 34) ^ rorc(x, 39);
    return xor3_64(ror64(x, 28), ror64(x, 34), ror64(x, 39));
}
DEVI uint64_t Sig1_512(uint64_t x) {
    if (CONSTP(x)) return rorc(x, 14) ^ rorc(x, 18) ^ rorc(x, 41);
    return xor3_64(ror64(x, 14), ror64(x, 18), ror64(x, 41));
}
DEVI uint64_t ch64c(uint64_t a, uint64_t b, uint64_t c) {
    if (CONSTP(a) && CONSTP(b) && CONSTP(c)) return (a & b) | (~a & c);
    return ch64(a, b, c);
}
DEVI uint64_t maj64c(uint64_t a, uint64_t b, uint64_t c) {
    if (CONSTP(a) && CONSTP(b) && CONSTP(c)) return (a & b) | (a & c) | (b & c);
    return maj64(a, b, c);
}
/* out = IV + compression of w from IV (w is overwritten by the schedule) */
DEVI void sha512_from_iv_folded(uint64_t out[8], uint64_t w[16]) {
    constexpr uint64_t IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                                0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                                0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
    uint64_t a = IV[0], b = IV[1], c = IV[2], d = IV[3], e = IV[4], f = IV[5], g = IV[6], h = IV[7];
#pragma clang loop unroll(full)
    for (int t = 0; t < 80; t++) {
        uint64_t wt;
        if (t < 16) {
            wt = w[t];
        } else {
            wt = sum4k(w[t & 15], sig0_512(w[(t - 15) & 15]), w[(t - 7) & 15], sig1_512(w[(t - 2) & 15]), 0ull);
            w[t & 15] = wt;
        }
        const uint64_t t1 = sum4k(h, Sig1_512(e), ch64c(e, f, g), wt, k512(t));
        const uint64_t t2 = sum2(Sig0_512(a), maj64c(a, b, c));
        h = g; g = f; f = e; e = sum2(d, t1); d = c; c = b; b = a; a = sum2(t1, t2);
    }
    out[0] = add64k(a, IV[0]); out[1] = add64k(b, IV[1]); out[2] = add64k(c, IV[2]); out[3] = add64k(d, IV[3]);
    out[4] = add64k(e, IV[4]); out[5] = add64k(f, IV[5]); out[6] = add64k(g, IV[6]); out[7] = add64k(h, IV[7]);
}
}  // namespace

/* ================================================================== key derivation */
/* waves per SIMD the register allocation must allow: SHA-1 runs k_office_kdf's loop (<= 64 VGPRs, 8 waves); the
 * SHA-512 compression holds 8 + 16 64-bit values and its temporaries (<= 128 VGPRs, 4 waves) */
#ifndef AGILE_SHA1_WAVES
#define AGILE_SHA1_WAVES 8
#endif
#ifndef AGILE_SHA512_WAVES
#define AGILE_SHA512_WAVES 4
#endif

/* keys: [word][candidate], words 0..nk-1 key1, nk..2nk-1 key2, nk = keyBits / 32 (BE words) */
template <int MODE>
DEVI void agile_kdf_sha1(const dprf_enum &e, const dprf_agile_params &p, const uint8_t *cs, uint32_t g, uint32_t *keys) {
    uint32_t h[5];
    {
        cand c;
        get_candidate<MODE, true>(e, cs, g, c);
        /* h = SHA1(salt || UTF16LE(pw)): 16 + up to 64 bytes, one or two blocks chosen per lane */
        uint32_t m[32];
        m[0] = p.salt[0]; m[1] = p.salt[1]; m[2] = p.salt[2]; m[3] = p.salt[3];
        be_append<4>(m, c);
        const uint32_t total = 16u + c.len, bits = total * 8u;
        const bool two = total > 55u;
        uint32_t b0[16], b1[16];
#pragma unroll
        for (int j = 0; j < 16; j++) { b0[j] = m[j]; b1[j] = m[16 + j]; }
        if (!two) b0[15] = bits;
        b1[15] = bits;
        sha1_iv(h);
        sha1_compress(h, b0);
        if (two) sha1_compress(h, b1);
    }
    /* spinCount x h = SHA1(LE32(i) || h): a 24-byte message, W0 = bswap(i) is wave-uniform */
    for (uint32_t i = 0; i < p.spin; i++) {
        uint32_t w[16] = {bswap32(i), h[0], h[1], h[2], h[3], h[4], 0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 192u};
        uint32_t s[5];
        sha1_iv(s);
        sha1_compress(s, w);
        h[0] = s[0]; h[1] = s[1]; h[2] = s[2]; h[3] = s[3]; h[4] = s[4];
    }
    uint32_t k1[5], k2[5];
    sha1_h_blockkey(h, BK1_HI, BK1_LO, k1);
    sha1_h_blockkey(h, BK2_HI, BK2_LO, k2);
    const size_t n = e.count;
    if (p.key_words == 4u) {
#pragma unroll
        for (int k = 0; k < 4; k++) { keys[(size_t)k * n + g] = k1[k]; keys[(size_t)(4 + k) * n + g] = k2[k]; }
    } else {
        /* 256-bit key from a 20-byte hash: padded with 0x36 up to 32 bytes */
#pragma unroll
        for (int k = 0; k < 8; k++) {
            keys[(size_t)k * n + g] = k < 5 ? k1[k < 5 ? k : 0] : 0x36363636u;
            keys[(size_t)(8 + k) * n + g] = k < 5 ? k2[k < 5 ? k : 0] : 0x36363636u;
        }
    }
}

template <int MODE>
DEVI void agile_kdf_sha512(const dprf_enum &e, const dprf_agile_params &p, const uint8_t *cs, uint32_t g, uint32_t *keys) {
    uint64_t h[8];
    {
        cand c;
        get_candidate<MODE, true>(e, cs, g, c);
        /* h = SHA512(salt || UTF16LE(pw)): at most 80 bytes, always one 128-byte block */
        uint32_t m[32];
        m[0] = p.salt[0]; m[1] = p.salt[1]; m[2] = p.salt[2]; m[3] = p.salt[3];
        be_append<4>(m, c);
        uint64_t w[16];
#pragma unroll
        for (int k = 0; k < 15; k++) w[k] = pack64(m[2 * k], m[2 * k + 1]);
        w[15] = pack64(0u, (16u + c.len) * 8u);
        sha512_iv(h, false);
        sha512_compress(h, w);
    }
    /* spinCount x h = SHA512(LE32(i) || h): 68 bytes, the state shifted by half a word against the message words --
     * with 32-bit halves in registers the shift is only a different pairing of them */
    for (uint32_t i = 0; i < p.spin; i++) {
        uint64_t w[16];
        w[0] = pack64(bswap32(i), hi32(h[0]));
#pragma unroll
        for (int k = 1; k < 8; k++) w[k] = pack64(lo32(h[k - 1]), hi32(h[k]));
        w[8] = pack64(lo32(h[7]), 0x80000000u);
#pragma unroll
        for (int k = 9; k < 15; k++) w[k] = 0ull;
        w[15] = pack64(0u, 544u);
        uint64_t s[8];
#if AGILE_SHA512_FOLD
        sha512_from_iv_folded(s, w);
#else
        sha512_iv(s, false);
        sha512_compress(s, w);
#endif
#pragma unroll
        for (int k = 0; k < 8; k++) h[k] = s[k];
    }
    const size_t n = e.count;
    const uint32_t nk = p.key_words;   /* 4 or 8 */
    {
        uint64_t k1[8];
        sha512_h_blockkey(h, BK1_HI, BK1_LO, k1);
#pragma unroll
        for (int k = 0; k < 8; k++)
            if ((uint32_t)k < nk) keys[(size_t)k * n + g] = (k & 1) ? lo32(k1[k >> 1]) : hi32(k1[k >> 1]);
    }
    {
        uint64_t k2[8];
        sha512_h_blockkey(h, BK2_HI, BK2_LO, k2);
#pragma unroll
        for (int k = 0; k < 8; k++)
            if ((uint32_t)k < nk) keys[(size_t)(nk + k) * n + g] = (k & 1) ? lo32(k2[k >> 1]) : hi32(k2[k >> 1]);
    }
}

template <int MODE, bool SHA512>
__global__ void __launch_bounds__(256, SHA512 ? AGILE_SHA512_WAVES : AGILE_SHA1_WAVES)
k_agile_kdf(dprf_enum e, dprf_agile_params p, dprf_results *R, uint32_t stop_on_first, uint32_t *keys) {
    __shared__ uint8_t cs[256];
    __shared__ uint32_t flag;
    if (!block_prologue<false, false>(e, nullptr, R, stop_on_first, cs, nullptr, &flag)) return;
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.count) return;
    if constexpr (SHA512) agile_kdf_sha512<MODE>(e, p, cs, g, keys);
    else agile_kdf_sha1<MODE>(e, p, cs, g, keys);
}

/* ================================================================== verifier check */
template <bool KEY256>
DEVI void agile_dec_schedule(const aes_lds &L, const uint32_t *key, uint32_t *dk) {
    constexpr int NR = KEY256 ? 14 : 10;
    uint32_t rk[4 * (NR + 1)];
    if constexpr (KEY256) aes256_expand(L, key, rk);
    else aes128_expand(L, key, rk);
    aes_dec_schedule<NR>(L, rk, dk);
}

template <bool SHA512, bool KEY256>
__global__ void __launch_bounds__(256)
k_agile_check(dprf_enum e, dprf_agile_params p, const dprf_aes_tables *T, dprf_results *R, uint32_t cap,
              uint32_t stop_on_first, const uint32_t *keys) {
    constexpr int NK = KEY256 ? 8 : 4, NR = KEY256 ? 14 : 10;
    __shared__ uint8_t cs[256];
    __shared__ aes_lds L;
    __shared__ uint32_t flag;
    if (!block_prologue<true, true>(e, T, R, stop_on_first, cs, &L, &flag)) return;
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = g < e.count;
    const size_t n = e.count;
    uint32_t vin[4], v0[4], v1[4];
    {
        /* vin = D(key1, encryptedVerifierHashInput) ^ salt */
        uint32_t key[NK], dk[4 * (NR + 1)];
#pragma unroll
        for (int k = 0; k < NK; k++) key[k] = valid ? keys[(size_t)k * n + g] : 0u;
        agile_dec_schedule<KEY256>(L, key, dk);
        aes_decrypt<NR>(L, dk, p.evi, vin);
#pragma unroll
        for (int k = 0; k < 4; k++) vin[k] ^= p.salt[k];
    }
    {
        /* vhv = D(key2, encryptedVerifierHashValue[0:32]), CBC: block 0 ^ salt, block 1 ^ ciphertext block 0 */
        uint32_t key[NK], dk[4 * (NR + 1)];
#pragma unroll
        for (int k = 0; k < NK; k++) key[k] = valid ? keys[(size_t)(NK + k) * n + g] : 0u;
        agile_dec_schedule<KEY256>(L, key, dk);
        aes_decrypt<NR>(L, dk, p.evh, v0);
        aes_decrypt<NR>(L, dk, p.evh + 4, v1);
#pragma unroll
        for (int k = 0; k < 4; k++) { v0[k] ^= p.salt[k]; v1[k] ^= p.evh[k]; }
    }
    bool ok;
    if constexpr (SHA512) {
        /* SHA512(vin)[0:32] == vhv[0:32] */
        uint64_t w[16], s[8];
        w[0] = pack64(vin[0], vin[1]);
        w[1] = pack64(vin[2], vin[3]);
        w[2] = pack64(0x80000000u, 0u);
#pragma unroll
        for (int k = 3; k < 15; k++) w[k] = 0ull;
        w[15] = pack64(0u, 128u);
        sha512_iv(s, false);
        sha512_compress(s, w);
        ok = hi32(s[0]) == v0[0] && lo32(s[0]) == v0[1] && hi32(s[1]) == v0[2] && lo32(s[1]) == v0[3] &&
             hi32(s[2]) == v1[0] && lo32(s[2]) == v1[1] && hi32(s[3]) == v1[2] && lo32(s[3]) == v1[3];
    } else {
        /* SHA1(vin) == vhv[0:20] */
        uint32_t s[5];
        uint32_t w[16] = {vin[0], vin[1], vin[2], vin[3], 0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 128u};
        sha1_iv(s);
        sha1_compress(s, w);
        ok = s[0] == v0[0] && s[1] == v0[1] && s[2] == v0[2] && s[3] == v0[3] && s[4] == v1[0];
    }
    if (valid && ok) report_hit(e, R, e.start + g, cap, stop_on_first);
}

/* ------------------------------------------------------------------ launcher */
hipError_t launch_agile(const dprf_enum &e, const dprf_agile_params &p, const dprf_aes_tables *T, dprf_results *R,
                        uint32_t cap, uint32_t stop, hipStream_t s, uint32_t *keys, hipEvent_t mid) {
    /* the host refuses Agile candidates longer than a slot: no long-list mode */
    if (e.mode > 1u || (p.key_words != 4u && p.key_words != 8u)) return hipErrorInvalidValue;
    const dim3 grid = GRID(e.count, 256), block(256);
    if (p.sha512) {
        if (e.mode == 0) hipLaunchKernelGGL((k_agile_kdf<0, true>), grid, block, 0, s, e, p, R, stop, keys);
        else hipLaunchKernelGGL((k_agile_kdf<1, true>), grid, block, 0, s, e, p, R, stop, keys);
    } else {
        if (e.mode == 0) hipLaunchKernelGGL((k_agile_kdf<0, false>), grid, block, 0, s, e, p, R, stop, keys);
        else hipLaunchKernelGGL((k_agile_kdf<1, false>), grid, block, 0, s, e, p, R, stop, keys);
    }
    if (mid) (void)hipEventRecord(mid, s);
    if (p.sha512) {
        if (p.key_words == 8u) hipLaunchKernelGGL((k_agile_check<true, true>), grid, block, 0, s, e, p, T, R, cap, stop, keys);
        else hipLaunchKernelGGL((k_agile_check<true, false>), grid, block, 0, s, e, p, T, R, cap, stop, keys);
    } else {
        if (p.key_words == 8u) hipLaunchKernelGGL((k_agile_check<false, true>), grid, block, 0, s, e, p, T, R, cap, stop, keys);
        else hipLaunchKernelGGL((k_agile_check<false, false>), grid, block, 0, s, e, p, T, R, cap, stop, keys);
    }
    return hipGetLastError();
}
