/* dprf_kernels.hip -- gfx950 verification kernels, one candidate per lane.
 *
 * Each kernel restates one reference verify() for a batch of candidates:
 *   k_office_kdf + k_office_check   msoffcrypto_password_verifier.c:56-191  (SHA-1 x50,002; AES-128-ECB check)
 *   k_odt_kdf + k_odt_check         odt_password_verifier.c:51-126  (SHA-256, PBKDF2-HMAC-SHA1 x1024; AES-256-CBC)
 *   k_pdf_r24  pdf_password_verifier.c:134-191         (MD5 [x50] + RC4 [x20], S-box in LDS)
 *   k_pdf_r5   pdf_password_verifier.c:194-221         (one SHA-256)
 *   k_pdf_r6   pdf_password_verifier.c:226-291         (dprf_kernels_r6.hip)
 * Candidates come either from on-device enumeration of a keyspace index (range mode, the
 * brute_force.py -pr path) or from a packed slot buffer (list mode, the client payload path).
 * A hit appends its index to a device buffer (atomic), lowers `first` (atomicMin) and, when asked,
 * raises a stop flag that later launches of the same call observe and skip.
 */
#include "dev_crypto.h"
#include "dprf_params.h"
#include "dprf_launch.h"
#include "dprf_hits.h"
#include "dprf_cand.h"
#include "rc4_wg.h"

/* The candidate source, the block prologue and be_append are dprf_cand.h's.  The kernels of this file read a list
 * candidate's length byte unclamped (get_candidate<MODE, UTF16, LIST_CLAMP>): the four objects built from it are the
 * measured ones and keep their machine code, and the host never packs more than a slot. */
#define LIST_CLAMP false

/* SHA-1 / SHA-256 of a <= 119-byte message held in m[32] (BE, already terminated with 0x80):
 * one or two blocks, chosen per lane. */
DEVI void sha1_msg2(uint32_t m[32], uint32_t total, uint32_t out[5]) {
    const uint32_t bits = total * 8u;
    const bool two = total > 55u;
    uint32_t b0[16], b1[16];
#pragma unroll
    for (int j = 0; j < 16; j++) { b0[j] = m[j]; b1[j] = m[16 + j]; }
    if (!two) b0[15] = bits;
    b1[15] = bits;
    sha1_iv(out);
    sha1_compress(out, b0);
    if (two) sha1_compress(out, b1);
}
DEVI void sha256_msg2(uint32_t m[32], uint32_t total, uint32_t out[8]) {
    const uint32_t bits = total * 8u;
    const bool two = total > 55u;
    uint32_t b0[16], b1[16];
#pragma unroll
    for (int j = 0; j < 16; j++) { b0[j] = m[j]; b1[j] = m[16 + j]; }
    if (!two) b0[15] = bits;
    b1[15] = bits;
    sha256_iv(out);
    sha256_compress(out, b0);
    if (two) sha256_compress(out, b1);
}

/* The file is compiled four times (Makefile): the Office kernels (DPRF_PART_OFFICE), the ODF kernels
 * (DPRF_PART_ODT) and the PDF R2-R5 kernels (DPRF_PART_PDF), each object with the LLVM machine-scheduler
 * strategy that measured fastest for it AND leaves its kernels without scratch (resource_gate.py), and the long-list
 * prehash (DPRF_PART_LONG).  A fifth time for the 40-bit key search of PDF R2-R4 (DPRF_PART_KEY40, never part of the
 * default set): the verdict stage of k_pdf_r24 below and k_key40_pdf at the end of the PDF kernels, in an object of
 * its own, so that the four above keep their machine code.  A sixth time for the password search against a known
 * 40-bit key (DPRF_PART_COLLIDE, likewise): the key derivation of k_pdf_r24's key wave and k_collide_pdf at the end. */
#if !defined(DPRF_PART_OFFICE) && !defined(DPRF_PART_ODT) && !defined(DPRF_PART_PDF) && !defined(DPRF_PART_LONG) && \
    !defined(DPRF_PART_KEY40) && !defined(DPRF_PART_COLLIDE)
#define DPRF_PART_OFFICE
#define DPRF_PART_ODT
#define DPRF_PART_PDF
#define DPRF_PART_LONG
#endif

#ifdef DPRF_PART_LONG
/* ================================================================== long candidates (round 4) */
/* Candidates longer than the 64-byte list slot: the reference hashes any strlen(password) -- ODF's start key
 * (odt...c:78-79), Office's H0 over salt || UTF-16LE (msoffcrypto...c:94-101, iconv of any length :275-336), PDF R5
 * after truncation at 127 (pdf...c:197-206) and R6's K0 over the whole password (:240-245, <= 176 bytes, :228).  This
 * kernel computes that first message's hash for one record per lane, streaming the record from the blob in 64-byte
 * blocks (a lane loops over its own block count; records are rare, so the divergence costs nothing that matters);
 * the format's usual kernels then run from the hash in `keys` (Office / ODF KDF, R6), or it compares directly (R5).
 * Records sit 16-byte aligned in the blob, zero past their length; message words are built with static indices only. */
DEVI uint32_t long_msg_word(const uint32_t *rec, uint32_t len, uint32_t dw, const uint32_t sw[3], uint32_t ns) {
    /* LE word dw of record || suffix bytes || 0x80: the suffix words sw[0..ns) (ns - 1 suffix words + the 0x80 word)
     * land at byte offset len */
    uint32_t v = 4u * dw < len ? rec[dw] & le_keep_mask(0, len - 4u * dw) : 0u;
    const uint32_t q = len >> 2, r = (len & 3u) * 8u;
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
        if (k >= ns) break;
        if (dw == q + k) v |= sw[k] << r;
        if (r && dw == q + k + 1u) v |= sw[k] >> (32u - r);
    }
    return v;
}
__global__ void __launch_bounds__(256)
k_long_prehash(dprf_enum e, dprf_long_params lp, dprf_results *R, uint32_t cap, uint32_t stop_on_first) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.count) return;
    const uint64_t rec = e.start + g;
    const uint32_t *d = e.slots + e.loff[rec];
    const uint32_t len = e.llen[rec];
    const bool sha1 = lp.alg == DPRF_LONG_SHA1_SALT16;
    const uint32_t prew = sha1 ? 4u : 0u;                                /* message words before the record */
    const bool salt = lp.alg == DPRF_LONG_SHA256_SALT8 || lp.alg == DPRF_LONG_R5;
    const uint32_t sw[3] = {salt ? lp.suffix[0] : 0x80u, salt ? lp.suffix[1] : 0u, 0x80u};
    const uint32_t ns = salt ? 3u : 1u;
    const uint32_t total = 4u * prew + len + (salt ? 8u : 0u);           /* message bytes */
    const uint32_t nb = (total + 9u + 63u) >> 6;                        /* blocks incl. 0x80 and the bit length */
    uint32_t h[8];
    if (sha1) { sha1_iv(h); h[5] = h[6] = h[7] = 0u; }
    else sha256_iv(h);
    for (uint32_t b = 0; b < nb; b++) {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t t = 16u * b + (uint32_t)j;
            w[j] = t < prew ? lp.prefix[j & 3] : bswap32(long_msg_word(d, len, t - prew, sw, ns));
        }
        if (b + 1u == nb) { w[14] = 0u; w[15] = total * 8u; }
        if (sha1) sha1_compress(h, w);
        else sha256_compress(h, w);
    }
    if (lp.alg == DPRF_LONG_R5) {
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 8; k++) ok = ok && h[k] == lp.target[k];
        if (ok) report_hit(e, R, rec, cap, stop_on_first);
        return;
    }
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (k < 5 || !sha1) e.keys[(size_t)k * e.count + g] = h[k];
}

#endif /* DPRF_PART_LONG */

#ifdef DPRF_PART_OFFICE
/* ================================================================== Office (ECMA-376 Standard) */
/* Two launches per batch.  k_office_kdf runs the 50,002 dependent SHA-1s at 8 waves/SIMD (<= 64 VGPRs)
 * and leaves the AES-128 key X1[0:16] of every candidate in HBM ([word][candidate], coalesced);
 * k_office_check does the AES-128 verifier check with its own register budget.  The hand-off costs
 * 32 bytes per candidate against ~3e7 issue slots of hashing. */
template <int MODE>
__global__ void __launch_bounds__(256, 8)
k_office_kdf(dprf_enum e, dprf_office_params p, dprf_results *R, uint32_t stop_on_first, uint32_t *keys) {
    __shared__ uint8_t cs[256];
    __shared__ uint32_t flag;
    if (!block_prologue<false, false>(e, nullptr, R, stop_on_first, cs, nullptr, &flag)) return;
    const uint32_t g0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (g0 >= e.count) return;
    const uint32_t g = g0;
    uint32_t h[5];
    if constexpr (MODE == 2) {
        /* long list: H0 from k_long_prehash (same place this kernel leaves X1: the lane's own column) */
#pragma unroll
        for (int k = 0; k < 5; k++) h[k] = keys[(size_t)k * e.count + g];
    } else {
        cand c;
        get_candidate<MODE, true, LIST_CLAMP>(e, cs, g, c);
        /* H0 = SHA1(salt[0:16] || UTF16LE(pw)) (msoffcrypto...c:94-101) */
        uint32_t m[32];
        m[0] = p.salt[0]; m[1] = p.salt[1]; m[2] = p.salt[2]; m[3] = p.salt[3];
        be_append<4>(m, c);
        sha1_msg2(m, 16u + c.len, h);
    }

    /* 50,000 x H = SHA1(LE32(i) || H) (:105-113): W0 = bswap(i) is wave-uniform */
    for (uint32_t i = 0; i < 50000u; i++) {
        uint32_t w[16] = {bswap32(i), h[0], h[1], h[2], h[3], h[4], 0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 192u};
        uint32_t s[5];
        sha1_iv(s);
        sha1_compress(s, w);
        h[0] = s[0]; h[1] = s[1]; h[2] = s[2]; h[3] = s[3]; h[4] = s[4];
    }
    /* H = SHA1(H || 00000000) (:115-118) */
    {
        uint32_t w[16] = {h[0], h[1], h[2], h[3], h[4], 0u, 0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 192u};
        sha1_iv(h);
        sha1_compress(h, w);
    }
    /* X1 = SHA1((0x36 x 64) ^ H), key = X1[0:16] (:128-153) */
    uint32_t x1[5];
    {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = 0x36363636u ^ (j < 5 ? h[j] : 0u);
        sha1_iv(x1);
        sha1_compress(x1, w);
        uint32_t w2[16] = {0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 512u};
        sha1_compress(x1, w2);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) keys[(size_t)k * e.count + g] = x1[k];
}

__global__ void __launch_bounds__(256)
k_office_check(dprf_enum e, dprf_office_params p, const dprf_aes_tables *T, dprf_results *R, uint32_t cap,
               uint32_t stop_on_first, const uint32_t *keys) {
    __shared__ uint8_t cs[256];
    __shared__ aes_lds L;
    __shared__ uint32_t flag;
    if (!block_prologue<true>(e, T, R, stop_on_first, cs, &L, &flag)) return;
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = g < e.count;
    uint32_t key[4];
#pragma unroll
    for (int k = 0; k < 4; k++) key[k] = valid ? keys[(size_t)k * e.count + g] : 0u;
    /* AES-128-ECB decrypt of verifier and verifier hash, always AES-128 (:159-172, :207) */
    uint32_t rk[44], dk[44];
    aes128_expand(L, key, rk);
    aes_dec_schedule<10>(L, rk, dk);
    uint32_t dv[4], dh0[4], dh1[4];
    aes_decrypt<10>(L, dk, p.ev, dv);
    aes_decrypt<10>(L, dk, p.evh, dh0);
    aes_decrypt<10>(L, dk, p.evh + 4, dh1);
    /* decryptedVerifierHash[hash_size] == 0 (:168), hash_size uniform in [0,32) */
    const uint32_t hs = p.hash_size;
    const uint32_t wi = (hs & 15u) >> 2, sh = 24u - 8u * (hs & 3u);
    uint32_t word;
    if (hs < 16u) word = wi == 0 ? dh0[0] : wi == 1 ? dh0[1] : wi == 2 ? dh0[2] : dh0[3];
    else word = wi == 0 ? dh1[0] : wi == 1 ? dh1[1] : wi == 2 ? dh1[2] : dh1[3];
    bool ok = ((word >> sh) & 0xffu) == 0u;
    /* SHA1(verifier) == dec_evh[0:20] (:175-188) */
    uint32_t vh[5];
    {
        uint32_t w[16] = {dv[0], dv[1], dv[2], dv[3], 0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 128u};
        sha1_iv(vh);
        sha1_compress(vh, w);
    }
    ok = ok && vh[0] == dh0[0] && vh[1] == dh0[1] && vh[2] == dh0[2] && vh[3] == dh0[3] && vh[4] == dh1[0];
    if (valid && ok) report_hit(e, R, e.start + g, cap, stop_on_first);
}

#endif /* DPRF_PART_OFFICE */

#ifdef DPRF_PART_ODT
/* ================================================================== ODF 1.2 (AES-256-CBC, PBKDF2-HMAC-SHA1) */
/* Two launches per batch, as for Office: k_odt_kdf (SHA-256 start key + PBKDF2, ODT_KDF_WAVES per SIMD) leaves the
 * 32-byte AES-256 key of every candidate in HBM; k_odt_check decrypts and verifies. */
/* Waves per SIMD of k_odt_kdf.  The long-reach schedule forms of sha1_compress_pre (dev_crypto.h) keep W[0..4],
 * W[16..22] and W[32..46] live next to the last 16 words: 96 VGPRs, 5 waves (at 6: 80 VGPRs and 40 B/lane of scratch,
 * which the resource gate refuses).  Occupancy itself does not move this kernel: the same code bounded to 4 waves
 * measures the same, and the standard schedule measured the same at 8 / 6 / 4 (round 2); with the squared form
 * alone (SHA1_H20_FORMS=2) 6 and 7 waves are equal too (profiles/ab_sha1_sched.txt). */
#ifndef ODT_KDF_WAVES
#define ODT_KDF_WAVES 5
#endif
template <int MODE>
__global__ void __launch_bounds__(256, ODT_KDF_WAVES)
k_odt_kdf(dprf_enum e, dprf_odt_params p, dprf_results *R, uint32_t stop_on_first, uint32_t *keys) {
    __shared__ uint8_t cs[256];
    __shared__ uint32_t flag;
    if (!block_prologue<false, false>(e, nullptr, R, stop_on_first, cs, nullptr, &flag)) return;
    const uint32_t g0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (g0 >= e.count) return;
    const uint32_t g = g0;
    /* start key = SHA256(password) (odt...c:78-79) */
    uint32_t sk[8];
    if constexpr (MODE == 2) {
        /* long list: from k_long_prehash, in the lane's own key column */
#pragma unroll
        for (int k = 0; k < 8; k++) sk[k] = keys[(size_t)k * e.count + g];
    } else {
        cand c;
        get_candidate<MODE, false, LIST_CLAMP>(e, cs, g, c);
        uint32_t m[32];
        be_append<0>(m, c);
        sha256_msg2(m, c.len, sk);
    }
    /* the key column for the stores; long list: hidden from LLVM, which otherwise keeps the loads' eight addresses
     * live through PBKDF2 for the stores (16 VGPRs the loops need) */
    uint32_t gk = g;
    if constexpr (MODE == 2) asm volatile("" : "+v"(gk));
    /* PBKDF2-HMAC-SHA1(sk, salt, 1024, 32) (:85): ipad/opad midstates once per candidate */
    uint32_t ist[5], ost[5];
    {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = 0x36363636u ^ (j < 8 ? sk[j] : 0u);
        sha1_iv(ist); sha1_compress(ist, w);
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = 0x5c5c5c5cu ^ (j < 8 ? sk[j] : 0u);
        sha1_iv(ost); sha1_compress(ost, w);
    }
    /* the midstates' message-independent parts of rounds 0-4, once per candidate (dev_crypto.h sha1_pre) */
    const sha1_pre_t ipre = sha1_pre(ist), opre = sha1_pre(ost);
#pragma unroll
    for (int blkno = 1; blkno <= 2; blkno++) {
        uint32_t u[5], t[5];
        {
            /* both messages are 20 bytes: salt | INT(blkno), then the inner digest (dev_crypto.h sha1_compress_pre) */
            const uint32_t m[5] = {p.salt[0], p.salt[1], p.salt[2], p.salt[3], (uint32_t)blkno};
            uint32_t s[5];
            sha1_compress_pre(ist, ipre, m, s);
            sha1_compress_pre(ost, opre, s, u);
        }
        t[0] = u[0]; t[1] = u[1]; t[2] = u[2]; t[3] = u[3]; t[4] = u[4];
        for (int it = 1; it < 1024; it++) {
            uint32_t s[5];
            sha1_compress_pre(ist, ipre, u, s);
            sha1_compress_pre(ost, opre, s, u);
            /* two-input ops of the loop in 8-byte encodings (dev_crypto.h xor2_e64) */
            t[0] = xor2_e64(t[0], u[0]); t[1] = xor2_e64(t[1], u[1]); t[2] = xor2_e64(t[2], u[2]);
            t[3] = xor2_e64(t[3], u[3]); t[4] = xor2_e64(t[4], u[4]);
        }
        /* each block's key words go out as soon as they are known (block 1's five need not stay live through
         * block 2) */
        if (blkno == 1) {
#pragma unroll
            for (int k = 0; k < 5; k++) keys[(size_t)k * e.count + gk] = t[k];
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) keys[(size_t)(5 + k) * e.count + gk] = t[k];
        }
    }
}

/* The 64 AES-256 block decryptions per candidate read Td0 14,336 times.  A single 1 KiB Td0 puts
 * random indices of 32 lanes on 32 banks (~3.5-way conflicts: 65 % of this kernel's cycles were bank
 * conflicts, profiles/prof_odt_r01.json).  The tables follow R6's split-table scheme (dprf_kernels_r6.hip
 * aes128_encrypt_split; the replicated single table of rounds 1-2, 12 v_alignbit per round, is in HISTORY.md) for
 * the inverse cipher: four tables Td_t = ror(Td0, 8t) x 16 copies fill the 256-byte rows, lane group A (bit 4 of the lane clear) reads
 * Td_t and group B Td_t+1 in every lookup (32 different banks per 32-lane half), B keeps its state rotated -- after
 * inner round r its register j holds ror(s_(j + rho_r), 8 eps_r) with (rho, eps) -> (rho - eps, eps + 1) for the
 * inverse cipher's column order -- and its round keys are permuted to match; no rotates are left.  Si sits in one
 * more row (address 0x10000 + x, one v_perm; the last round's 16 byte reads share its banks).
 * tests/test_odt_split_model.py restates it against FIPS-197. */
#define ODT_TD_ROW 256
__shared__ __attribute__((aligned(16))) uint32_t odt_td[(256 + 1) * ODT_TD_ROW / 4];

/* B's representation (rho, eps) after inner round r = 0..13 of the inverse cipher */
__device__ constexpr int ODT_RHO[14] = {0, 0, 3, 1, 2, 2, 1, 3, 0, 0, 3, 1, 2, 2};
__device__ constexpr int ODT_EPS[14] = {0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1};
#define ODT_SEL(t) (0x0c0c0000u | ((4u + 3u - (t)) << 8) | (t))
/* One inner round: 16 lookups issued column by column (column j: s_j, s_j-1, s_j-2, s_j-3 for lookups t = 0..3),
 * then each column's two v_bitop3 behind the wait covering its reads (as r6_round_asm). */
DEVI void odt_round_asm(uint32_t &s0, uint32_t &s1, uint32_t &s2, uint32_t &s3, uint32_t base, uint32_t k0,
                        uint32_t k1, uint32_t k2, uint32_t k3) {
    uint32_t t[16];
#define ODL(d, s, sel) "v_perm_b32 %" #d ", %" #s ", %20, %" #sel "\n\tds_read_b32 %" #d ", %" #d "\n\t"
    asm volatile(
        ODL(4, 0, 25) ODL(5, 3, 26) ODL(6, 2, 27) ODL(7, 1, 28)
        ODL(8, 1, 25) ODL(9, 0, 26) ODL(10, 3, 27) ODL(11, 2, 28)
        ODL(12, 2, 25) ODL(13, 1, 26) ODL(14, 0, 27) ODL(15, 3, 28)
        ODL(16, 3, 25) ODL(17, 2, 26) ODL(18, 1, 27) ODL(19, 0, 28)
        "s_waitcnt lgkmcnt(12)\n\t"
        "v_bitop3_b32 %4, %4, %5, %6 bitop3:0x96\n\t"
        "v_bitop3_b32 %0, %4, %7, %21 bitop3:0x96\n\t"
        "s_waitcnt lgkmcnt(8)\n\t"
        "v_bitop3_b32 %8, %8, %9, %10 bitop3:0x96\n\t"
        "v_bitop3_b32 %1, %8, %11, %22 bitop3:0x96\n\t"
        "s_waitcnt lgkmcnt(4)\n\t"
        "v_bitop3_b32 %12, %12, %13, %14 bitop3:0x96\n\t"
        "v_bitop3_b32 %2, %12, %15, %23 bitop3:0x96\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_bitop3_b32 %16, %16, %17, %18 bitop3:0x96\n\t"
        "v_bitop3_b32 %3, %16, %19, %24 bitop3:0x96"
        : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3), "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3]), "=&v"(t[4]),
          "=&v"(t[5]), "=&v"(t[6]), "=&v"(t[7]), "=&v"(t[8]), "=&v"(t[9]), "=&v"(t[10]), "=&v"(t[11]),
          "=&v"(t[12]), "=&v"(t[13]), "=&v"(t[14]), "=&v"(t[15])
        : "v"(base), "v"(k0), "v"(k1), "v"(k2), "v"(k3), "s"(ODT_SEL(0)), "s"(ODT_SEL(1)), "s"(ODT_SEL(2)),
          "s"(ODT_SEL(3))
        : "memory");
#undef ODL
}
/* Si[byte K of v] from the row after the tables (address 0x10000 + x) */
template <int K>
DEVI uint32_t odt_si(uint32_t v) {
    const uint32_t a = __builtin_amdgcn_perm(v, 0x00010000u, 0x0c020000u | (4u + K));
    return ((const uint8_t *)odt_td)[a];
}
/* Group B's round keys in its representation (A: unchanged) -- once per key schedule */
DEVI void odt_dk_split(uint32_t dk[60], uint32_t base) {
    const bool gb = (base & 0x40u) != 0u;
    const uint32_t sk[4] = {gb ? 0x03020100u : 0x07060504u, gb ? 0x00030201u : 0x07060504u,
                            gb ? 0x01000302u : 0x07060504u, gb ? 0x02010003u : 0x07060504u};
#pragma unroll
    for (int r = 1; r <= 14; r++) {
        const int rho = r < 14 ? ODT_RHO[r] : ODT_RHO[13] - ODT_EPS[13], eps = r < 14 ? ODT_EPS[r] : ODT_EPS[13];
        if (rho == 0 && eps == 0) continue;
        const uint32_t kk[4] = {dk[4 * r], dk[4 * r + 1], dk[4 * r + 2], dk[4 * r + 3]};
#pragma unroll
        for (int j = 0; j < 4; j++) dk[4 * r + j] = perm(kk[j], kk[(j + rho) & 3], sk[eps]);
    }
}
DEVI void aes256_decrypt_split(const uint32_t *dk, const uint32_t in[4], uint32_t out[4], uint32_t base) {
    uint32_t s[4] = {in[0] ^ dk[0], in[1] ^ dk[1], in[2] ^ dk[2], in[3] ^ dk[3]};
#pragma unroll
    for (int r = 1; r < 14; r++) odt_round_asm(s[0], s[1], s[2], s[3], base, dk[4 * r], dk[4 * r + 1], dk[4 * r + 2], dk[4 * r + 3]);
    /* last round: byte p of word j <- Si[byte p of s_(j-3+p)]; B's word j then holds ror(out[j + 1], 8) */
    uint32_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
        acc[j] = ((odt_si<3>(s[j]) << 24) | (odt_si<2>(s[(j + 3) & 3]) << 16) | (odt_si<1>(s[(j + 2) & 3]) << 8) |
                  odt_si<0>(s[(j + 1) & 3])) ^ dk[56 + j];
    const uint32_t selr = (base & 0x40u) ? 0x02010003u : 0x07060504u;
#pragma unroll
    for (int j = 0; j < 4; j++) out[j] = perm(acc[j], acc[(j + 3) & 3], selr);
}

#define ODT_CHECK_THREADS 512
__global__ void __launch_bounds__(ODT_CHECK_THREADS, 4)   /* 2 workgroups (64 KiB table each) per CU */
k_odt_check(dprf_enum e, dprf_odt_params p, const dprf_aes_tables *T, dprf_results *R, uint32_t cap,
            uint32_t stop_on_first, const uint32_t *keys) {
    __shared__ uint8_t cs[256];
    __shared__ aes_lds L;
    __shared__ uint32_t flag;
    for (uint32_t k = threadIdx.x; k < 256u * ODT_TD_ROW / 4; k += blockDim.x) {
        const uint32_t x = k >> 6, c = k & 63u;
        odt_td[k] = ror32(T->td0[x], 8u * (c >> 4));                             /* Td_(c/16), copy c % 16 */
    }
    if (threadIdx.x < 64u) {
        const uint32_t x = 4u * threadIdx.x;                                     /* the Si row at 0x10000 */
        odt_td[256u * ODT_TD_ROW / 4 + threadIdx.x] = (uint32_t)T->inv_sbox[x] | ((uint32_t)T->inv_sbox[x + 1] << 8) |
                                                     ((uint32_t)T->inv_sbox[x + 2] << 16) | ((uint32_t)T->inv_sbox[x + 3] << 24);
    }
    if (!block_prologue<true>(e, T, R, stop_on_first, cs, &L, &flag)) return;
    /* odt_round_asm uses the v_perm result as the whole LDS address: the table must sit at LDS address 0 (checked;
     * a build that ever breaks this fails loudly instead of computing wrong) */
    if ((uint32_t)(size_t)(__attribute__((address_space(3))) uint8_t *)odt_td != 0u) {
        if (threadIdx.x == 0) atomicOr(&R->pad_, 4u);
        return;
    }
    const uint32_t lanec = (threadIdx.x & 15u) << 2;
    /* split tables: byte t = row offset of the copy lookup t reads (A: Td_t, B: Td_t+1) */
    const uint32_t base = lanec * 0x01010101u + ((threadIdx.x & 16u) ? 0x00c08040u : 0xc0804000u);
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = g < e.count;
    uint32_t key[8];
#pragma unroll
    for (int k = 0; k < 8; k++) key[k] = valid ? keys[(size_t)k * e.count + g] : 0u;
    /* AES-256-CBC decrypt, no padding (:90-92) */
    uint32_t rk[60], dk[60];
    aes256_expand(L, key, rk);
    aes_dec_schedule<14>(L, rk, dk);
    odt_dk_split(dk, base);
#define ODT_DECRYPT(dk, ct, pt) aes256_decrypt_split(dk, ct, pt, base)
    bool ok;
    if (p.enc_len == 16u) {
        /* experimental 2-byte check (:98-101) */
        uint32_t ct[4] = {p.enc[0], p.enc[1], p.enc[2], p.enc[3]}, pt[4];
        ODT_DECRYPT(dk, ct, pt);
        ok = ((pt[0] ^ p.iv[0]) >> 16) == 0x0300u;
    } else {
        /* SHA256 over the first min(len,1024) plaintext bytes == checksum (:104-123) */
        uint32_t st[8];
        sha256_iv(st);
        uint32_t prev[4] = {p.iv[0], p.iv[1], p.iv[2], p.iv[3]};
        const uint32_t n = p.hash_len, nfull = n >> 6, rem = n & 63u;
        for (uint32_t b = 0; b < nfull; b++) {
            uint32_t w[16];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t *cp = p.enc + (b * 4u + q) * 4u;
                uint32_t ct[4] = {cp[0], cp[1], cp[2], cp[3]}, pt[4];
                ODT_DECRYPT(dk, ct, pt);
#pragma unroll
                for (int k = 0; k < 4; k++) { w[4 * q + k] = pt[k] ^ prev[k]; prev[k] = ct[k]; }
            }
            sha256_compress(st, w);
        }
        /* final block: rem (0/16/32/48) data bytes, 0x80, bit length */
        uint32_t w[16];
#pragma unroll
        for (int q = 0; q < 3; q++) {
            if ((uint32_t)q < (rem >> 4)) {
                const uint32_t *cp = p.enc + (nfull * 4u + q) * 4u;
                uint32_t ct[4] = {cp[0], cp[1], cp[2], cp[3]}, pt[4];
                ODT_DECRYPT(dk, ct, pt);
#pragma unroll
                for (int k = 0; k < 4; k++) { w[4 * q + k] = pt[k] ^ prev[k]; prev[k] = ct[k]; }
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) w[4 * q + k] = 0u;
            }
        }
#pragma unroll
        for (int k = 12; k < 16; k++) w[k] = 0u;
#pragma unroll
        for (int k = 0; k < 16; k++) if ((uint32_t)k == (rem >> 2)) w[k] = 0x80000000u;
        w[15] = n * 8u;
        sha256_compress(st, w);
        ok = true;
#pragma unroll
        for (int k = 0; k < 8; k++) ok = ok && st[k] == p.checksum[k];
    }
    if (valid && ok) report_hit(e, R, e.start + g, cap, stop_on_first);
#undef ODT_DECRYPT
}
#endif /* DPRF_PART_ODT */

#ifdef DPRF_PART_PDF
/* ================================================================== PDF R5 (one SHA-256) */
/* One SHA-256 per candidate is ~2,300 cycles of a wave: with one candidate per thread, wave launch and
 * the block prologue were a third of the kernel (2 Mi waves per 128 Mi-candidate launch).  Each thread
 * takes PER candidates: a run of PER consecutive indices in range mode when the charset has at least PER
 * characters (PER 16, or 8 for 8-15 characters: one wrap of the last digit per run at most), else -- and in
 * list mode -- PER candidates 256 apart. */
/* 1: range-mode threads take runs of consecutive candidates (below); 0: PER candidates 256 apart (A/B) */
#ifndef R5_RUNS
#define R5_RUNS 1
#endif
#ifndef R5_PER_MAX
#define R5_PER_MAX 16
#endif
/* SHA-256 of one block from the IV, compared with u[0:8], with an early exit: the last word of the digest
 * is IV7 + (e after round 60) -- that e only moves down to h in rounds 61-63 -- so a wave none of whose
 * lanes matches u[7] there (all but a 2^-32 fraction) skips rounds 61-63 and their schedule words. */
DEVI bool sha256_block_matches(uint32_t w[16], const uint32_t u[8], bool valid) {
    uint32_t a = 0x6a09e667u, b = 0xbb67ae85u, c = 0x3c6ef372u, d = 0xa54ff53au;
    uint32_t e = 0x510e527fu, f = 0x9b05688cu, g = 0x1f83d9abu, h = 0x5be0cd19u;
#pragma unroll
    for (int t = 0; t < 64; t++) {
        if (t == 61 && !__builtin_amdgcn_ballot_w64(valid && e + 0x5be0cd19u == u[7])) return false;
        uint32_t wt;
        if (t < 16) {
            wt = w[t];
        } else {
            wt = w[t & 15] + s0_256(w[(t - 15) & 15]) + w[(t - 7) & 15] + s1_256(w[(t - 2) & 15]);
            w[t & 15] = wt;
        }
        const uint32_t t1 = h + S1_256(e) + f_ch(e, f, g) + (k256(t) + wt);
        const uint32_t t2 = S0_256(a) + f_maj(a, b, c);
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    return valid && a + 0x6a09e667u == u[0] && b + 0xbb67ae85u == u[1] && c + 0x3c6ef372u == u[2] &&
           d + 0xa54ff53au == u[3] && e + 0x510e527fu == u[4] && f + 0x9b05688cu == u[5] &&
           g + 0x1f83d9abu == u[6] && h + 0x5be0cd19u == u[7];
}
/* NW (range mode): message words 0..NW-1 carry candidate bytes (NW = ceil(pwlen / 4), one instantiation per launch
 * length); the words after them are the launch-uniform tail alone, so the compiler keeps them, K + W of their rounds
 * and the schedule terms built only from them in SGPRs (the scalar unit) instead of spending VALU slots on them */
/* minimum waves per SIMD the register allocation must allow.  Measured (round 5, profiles/ab_r5_runs_r05q.txt,
 * -pr 7 alnum, three alternating rounds): no bound (132 VGPRs, 3 waves) 32.0 G with runs of 8; 4 waves 32.86 G,
 * 5 waves 32.95 G with runs of 16 */
#ifndef R5_WAVES
#define R5_WAVES 5
#endif
template <int MODE, int NW, int PER>
__global__ void __launch_bounds__(256, R5_WAVES)
k_pdf_r5(dprf_enum e, dprf_pdf_params p, dprf_results *R, uint32_t cap, uint32_t stop_on_first) {
    static_assert(NW >= 1 && NW <= DPRF_MAX_RANGE_LEN / 4, "candidate words");
    static_assert(PER == 8 || PER == 16, "run length");
    __shared__ uint8_t cs[256];
    __shared__ uint32_t flag;
    if (!block_prologue<false>(e, nullptr, R, stop_on_first, cs, nullptr, &flag, PER)) return;
    const uint32_t base = blockIdx.x * (blockDim.x * PER);
    /* Range mode: every candidate has length pwlen <= DPRF_MAX_RANGE_LEN, so the message is one block and
     * its tail -- salt8 || 0x80 at byte pwlen, the bit length in word 15 -- is the same for the whole
     * launch: 16 uniform BE words built once (SGPRs), OR-ed onto the candidate's BE words. */
    uint32_t tail[16];
    if (MODE == 0) {
        const uint32_t len = e.pwlen, q = len >> 2, r = (len & 3u) * 8u;
        const uint32_t sw[3] = {p.u[8], p.u[9], 0x80u};
#pragma unroll
        for (int j = 0; j < 16; j++) tail[j] = 0u;
#pragma unroll
        for (int s = 0; s < 3; s++) {
            const uint32_t lo = r ? (sw[s] << r) : sw[s];
            const uint32_t hi = r ? (sw[s] >> (32u - r)) : 0u;
#pragma unroll
            for (int j = 0; j < 15; j++) {
                if ((uint32_t)j == q + s) tail[j] |= lo;
                if ((uint32_t)j == q + s + 1) tail[j] |= hi;
            }
        }
#pragma unroll
        for (int j = 0; j < 15; j++) tail[j] = bswap32(tail[j]);
        tail[15] = (len + 8u) * 8u;
    }
    if (MODE == 0 && R5_RUNS && e.cslen >= PER) {
        /* Runs (round 5): thread t takes the PER consecutive indices base + PER t + k, which differ only in the last
         * character except across one wrap of the last digit (cslen >= PER).  The candidate is spelled twice
         * per run -- at its first index (last digit d0) and at the first index past the wrap (last digit 0, prefix + 1)
         * -- as BE message words with the tail already OR-ed in and the last character cleared; each candidate then
         * costs a select per word and one charset byte instead of a full mixed-radix spelling. */
        const uint32_t g0 = base + threadIdx.x * PER;
        const uint32_t gc = g0 < e.count ? g0 : e.count - 1u;
        const uint32_t lp = e.pwlen - 1u;                             /* position of the last character */
        const uint32_t lw = lp >> 2, lsh = 24u - 8u * (lp & 3u);      /* its BE word and bit offset */
        const uint32_t q0 = e.cslen == 1 ? gc : fastdiv(gc, e.div_m, e.div_s);
        uint32_t d0 = (uint32_t)e.sdig[lp] + (gc - q0 * e.cslen);
        d0 -= d0 >= e.cslen ? e.cslen : 0u;
        uint32_t w0[NW], w1[NW];
        {
            cand c;
            range_candidate<false>(e, cs, gc, c);
#pragma unroll
            for (int j = 0; j < NW; j++) w0[j] = bswap32(c.w[j]) | tail[j];
            range_candidate<false>(e, cs, gc + (e.cslen - d0), c);
#pragma unroll
            for (int j = 0; j < NW; j++) w1[j] = bswap32(c.w[j]) | tail[j];
#pragma unroll
            for (int j = 0; j < NW; j++) {
                const uint32_t m = (uint32_t)j == lw ? ~(0xffu << lsh) : ~0u;
                w0[j] &= m; w1[j] &= m;
            }
        }
#pragma unroll 1
        for (uint32_t k = 0; k < (uint32_t)PER; k++) {
            if (base + k >= e.count) break;                             /* uniform: a wave's runs start >= base */
            const uint32_t g = g0 + k;
            const bool valid = g < e.count;
            const uint32_t d = d0 + k;
            const bool lo = d < e.cslen;
            const uint32_t ch = (uint32_t)cs[lo ? d : d - e.cslen] << lsh;
            uint32_t b[16];
#pragma unroll
            for (int j = 0; j < 16; j++) {
                b[j] = j < NW ? (lo ? w0[j] : w1[j]) : tail[j];
                if (j < NW && (uint32_t)j == lw) b[j] |= ch;
            }
            if (sha256_block_matches(b, p.u, valid)) report_hit(e, R, e.start + g, cap, stop_on_first);
        }
        return;
    }
#pragma unroll 1
    for (uint32_t k = 0; k < (uint32_t)PER; k++) {
        const uint32_t g0 = base + k * blockDim.x + threadIdx.x;
        if (base + k * blockDim.x >= e.count) break;                 /* uniform */
        const bool valid = g0 < e.count;
        const uint32_t g = valid ? g0 : e.count - 1;
        cand c;
        get_candidate<MODE, false, LIST_CLAMP>(e, cs, g, c);
        if (MODE == 0) {
            /* range_candidate leaves the bytes past pwlen zero */
            uint32_t b[16];
#pragma unroll
            for (int j = 0; j < 16; j++) b[j] = (j < NW ? bswap32(c.w[j]) : 0u) | tail[j];
            if (sha256_block_matches(b, p.u, valid)) report_hit(e, R, e.start + g, cap, stop_on_first);
            continue;
        }
        if (NW < 8) {
            /* a list launch whose candidates all have at most 4 NW <= 16 bytes (launch_pdf_r5 picks NW from the
             * launch's longest): one message block, words past NW + 2 zero, and the round-61 early exit */
            uint32_t b[16];
#pragma unroll
            for (int j = 0; j < 16; j++) b[j] = j < NW ? (c.w[j] & le_keep_mask(j, c.len)) : 0u;
            const uint32_t sw[3] = {p.u[8], p.u[9], 0x80u};
            const uint32_t q = c.len >> 2, r = (c.len & 3u) * 8u;
#pragma unroll
            for (int s = 0; s < 3; s++) {
                const uint32_t lo = r ? (sw[s] << r) : sw[s];
                const uint32_t hi = r ? (sw[s] >> (32u - r)) : 0u;
#pragma unroll
                for (int j = 0; j < NW + 3; j++) {
                    if ((uint32_t)j == q + s) b[j] |= lo;
                    if ((uint32_t)j == q + s + 1) b[j] |= hi;
                }
            }
#pragma unroll
            for (int j = 0; j < NW + 3; j++) b[j] = bswap32(b[j]);
            b[15] = (c.len + 8u) * 8u;
            if (sha256_block_matches(b, p.u, valid)) report_hit(e, R, e.start + g, cap, stop_on_first);
            continue;
        }
        /* SHA256(pw[:127] || U[32:40]) == U[0:32] (pdf...c:194-221); host caps len at 127 and slots at 64 */
        uint32_t m[32];
#pragma unroll
        for (int j = 0; j < 32; j++) m[j] = j < DPRF_SLOT_WORDS ? (c.w[j] & le_keep_mask(j, c.len)) : 0u;
        /* append the 8 validation-salt bytes (LE words p.u[8], p.u[9]) at byte offset len, then 0x80 */
        const uint32_t sw[3] = {p.u[8], p.u[9], 0x80u};
        const uint32_t q = c.len >> 2, r = (c.len & 3u) * 8u;
#pragma unroll
        for (int s = 0; s < 3; s++) {
            const uint32_t lo = r ? (sw[s] << r) : sw[s];
            const uint32_t hi = r ? (sw[s] >> (32u - r)) : 0u;
#pragma unroll
            for (int j = 0; j < 32; j++) {
                if ((uint32_t)j == q + s) m[j] |= lo;
                if ((uint32_t)j == q + s + 1) m[j] |= hi;
            }
        }
#pragma unroll
        for (int j = 0; j < 32; j++) m[j] = bswap32(m[j]);
        uint32_t hh[8];
        sha256_msg2(m, c.len + 8u, hh);
        bool ok = true;
#pragma unroll
        for (int kk = 0; kk < 8; kk++) ok = ok && hh[kk] == p.u[kk];
        if (valid && ok) report_hit(e, R, e.start + g, cap, stop_on_first);
    }
}

#endif /* DPRF_PART_PDF */
/* ================================================================== PDF R2..R4 (MD5 + RC4) */
/* RC4 S-box layout, KSA and PRGA: rc4_dev.h; the two-wave workgroup and its driver: rc4_wg.h */

/* The padded password, the user key and r24_key, the two in a row, are the collider's too (DPRF_PART_COLLIDE) */
#if defined(DPRF_PART_PDF) || defined(DPRF_PART_COLLIDE)
/* Range mode: pwlen <= 32 and a candidate's bytes past it are zero, so PAD at byte offset pwlen is launch-uniform:
 * eight words built once per key wave and OR-ed onto every candidate.  List mode reads PAD per lane: zeros here. */
template <int MODE>
DEVI void r24_padtail(const dprf_enum &e, const dprf_pdf_params &p, uint32_t padtail[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) padtail[j] = 0u;
    if (MODE == 0) {
        const uint32_t q = e.pwlen >> 2, r = (e.pwlen & 3u) * 8u;
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const uint32_t lo = r ? (p.pad[t] << r) : p.pad[t];
            const uint32_t hi = r ? (p.pad[t] >> (32u - r)) : 0u;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if ((uint32_t)j == q + t) padtail[j] |= lo;
                if ((uint32_t)j == q + t + 1) padtail[j] |= hi;
            }
        }
    }
}
/* The 32 padded password bytes of candidate g, pw[:32] || PAD[0:32-len] (pdf...c:136-137), LE words.  Reads the
 * charset and PAD || PAD from the LDS overlay. */
template <int MODE>
DEVI void r24_padded_pw(const dprf_enum &e, const uint8_t *cs, const uint32_t *padw, const uint32_t padtail[8],
                        uint32_t g, uint32_t pw[8]) {
    cand c;
    get_candidate<MODE, false, LIST_CLAMP>(e, cs, g, c);
    const uint32_t len = c.len > 32u ? 32u : c.len;
    if (MODE == 0) {
#pragma unroll
        for (int j = 0; j < 8; j++) pw[j] = c.w[j] | padtail[j];
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            uint32_t v = c.w[j] & le_keep_mask(j, len);
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint32_t k = 4u * j + b;
                if (k >= len) v |= (uint32_t)((const uint8_t *)padw)[k - len] << (8 * b);
            }
            pw[j] = v;
        }
    }
}
/* User key of the 32 padded password bytes x: MD5(x || O || LE32(P) || ID [|| FFFFFFFF]) (pdf...c:136-139, :352-402),
 * then 50 x MD5(h[0:n]) for R >= 3 (:150-155).  In an owner search x comes from the RC4 wave and may hold any byte. */
template <int R, int NK>
DEVI void r24_user_key(const dprf_pdf_params &p, const uint32_t x[8], uint32_t h[4]) {
    {
        uint32_t m[16];
#pragma unroll
        for (int j = 0; j < 8; j++) { m[j] = x[j]; m[8 + j] = p.tail[j]; }
        md5_iv(h);
        md5_compress(h, m);
        for (uint32_t b = 0; b < p.tail_blocks; b++) {
#pragma unroll
            for (int j = 0; j < 16; j++) m[j] = p.tail[8 + 16 * b + j];
            md5_compress(h, m);
        }
    }
    if (R >= 3) {
        for (int i = 0; i < 50; i++) {
            uint32_t m[16];
            if (NK == 16) {
                m[0] = h[0]; m[1] = h[1]; m[2] = h[2]; m[3] = h[3]; m[4] = 0x80u;
#pragma unroll
                for (int j = 5; j < 16; j++) m[j] = 0u;
                m[14] = 128u;
            } else {
                m[0] = h[0]; m[1] = (h[1] & 0xffu) | 0x8000u;
#pragma unroll
                for (int j = 2; j < 16; j++) m[j] = 0u;
                m[14] = 40u;
            }
            md5_iv(h);
            md5_compress(h, m);
        }
    }
}
/* RC4 key of candidate g in a user-password search */
template <int MODE, int R, int NK>
DEVI void r24_key(const dprf_enum &e, const dprf_pdf_params &p, const uint8_t *cs, const uint32_t *padw,
                  const uint32_t padtail[8], uint32_t g, uint32_t h[4]) {
    uint32_t pw[8];
    r24_padded_pw<MODE>(e, cs, padw, padtail, g, pw);
    r24_user_key<R, NK>(p, pw, h);
}
#endif /* DPRF_PART_PDF || DPRF_PART_COLLIDE */
#ifdef DPRF_PART_PDF

/* One workgroup = one RC4 wave + one key wave, over NBAT batches of 64 candidates (round 2; rc4_wg.h).
 *
 * The RC4 wave owns the workgroup's 16 KiB S-box area (one 256-byte box per lane) and only ever runs KSAs and
 * PRGAs; the key wave derives the RC4 keys (enumeration + MD5 of the padded password and document tail, and for
 * R3/R4 the 50 MD5 iterations) of batch b+1 while the RC4 wave runs batch b.  Keys are handed over through the
 * S-box area while it is free, between two barriers at each batch boundary; charset, PAD and the skip flag sit
 * in an area of their own (16,720 B per workgroup: still 9 per CU).  The RC4 wave raises its issue priority
 * (s_setprio 3), so the MD5s take only the VALU cycles the KSA chains leave free.
 * Why: when one wave did both (round 1 - mid round 2), a wave hashing its keys held its S-box without running
 * a KSA -- ~8 % of the CU's 9 KSA chains idle for R3/R4, ~15 % for R2.  Measured (tools/ab_libs.sh, MI355X):
 * R3/R4 fused 464 M, split without / with the priority 458 / 481 M; a key wave that hashes nothing (probe) 484 M,
 * so the MD5s are fully hidden; then the KSA group size re-tuned (rc4_ksa): R3/R4 513 M, R2 8.77 -> 9.79 G.
 * Batches per workgroup, R3/R4: 2 / 4 / 8 = 472 / 480 / 481 M (G = 4), 6 / 8 / 12 = 513 / 513 / 507 M (G = 2);
 * R2: 8 / 16 / 24 = 9.58 / 9.68 / 9.70 G.  Re-measured on the group-deferred KSA: R3/R4 6 / 8 / 12 batches
 * 559 / 560 / 557 M, priority 0 / 1 / 3 529 / 560 / 560 M; R2 8 / 16 / 24 batches 11.08 / 11.25 / 11.32 G,
 * priority 0 10.56 G.  Round 3 (asm KSA): 8 / 12 / 16 = 613 / 608 / 603 M; round 4, with consecutive launches on two
 * streams (the last partial generation of one launch overlaps the next): 8 / 12 / 16 = 626.2 / 628.5 / 625.2 M (three
 * alternating runs each, every run of 12 above the neighbouring 8), so 12.  R2 likewise: 16 / 24 / 36 / 48 = 12.23 /
 * 12.27 / 12.32 / 12.31 G, so 36 (profiles/ab_r2_batches_r04l.txt). */
#endif /* DPRF_PART_PDF */
/* The batch counts, the KSA and the verdict stage are the key search's too (DPRF_PART_KEY40) */
#if defined(DPRF_PART_PDF) || defined(DPRF_PART_KEY40)
#ifndef R34_BATCHES
#define R34_BATCHES 12
#endif
#ifndef R2_BATCHES
#define R2_BATCHES 36
#endif
#ifndef R24_PRIO
#define R24_PRIO 3
#endif
/* 1: the KSA as the generated asm block (rc4_dev.h rc4_ksa_asm); 0: the C++ rc4_ksa (A/B builds) */
#ifndef R24_KSA_ASM
#define R24_KSA_ASM 1
#endif
/* dprf_results.pad_ bit of these kernels' LDS-address assumption (dprf_params.h) */
#define R24_ERR_LDS 2u
template <int NK>
DEVI void r24_ksa(uint8_t *S, uint32_t sbase, uint32_t lane, const uint32_t k[4]) {
    if (R24_KSA_ASM) rc4_ksa_asm<NK>(sbase, sbase + (lane << 2), k);
    else rc4_ksa<NK>(S, lane << 2, k);
}
/* Whether the candidate with RC4 key h is a hit (`valid`: its index is inside the launch), by the RC4 wave of the user
 * kernel; stage C(b) of k_pdf_r24_owner is a hand copy of this body (below: why), so a fix here is due there too.
 * R2: RC4-40 over PAD, compare 32 bytes of U (:161-163, :184-189).  The first 4 keystream bytes decide for all but
 * 2^-32 of the lanes: a wave continues the same keystream (i = 5.., j carried) only when one of its lanes matches
 * U[0:4].
 * R3/R4: c = RC4(key, MD5(PAD||ID)); c = RC4(key ^ x, c) for x = 1..19 (:167-174), compare 16 bytes.  Early reject:
 * every pass first produces only 2 keystream bytes and the candidate survives iff c19[0:2] equals U[0:2]; a wave in
 * which some lane survives (2^-16 per lane) redoes its candidates with the full keystream and the reference's
 * complete 16-byte compare (:184-189). */
template <int R, int NK>
DEVI bool r24_check(uint8_t *S, uint32_t sbase, uint32_t lane, const dprf_pdf_params &p, const uint32_t h[4],
                    bool valid) {
    bool ok = false;
    if (R == 2) {
        uint32_t d[8];
#pragma unroll
        for (int j = 0; j < 8; j++) d[j] = p.pad[j];
        r24_ksa<5>(S, sbase, lane, h);
        uint32_t jj = 0;
        rc4_prga_span<1, 4>(S, lane << 2, d, jj);
        if (__builtin_amdgcn_ballot_w64(valid && d[0] == p.u[0])) {
            rc4_prga_span<5, 32>(S, lane << 2, d, jj);
            ok = true;
#pragma unroll
            for (int j = 0; j < 8; j++) ok = ok && d[j] == p.u[j];
        }
    } else
    for (uint32_t full = 0; full < 2u; full++) {
        uint32_t d[4] = {p.h2[0], p.h2[1], p.h2[2], p.h2[3]};
        /* the asm KSA's key registers, made once per candidate; pass x's key (key ^ x) by XORing x ^ (x - 1)
         * into their byte 0 (16 v_xor per pass, the same count as forming kx and extracting its bytes) */
        uint32_t kb[NK];
        rc4_kb_init<NK>(h, kb);
        for (uint32_t x = 0; x < 20u; x++) {
            if (R24_KSA_ASM) {
                const uint32_t dx = x ^ (x - 1u);
                if (x) {
#pragma unroll
                    for (int q = 0; q < NK; q++) kb[q] ^= dx;
                }
                rc4_ksa_asm_kb<NK>(sbase, sbase + (lane << 2), kb);
            } else {
                const uint32_t xx = x * 0x01010101u;
                uint32_t kx[4] = {h[0] ^ xx, h[1] ^ xx, h[2] ^ xx, h[3] ^ xx};
                rc4_ksa<NK>(S, lane << 2, kx);
            }
            if (full) rc4_prga<16>(S, lane << 2, d);
            else rc4_prga<2>(S, lane << 2, d);
        }
        if (full) {
            ok = d[0] == p.u[0] && d[1] == p.u[1] && d[2] == p.u[2] && d[3] == p.u[3];
        } else {
            const bool pre = ((d[0] ^ p.u[0]) & 0xffffu) == 0u;
            if (!__builtin_amdgcn_ballot_w64(valid && pre)) break;
        }
    }
    return valid && ok;
}

template <int R> struct r24_batches { static constexpr uint32_t v = R == 2 ? R2_BATCHES : R34_BATCHES; };
#endif /* DPRF_PART_PDF || DPRF_PART_KEY40 */
#ifdef DPRF_PART_PDF
/* The user kernel's LDS: the S-box area first (LDS address 0: rc4_wg_sbox_base), then the overlay the key wave reads
 * -- 16,720 B per workgroup */
struct r24_lds {
    uint8_t S[RC4_WAVE_BYTES];
    uint8_t cs[256];                                      /* charset */
    uint32_t padw[16];                                    /* PAD || PAD */
    uint32_t flag[4];                                     /* block_prologue's skip flag */
};
DEVI void r24_stage_pad(r24_lds &L, const dprf_pdf_params &p) {
    if (threadIdx.x < 8) { L.padw[threadIdx.x] = p.pad[threadIdx.x]; L.padw[threadIdx.x + 8] = p.pad[threadIdx.x]; }
}
template <int MODE, int R, int NK>
__global__ void __launch_bounds__(128, 5)   /* 18 waves per CU (9 workgroups): <= 102 VGPRs */
k_pdf_r24(dprf_enum e, dprf_pdf_params p, dprf_results *R_, uint32_t cap, uint32_t stop_on_first) {
    constexpr uint32_t NBAT = r24_batches<R>::v;
    __shared__ __attribute__((aligned(16))) r24_lds L;
    uint8_t *S = L.S;
    r24_stage_pad(L, p);
    /* per = candidates per thread of the 128-thread block: 64 * NBAT candidates */
    if (!block_prologue<false>(e, nullptr, R_, stop_on_first, L.cs, nullptr, L.flag, NBAT / 2)) return;
    uint32_t padtail[8];
    r24_padtail<MODE>(e, p, padtail);
    rc4_wg_run<NBAT, R24_PRIO>(
        e, S, R24_KSA_ASM, R_, R24_ERR_LDS,
        /* key wave: the RC4 key of candidate g */
        [&](uint32_t g, uint32_t h[4]) { r24_key<MODE, R, NK>(e, p, L.cs, L.padw, padtail, g, h); },
        /* RC4 wave: the verdict of batch b under the lane's key h */
        [&](const rc4_wg &w, uint32_t sbase, uint32_t b, const uint32_t h[4]) {
            const uint32_t g = w.base + 64u * b + rc4_wg_lane_id();
            if (r24_check<R, NK>(S, sbase, w.lane, p, h, g < e.count))
                report_hit(e, R_, e.start + g, cap, stop_on_first);
        });
}

/* ================================================================== PDF R2..R4, owner password */
/* ISO 32000-1 Algorithms 3 and 7 (include/dprf.h "owner password"): the owner key MD5((pw[:32] || PAD)[:32]) [50 more
 * MD5s over all 16 bytes] decrypts O into x, a padded user password, and x must pass the user check above as a
 * 32-byte candidate.  Two key derivations and two RC4 stages per candidate, on k_pdf_r24's workgroup shape.
 * The kernel writes the workgroup frame, the PAD tail and the check stage out instead of using rc4_wg.h, r24_padtail
 * and r24_check: built on them its 128-bit range instantiation measured 0.3 % below its rate in two sessions
 * (HISTORY.md); r24_padded_pw and r24_user_key are the shared ones. */

/* Owner key (Algorithm 3 steps a-d): one MD5 block over the 32 padded bytes, then for R >= 3 fifty MD5s over the whole
 * 16-byte digest, whatever the key length (the user key's rounds hash h[0:n]) */
template <int R>
DEVI void r24_owner_key(const uint32_t pw[8], uint32_t h[4]) {
    {
        uint32_t m[16];
#pragma unroll
        for (int j = 0; j < 8; j++) { m[j] = pw[j]; m[8 + j] = 0u; }
        m[8] = 0x80u;
        m[14] = 256u;
        md5_iv(h);
        md5_compress(h, m);
    }
    if (R >= 3) {
        for (int i = 0; i < 50; i++) {
            uint32_t m[16];
            m[0] = h[0]; m[1] = h[1]; m[2] = h[2]; m[3] = h[3]; m[4] = 0x80u;
#pragma unroll
            for (int j = 5; j < 16; j++) m[j] = 0u;
            m[14] = 128u;
            md5_iv(h);
            md5_compress(h, m);
        }
    }
}
/* One workgroup = one RC4 wave + one key wave over NBAT batches of 64 candidates, as k_pdf_r24; per batch b
 *   O(b)  key wave: owner key of the batch's candidates
 *   D(b)  RC4 wave: x = O decrypted under it (R2: one RC4 pass; R3/R4: passes with key ^ 19 .. key ^ 0), 32 keystream
 *         bytes per pass -- x is only known after the last pass, so this stage has no early reject
 *   U(b)  key wave: user key of x
 *   C(b)  RC4 wave: k_pdf_r24's check of that key against U, early reject included
 * pipelined in two phases per batch so that both key derivations run behind an RC4 stage:
 *   phase A_b: RC4 wave D(b+1) | key wave U(b)        phase B_b: RC4 wave C(b) | key wave O(b+2)
 * after the prologue O(0); D(0) | O(1).  At every phase boundary the waves swap results through the S-box area, which
 * is free then: keys in words [0, 256), x in words [256, 768), between a barrier after the stage's last S-box access
 * and one after the writes; a third barrier keeps the RC4 wave's next KSA off the area until the key wave has read x.
 * The RC4 wave holds one key at a time; the key wave holds x(b+1) in registers across phase B_b. */
template <int MODE, int R, int NK>
__global__ void __launch_bounds__(128, 5)
k_pdf_r24_owner(dprf_enum e, dprf_pdf_params p, dprf_results *R_, uint32_t cap, uint32_t stop_on_first) {
    constexpr uint32_t NBAT = r24_batches<R>::v;
    static_assert(NBAT % 2 == 0, "block_prologue counts NBAT / 2 candidates per thread of the 128-thread block");
    __shared__ __attribute__((aligned(16))) uint8_t S[RC4_WAVE_BYTES];
    __shared__ __attribute__((aligned(16))) uint32_t aux[64 + 16 + 4];
    uint8_t *cs = (uint8_t *)aux;
    uint32_t *padw = aux + 64;
    uint32_t *flag = aux + 80;
    if (threadIdx.x < 8) { padw[threadIdx.x] = p.pad[threadIdx.x]; padw[threadIdx.x + 8] = p.pad[threadIdx.x]; }
    if (!block_prologue<false>(e, nullptr, R_, stop_on_first, cs, nullptr, flag, NBAT / 2)) return;
    const uint32_t base = blockIdx.x * (64u * NBAT);
    const uint32_t left = e.count - base;
    const uint32_t nb = left >= 64u * NBAT ? (uint32_t)NBAT : (left + 63u) / 64u;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t *keyx = (uint32_t *)S;                       /* [4][64] key words, only inside an exchange */
    uint32_t *xx = keyx + 256;                            /* [8][64] words of x, likewise */
#define R24O_PUT_KEY(h) do { _Pragma("unroll") for (int q = 0; q < 4; q++) keyx[64 * q + lane] = (h)[q]; } while (0)
#define R24O_GET_KEY(h) do { _Pragma("unroll") for (int q = 0; q < 4; q++) (h)[q] = keyx[64 * q + lane]; } while (0)
#define R24O_PUT_X(x) do { _Pragma("unroll") for (int q = 0; q < 8; q++) xx[64 * q + lane] = (x)[q]; } while (0)
#define R24O_GET_X(x) do { _Pragma("unroll") for (int q = 0; q < 8; q++) (x)[q] = xx[64 * q + lane]; } while (0)
    if (threadIdx.x >= 64u) {
        /* key wave */
        uint32_t padtail[8];
#pragma unroll
        for (int j = 0; j < 8; j++) padtail[j] = 0u;
        if (MODE == 0) {
            const uint32_t q = e.pwlen >> 2, r = (e.pwlen & 3u) * 8u;
#pragma unroll
            for (int t = 0; t < 8; t++) {
                const uint32_t lo = r ? (p.pad[t] << r) : p.pad[t];
                const uint32_t hi = r ? (p.pad[t] >> (32u - r)) : 0u;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    if ((uint32_t)j == q + t) padtail[j] |= lo;
                    if ((uint32_t)j == q + t + 1) padtail[j] |= hi;
                }
            }
        }
        uint32_t h[4], x[8];
#define R24O_OWNER_KEY(b) do {                                                                          \
            const uint32_t g0_ = base + 64u * (b) + lane;                                               \
            uint32_t pw_[8];                                                                            \
            r24_padded_pw<MODE>(e, cs, padw, padtail, g0_ < e.count ? g0_ : e.count - 1, pw_);          \
            r24_owner_key<R>(pw_, h);                                                                   \
        } while (0)
        R24O_OWNER_KEY(0u);
        __syncthreads(); R24O_PUT_KEY(h); __syncthreads(); __syncthreads();          /* O(0) -> RC4 wave */
        if (nb > 1u) R24O_OWNER_KEY(1u);
        __syncthreads(); R24O_PUT_KEY(h); __syncthreads(); R24O_GET_X(x); __syncthreads();   /* O(1) out, x(0) in */
#pragma unroll 1
        for (uint32_t b = 0; b < nb; b++) {
            r24_user_key<R, NK>(p, x, h);
            __syncthreads(); R24O_PUT_KEY(h); __syncthreads(); R24O_GET_X(x); __syncthreads();   /* U(b) out, x(b+1) in */
            if (b + 2u < nb) R24O_OWNER_KEY(b + 2u);
            __syncthreads(); R24O_PUT_KEY(h); __syncthreads(); __syncthreads();      /* O(b+2) out */
        }
#undef R24O_OWNER_KEY
        return;
    }
    /* RC4 wave */
    __builtin_amdgcn_s_setprio(R24_PRIO);
    uint8_t *Sw = S;
    /* the asm KSA needs the S-box area at an LDS address with zero low 16 bits, as in k_pdf_r24 */
    const uint32_t sbase = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(__attribute__((address_space(3))) uint8_t *)S);
    if (R24_KSA_ASM && (sbase & 0xffffu) != 0u) {
        if (lane == 0) atomicOr(&R_->pad_, 2u);
        for (uint32_t k = 0; k < 6u + 6u * nb; k++) __syncthreads();                 /* keep the key wave's barriers */
        return;
    }
    uint32_t h[4], d[8];
    /* D: x = O decrypted under the owner key in h */
#define R24O_DECRYPT() do {                                                                             \
        _Pragma("unroll") for (int j = 0; j < 8; j++) d[j] = p.o[j];                                    \
        if (R == 2) {                                                                                   \
            r24_ksa<5>(Sw, sbase, lane, h);                                                             \
            rc4_prga<32>(Sw, lane << 2, d);                                                             \
        } else if (R24_KSA_ASM) {                                                                       \
            uint32_t kb[NK];                                                                            \
            rc4_kb_init<NK>(h, kb);                                                                     \
            _Pragma("unroll") for (int q = 0; q < NK; q++) kb[q] ^= 19u;                                \
            for (uint32_t x = 19u; x < 20u; x--) {                                                      \
                if (x != 19u) {                                                                         \
                    const uint32_t dx = x ^ (x + 1u);                                                   \
                    _Pragma("unroll") for (int q = 0; q < NK; q++) kb[q] ^= dx;                         \
                }                                                                                       \
                rc4_ksa_asm_kb<NK>(sbase, sbase + (lane << 2), kb);                                     \
                rc4_prga<32>(Sw, lane << 2, d);                                                         \
            }                                                                                           \
        } else {                                                                                        \
            for (uint32_t x = 19u; x < 20u; x--) {                                                      \
                const uint32_t xv = x * 0x01010101u;                                                    \
                uint32_t kx[4] = {h[0] ^ xv, h[1] ^ xv, h[2] ^ xv, h[3] ^ xv};                          \
                rc4_ksa<NK>(Sw, lane << 2, kx);                                                         \
                rc4_prga<32>(Sw, lane << 2, d);                                                         \
            }                                                                                           \
        }                                                                                               \
    } while (0)
    __syncthreads(); __syncthreads(); R24O_GET_KEY(h); __syncthreads();              /* O(0) */
    R24O_DECRYPT();
    __syncthreads(); R24O_PUT_X(d); __syncthreads(); R24O_GET_KEY(h); __syncthreads();   /* x(0) out, O(1) in */
#pragma unroll 1
    for (uint32_t b = 0; b < nb; b++) {
        if (b + 1u < nb) R24O_DECRYPT();
        __syncthreads(); R24O_PUT_X(d); __syncthreads(); R24O_GET_KEY(h); __syncthreads();   /* x(b+1) out, U(b) in */
        /* C(b): k_pdf_r24's check with the user key of x */
        uint32_t lid;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lid));
        const uint32_t g = base + 64u * b + lid;
        const bool valid = g < e.count;
        bool ok = false;
        if (R == 2) {
            uint32_t c[8];
#pragma unroll
            for (int j = 0; j < 8; j++) c[j] = p.pad[j];
            r24_ksa<5>(Sw, sbase, lane, h);
            uint32_t jj = 0;
            rc4_prga_span<1, 4>(Sw, lane << 2, c, jj);
            if (__builtin_amdgcn_ballot_w64(valid && c[0] == p.u[0])) {
                rc4_prga_span<5, 32>(Sw, lane << 2, c, jj);
                ok = true;
#pragma unroll
                for (int j = 0; j < 8; j++) ok = ok && c[j] == p.u[j];
            }
        } else
        for (uint32_t full = 0; full < 2u; full++) {
            uint32_t c[4] = {p.h2[0], p.h2[1], p.h2[2], p.h2[3]};
            uint32_t kb[NK];
            rc4_kb_init<NK>(h, kb);
            for (uint32_t x = 0; x < 20u; x++) {
                if (R24_KSA_ASM) {
                    const uint32_t dx = x ^ (x - 1u);
                    if (x) {
#pragma unroll
                        for (int q = 0; q < NK; q++) kb[q] ^= dx;
                    }
                    rc4_ksa_asm_kb<NK>(sbase, sbase + (lane << 2), kb);
                } else {
                    const uint32_t xv = x * 0x01010101u;
                    uint32_t kx[4] = {h[0] ^ xv, h[1] ^ xv, h[2] ^ xv, h[3] ^ xv};
                    rc4_ksa<NK>(Sw, lane << 2, kx);
                }
                if (full) rc4_prga<16>(Sw, lane << 2, c);
                else rc4_prga<2>(Sw, lane << 2, c);
            }
            if (full) {
                ok = c[0] == p.u[0] && c[1] == p.u[1] && c[2] == p.u[2] && c[3] == p.u[3];
            } else {
                const bool pre = ((c[0] ^ p.u[0]) & 0xffffu) == 0u;
                if (!__builtin_amdgcn_ballot_w64(valid && pre)) break;
            }
        }
        if (valid && ok) report_hit(e, R_, e.start + g, cap, stop_on_first);
        __syncthreads(); __syncthreads(); R24O_GET_KEY(h); __syncthreads();          /* O(b+2) in */
    }
#undef R24O_DECRYPT
#undef R24O_PUT_KEY
#undef R24O_GET_KEY
#undef R24O_PUT_X
#undef R24O_GET_X
}

/* ================================================================== PDF R5, owner password */
/* SHA-256(pw[:127] || O[32:40] || U[0:48]) == O[0:32] (ISO 32000-2 Algorithm 12 with R5's single hash): the message is
 * the candidate plus 56 document bytes, so two blocks for candidates up to 63 bytes and three for a 64-byte one.
 * Range mode (NW = candidate words, one instantiation per launch length): everything past the candidate words -- the
 * 56 bytes at offset pwlen, the terminator and the bit length -- is launch-uniform, built once per thread from the
 * kernel arguments (scalar registers) and OR-ed onto the candidate's BE words; the second block is uniform as a whole.
 * List mode (NW = 16): the 56 bytes sit in LDS and each lane pulls message word j from words j - len / 4 - 1 and
 * j - len / 4 of them (a funnel shift by its own len % 4), so no lane indexes a register array.
 * Each thread takes PER candidates 256 apart, as k_pdf_r5's list path. */
#define R5O_PER 8
/* 3 waves per SIMD (<= 168 VGPRs): at 4 (128) the NW = 4 range instantiation spilled 12 B per lane -- the two-block
 * message with its uniform second block keeps more schedule terms live than k_pdf_r5's single block */
template <int MODE, int NW>
__global__ void __launch_bounds__(256, 3)
k_pdf_r5_owner(dprf_enum e, dprf_pdf_params p, dprf_results *R, uint32_t cap, uint32_t stop_on_first) {
    static_assert(NW >= 1 && NW <= DPRF_SLOT_WORDS, "candidate words");
    __shared__ uint8_t cs[256];
    __shared__ uint32_t flag;
    __shared__ uint32_t suf[1 + DPRF_PDF_OSUF_WORDS + 1 + 48];    /* 0 | O[32:40] || U[0:48] | 0x80 | zeros */
    if (MODE != 0) {
        for (uint32_t k = threadIdx.x; k < sizeof(suf) / 4; k += blockDim.x) {
            uint32_t v = 0u;
#pragma unroll
            for (int j = 0; j < DPRF_PDF_OSUF_WORDS; j++) v = k == (uint32_t)(j + 1) ? p.osuf[j] : v;
            suf[k] = k == DPRF_PDF_OSUF_WORDS + 1u ? 0x80u : v;
        }
    }
    if (!block_prologue<false>(e, nullptr, R, stop_on_first, cs, nullptr, &flag, R5O_PER)) return;
    const uint32_t base = blockIdx.x * (blockDim.x * R5O_PER);
    uint32_t tail[32];
    if (MODE == 0) {
        const uint32_t len = e.pwlen, q = len >> 2, r = (len & 3u) * 8u;
#pragma unroll
        for (int j = 0; j < 32; j++) tail[j] = 0u;
#pragma unroll
        for (int s = 0; s <= DPRF_PDF_OSUF_WORDS; s++) {
            const uint32_t w = s < DPRF_PDF_OSUF_WORDS ? p.osuf[s < DPRF_PDF_OSUF_WORDS ? s : 0] : 0x80u;
            const uint32_t lo = r ? (w << r) : w;
            const uint32_t hi = r ? (w >> (32u - r)) : 0u;
#pragma unroll
            for (int j = 0; j < 31; j++) {
                if ((uint32_t)j == q + s) tail[j] |= lo;
                if ((uint32_t)j == q + s + 1) tail[j] |= hi;
            }
        }
#pragma unroll
        for (int j = 0; j < 31; j++) tail[j] = bswap32(tail[j]);
        tail[31] = (len + 56u) * 8u;
    }
#pragma unroll 1
    for (uint32_t k = 0; k < (uint32_t)R5O_PER; k++) {
        const uint32_t g0 = base + k * blockDim.x + threadIdx.x;
        if (base + k * blockDim.x >= e.count) break;                 /* uniform */
        const bool valid = g0 < e.count;
        const uint32_t g = valid ? g0 : e.count - 1;
        cand c;
        get_candidate<MODE, false, LIST_CLAMP>(e, cs, g, c);
        uint32_t hh[8];
        sha256_iv(hh);
        if (MODE == 0) {
            /* range_candidate leaves the bytes past pwlen zero; pwlen <= 32: always two blocks */
            uint32_t b[16];
#pragma unroll
            for (int j = 0; j < 16; j++) b[j] = (j < NW ? bswap32(c.w[j]) : 0u) | tail[j];
            sha256_compress(hh, b);
#pragma unroll
            for (int j = 0; j < 16; j++) b[j] = tail[16 + j];
            sha256_compress(hh, b);
        } else {
            /* the host caps list candidates of an owner search at the 64-byte slot */
            const uint32_t len = c.len > 64u ? 64u : c.len;
            const uint32_t q = len >> 2, r = (len & 3u) * 8u;
            const uint32_t total = len + 56u;
            const uint32_t nblk = (total + 9u + 63u) >> 6;            /* 2, or 3 for a 64-byte candidate */
#pragma unroll
            for (int blk = 0; blk < 3; blk++) {
                if (blk == 2 && !__builtin_amdgcn_ballot_w64(nblk > 2u)) break;
                uint32_t b[16];
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const int t = 16 * blk + j;
                    /* LE message word t: candidate bytes, then suffix byte i at message byte len + i */
                    uint32_t v = t < DPRF_SLOT_WORDS ? (c.w[t < DPRF_SLOT_WORDS ? t : 0] & le_keep_mask(t, len)) : 0u;
                    const uint32_t si = (uint32_t)t + 1u - q;         /* suf[] index of the word at or above this one */
                    if ((uint32_t)t >= q) {
                        const uint32_t lo = suf[si], below = suf[si - 1u];
                        v |= r ? ((lo << r) | (below >> (32u - r))) : lo;
                    }
                    b[j] = bswap32(v);
                }
                if ((uint32_t)blk + 1u == nblk) b[15] = total * 8u;
                uint32_t st[8];
#pragma unroll
                for (int kk = 0; kk < 8; kk++) st[kk] = hh[kk];
                sha256_compress(st, b);
                if ((uint32_t)blk < nblk) {
#pragma unroll
                    for (int kk = 0; kk < 8; kk++) hh[kk] = st[kk];
                }
            }
        }
        bool ok = true;
#pragma unroll
        for (int kk = 0; kk < 8; kk++) ok = ok && hh[kk] == p.o[kk];
        if (valid && ok) report_hit(e, R, e.start + g, cap, stop_on_first);
    }
}

#endif /* DPRF_PART_PDF */

/* ------------------------------------------------------------------ launchers */

#ifdef DPRF_PART_OFFICE
hipError_t launch_office(const dprf_enum &e, const dprf_office_params &p, const dprf_aes_tables *T,
                         dprf_results *R, uint32_t cap, uint32_t stop, hipStream_t s, uint32_t *keys,
                         hipEvent_t mid) {
    if (e.mode == 0) hipLaunchKernelGGL(k_office_kdf<0>, GRID(e.count, 256), dim3(256), 0, s, e, p, R, stop, keys);
    else if (e.mode == 1) hipLaunchKernelGGL(k_office_kdf<1>, GRID(e.count, 256), dim3(256), 0, s, e, p, R, stop, keys);
    else hipLaunchKernelGGL(k_office_kdf<2>, GRID(e.count, 256), dim3(256), 0, s, e, p, R, stop, keys);
    if (mid) (void)hipEventRecord(mid, s);
    hipLaunchKernelGGL(k_office_check, GRID(e.count, 256), dim3(256), 0, s, e, p, T, R, cap, stop, keys);
    return hipGetLastError();
}
#endif

#ifdef DPRF_PART_ODT
hipError_t launch_odt(const dprf_enum &e, const dprf_odt_params &p, const dprf_aes_tables *T,
                      dprf_results *R, uint32_t cap, uint32_t stop, hipStream_t s, uint32_t *keys,
                         hipEvent_t mid) {
    if (e.mode == 0) hipLaunchKernelGGL(k_odt_kdf<0>, GRID(e.count, 256), dim3(256), 0, s, e, p, R, stop, keys);
    else if (e.mode == 1) hipLaunchKernelGGL(k_odt_kdf<1>, GRID(e.count, 256), dim3(256), 0, s, e, p, R, stop, keys);
    else hipLaunchKernelGGL(k_odt_kdf<2>, GRID(e.count, 256), dim3(256), 0, s, e, p, R, stop, keys);
    if (mid) (void)hipEventRecord(mid, s);
    hipLaunchKernelGGL(k_odt_check, GRID(e.count, ODT_CHECK_THREADS), dim3(ODT_CHECK_THREADS), 0, s, e, p, T, R, cap, stop, keys);
    return hipGetLastError();
}
#endif /* DPRF_PART_ODT */

#ifdef DPRF_PART_LONG
hipError_t launch_long_prehash(const dprf_enum &e, const dprf_long_params &lp, dprf_results *R, uint32_t cap,
                               uint32_t stop, hipStream_t s) {
    hipLaunchKernelGGL(k_long_prehash, GRID(e.count, 256), dim3(256), 0, s, e, lp, R, cap, stop);
    return hipGetLastError();
}
#endif

#ifdef DPRF_PART_PDF
hipError_t launch_pdf_r5(const dprf_enum &e, const dprf_pdf_params &p, dprf_results *R, uint32_t cap,
                         uint32_t stop, hipStream_t s) {
#define L5(M, NW, PER) hipLaunchKernelGGL((k_pdf_r5<M, NW, PER>), GRID(e.count, 256 * PER), dim3(256), 0, s, e, p, R, cap, stop)
#define L5W(NW) do { if (R5_PER_MAX >= 16 && e.cslen >= 16) L5(0, NW, 16); else L5(0, NW, 8); } while (0)
#define L5O(M, NW) hipLaunchKernelGGL((k_pdf_r5_owner<M, NW>), GRID(e.count, 256 * R5O_PER), dim3(256), 0, s, e, p, R, cap, stop)
    if (p.owner) {
        if (e.mode == 2) return hipErrorInvalidValue;    /* the host refuses long owner candidates */
        if (e.mode == 0) {
            switch ((e.pwlen + 3u) >> 2) {
            case 0: case 1: L5O(0, 1); break;
            case 2: L5O(0, 2); break;
            case 3: L5O(0, 3); break;
            case 4: L5O(0, 4); break;
            default: L5O(0, 8); break;
            }
        } else {
            L5O(1, 16);
        }
    } else
    if (e.mode == 0) {
        switch ((e.pwlen + 3u) >> 2) {
        case 0: case 1: L5W(1); break;
        case 2: L5W(2); break;
        case 3: L5W(3); break;
        case 4: L5W(4); break;
        default: L5W(8); break;
        }
    } else if (e.mode == 1 && e.pwlen <= 8) {
        L5(1, 2, 8);
    } else if (e.mode == 1 && e.pwlen <= 16) {
        L5(1, 4, 8);
    } else {
        L5(1, 8, 8);
    }
#undef L5O
#undef L5W
#undef L5
    return hipGetLastError();
}
/* R2-R4: the instantiation is (MODE, R, NK) of the user or of the owner kernel -- (R, NK) picked once, the mode once */
template <int RR, int NK>
static void launch_r24(const dprf_enum &e, const dprf_pdf_params &p, dprf_results *R, uint32_t cap, uint32_t stop,
                       hipStream_t s) {
    const auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, GRID(e.count, 64 * r24_batches<RR>::v), dim3(128), 0, s, e, p, R, cap, stop);
    };
    if (p.owner) go(e.mode == 0 ? k_pdf_r24_owner<0, RR, NK> : k_pdf_r24_owner<1, RR, NK>);
    else go(e.mode == 0 ? k_pdf_r24<0, RR, NK> : k_pdf_r24<1, RR, NK>);
}
hipError_t launch_pdf_r24(const dprf_enum &e, const dprf_pdf_params &p, dprf_results *R, uint32_t cap,
                          uint32_t stop, hipStream_t s) {
    if (p.R == 2) launch_r24<2, 5>(e, p, R, cap, stop, s);
    else if (p.n == 16) launch_r24<3, 16>(e, p, R, cap, stop, s);
    else launch_r24<3, 5>(e, p, R, cap, stop, s);
    return hipGetLastError();
}
#endif /* DPRF_PART_PDF */

#ifdef DPRF_PART_KEY40
/* ================================================================== PDF R2..R4, 40-bit key search */
/* dprf_search_key40 (include/dprf.h "40-bit key search"): the candidate is the RC4 key itself.  Index i = e.start + g
 * stands for the five bytes of i written big-endian, so nothing is hashed and the workgroup has no key wave: one RC4
 * wave of 64 threads over NBAT batches of 64 keys (rc4_wg.h rc4_wg_run1), the lane's key words formed in registers and
 * judged by r24_check<R, 5> as it stands -- R2: RC4(key, PAD) against U[0:32]; R3/R4 with Length 40: the 20-pass
 * chain against U[0:16].  LDS: the 16 KiB S-box area first (LDS address 0: rc4_wg_sbox_base) and the skip flag, 16,400
 * B per workgroup: 9 per CU, as k_pdf_r24 (a tenth chain loses). */
template <int R>
__global__ void __launch_bounds__(64, 3)   /* 9 one-wave workgroups per CU: at most 3 waves on a SIMD */
k_key40_pdf(dprf_enum e, dprf_pdf_params p, dprf_results *R_, uint32_t cap, uint32_t stop_on_first) {
    constexpr uint32_t NBAT = r24_batches<R>::v;
    __shared__ __attribute__((aligned(16))) key40_lds L;
    uint8_t *S = L.S;
    /* per = keys per thread of the 64-thread block: 64 * NBAT keys; no charset to stage */
    if (!block_prologue<false, true, false>(e, nullptr, R_, stop_on_first, nullptr, nullptr, L.flag, NBAT)) return;
    rc4_wg_run1<NBAT>(e, S, R24_KSA_ASM, R_, R24_ERR_LDS,
                      [&](const rc4_wg &w, uint32_t sbase, uint32_t b) {
                          const uint32_t g = w.base + 64u * b + rc4_wg_lane_id();
                          const uint64_t i = e.start + g;   /* 64-bit: a launch may cross index 2^32 */
                          uint32_t k[4];
                          rc4_wg_key40(i, k);
                          if (r24_check<R, 5>(S, sbase, w.lane, p, k, g < e.count))
                              report_hit(e, R_, i, cap, stop_on_first);
                      });
}

hipError_t launch_key40_pdf(const dprf_enum &e, const dprf_pdf_params &p, dprf_results *R, uint32_t cap,
                            uint32_t stop, hipStream_t s) {
    /* the host refuses every other document (dprf_doc.cpp check_key40) */
    if (e.mode != DPRF_ENUM_KEY40 || p.R < 2u || p.R > 4u || (p.R != 2u && p.n != 5u)) return hipErrorInvalidValue;
    if (p.R == 2)
        hipLaunchKernelGGL(k_key40_pdf<2>, GRID(e.count, 64 * r24_batches<2>::v), dim3(64), 0, s, e, p, R, cap, stop);
    else
        hipLaunchKernelGGL(k_key40_pdf<3>, GRID(e.count, 64 * r24_batches<3>::v), dim3(64), 0, s, e, p, R, cap, stop);
    return hipGetLastError();
}
#endif /* DPRF_PART_KEY40 */

#ifdef DPRF_PART_COLLIDE
/* ================================================================== PDF R2..R4, password for a known 40-bit key */
/* dprf_ctx_set_key40 (include/dprf.h "password for a known key"): a candidate verifies when its user key -- the MD5 of
 * the padded password and the document tail, for R3/R4 with Length 40 the 50 further MD5s of five bytes: r24_key, as
 * k_pdf_r24's key wave computes it -- is the key the context was given.  Nothing of U is read and no RC4 runs: no S-box, no key wave, no two-wave frame.  The shape is
 * k_pdf_r5's: a 256-thread block, PER candidates per thread 256 apart, 336 B of LDS (charset, PAD || PAD, skip flag).
 * k0 / k1: the key's bytes 0..3 as an LE word and its byte 4 (dprf_doc.h key40_words) -- h[0] and h[1] & 0xff. */
#ifndef COLLIDE_R2_PER
#define COLLIDE_R2_PER 8            /* two compressions per candidate: the prologue is spread as for R5 */
#endif
#ifndef COLLIDE_R3_PER
#define COLLIDE_R3_PER 2            /* 52 compressions per candidate: the prologue is noise either way */
#endif
struct collide_pdf_lds {
    uint8_t cs[256];                                      /* charset */
    uint32_t padw[16];                                    /* PAD || PAD */
    uint32_t flag[4];                                     /* block_prologue's skip flag */
};
template <int MODE, int R>
__global__ void __launch_bounds__(256, 4)
k_collide_pdf(dprf_enum e, dprf_pdf_params p, uint32_t k0, uint32_t k1, dprf_results *R_, uint32_t cap,
              uint32_t stop_on_first) {
    constexpr uint32_t PER = R == 2 ? COLLIDE_R2_PER : COLLIDE_R3_PER;
    __shared__ __attribute__((aligned(16))) collide_pdf_lds L;
    if (threadIdx.x < 8) { L.padw[threadIdx.x] = p.pad[threadIdx.x]; L.padw[threadIdx.x + 8] = p.pad[threadIdx.x]; }
    if (!block_prologue<false>(e, nullptr, R_, stop_on_first, L.cs, nullptr, L.flag, PER)) return;
    uint32_t padtail[8];
    r24_padtail<MODE>(e, p, padtail);
    const uint32_t base = blockIdx.x * (256u * PER);
#pragma unroll 1
    for (uint32_t k = 0; k < PER; k++) {
        if (base + 256u * k >= e.count) break;                       /* uniform */
        const uint32_t g0 = base + 256u * k + threadIdx.x;
        const bool valid = g0 < e.count;
        const uint32_t g = valid ? g0 : e.count - 1u;
        uint32_t h[4];
        r24_key<MODE, R, 5>(e, p, L.cs, L.padw, padtail, g, h);
        if (valid && h[0] == k0 && (h[1] & 0xffu) == k1) report_hit(e, R_, e.start + g, cap, stop_on_first);
    }
}

hipError_t launch_collide_pdf(const dprf_enum &e, const dprf_pdf_params &p, const uint32_t key[2], dprf_results *R,
                              uint32_t cap, uint32_t stop, hipStream_t s) {
    /* the host refuses every other document and the owner mode (dprf_doc.cpp check_set_key40) */
    if (e.mode > 1u || p.owner || p.R < 2u || p.R > 4u || (p.R != 2u && p.n != 5u)) return hipErrorInvalidValue;
    const auto go = [&](auto kernel, uint32_t per) {
        hipLaunchKernelGGL(kernel, GRID(e.count, 256u * per), dim3(256), 0, s, e, p, key[0], key[1], R, cap, stop);
    };
    if (p.R == 2) go(e.mode == 0 ? k_collide_pdf<0, 2> : k_collide_pdf<1, 2>, COLLIDE_R2_PER);
    else go(e.mode == 0 ? k_collide_pdf<0, 3> : k_collide_pdf<1, 3>, COLLIDE_R3_PER);
    return hipGetLastError();
}
#endif /* DPRF_PART_COLLIDE */
