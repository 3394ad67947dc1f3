/* dprf_kernels_oldoffice.hip -- Office 97-2003 binary documents (.doc / .xls), RC4 encryption
 * (MS-OFFCRYPTO 2.3.6 "RC4" and 2.3.5 "RC4 CryptoAPI"; include/dprf.h "Office 97-2003"), one candidate per lane,
 * one launch per batch:
 *   k_oldoffice<MODE, false>   types 0 / 1: h = MD5(pw16); h = MD5((h[0:5] || salt) x 16); k = MD5(h[0:5] || LE32(0));
 *                              d = RC4(k, encryptedVerifier || encryptedVerifierHash) (32 bytes);
 *                              a hit when MD5(d[0:16]) == d[16:32]
 *   k_oldoffice<MODE, true>    types 3 / 4: h = SHA1(salt || pw16); k = SHA1(h || LE32(0)); key = k[0:5] || 11 x 00
 *                              (type 3) or k[0:16] (type 4); d = RC4(key, ...) (36 bytes);
 *                              a hit when SHA1(d[0:16]) == d[16:36]
 * pw16 is the candidate in UTF-16LE.  MODE 0 enumerates the range index, MODE 1 reads the list / spelled slot.  No
 * reference verifier exists for this stream: the definition is pinned by tests/oldoffice_model.py and the public
 * vectors in tests/golden/oldoffice_vectors.json.
 *
 * The workgroup is k_pdf_r24's (dprf_kernels.hip; written out here and not on rc4_wg.h's driver: on the driver both
 * families measured below the parent's rate, HISTORY.md): one RC4 wave that owns a 16 KiB S-box area (rc4_dev.h, one 256-byte
 * box per lane) and one key wave that hashes the RC4 keys of batch b + 1 while the RC4 wave runs batch b; the keys
 * change hands through the S-box area between two barriers.  16,656 bytes of LDS per workgroup: 9 workgroups per CU.
 *
 * A translation unit of its own: the other kernel objects keep their machine code.  The candidate source, the
 * block prologue and be_append are dprf_cand.h's.
 */
#include "dev_crypto.h"
#include "dprf_params.h"
#include "dprf_launch.h"
#include "dprf_hits.h"
#include "dprf_cand.h"
#include "rc4_dev.h"

namespace {
/* ------------------------------------------------------------------ RC4 key of one candidate */
/* Types 0 / 1: nine MD5 compressions at most (the first message is one block up to 27 characters, two from 28). */
DEVI void key_md5(const dprf_oldoffice_params &p, const cand &c, uint32_t k[4]) {
    uint32_t h[4];
    {
        /* h = MD5(pw16): the slot's words are the message as they stand (MD5 reads LE words) */
        uint32_t b0[16], b1[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            b0[j] = (c.w[j] & le_keep_mask(j, c.len)) | le_pad80(j, c.len);
            b1[j] = 0u;
        }
        /* a candidate that fills its whole slot has its terminator in the word after it */
        b1[0] = c.len == 4u * DPRF_SLOT_WORDS ? 0x80u : 0u;
        const bool two = c.len > 55u;
        if (!two) b0[14] = c.len * 8u;       /* len <= 55: words 14, 15 hold no candidate byte */
        b1[14] = c.len * 8u;
        md5_iv(h);
        md5_compress(h, b0);
        if (two) md5_compress(h, b1);
    }
    {
        /* h = MD5((h[0:5] || salt) x 16): 336 bytes, six blocks.  p.rep holds the whole padded message with the 16
         * salt copies in place and zeros where the five hash bytes go: document constants, read as kernel arguments.
         * Copy r of the five bytes starts at byte 21 r -- a compile-time word and shift. */
        const uint32_t lo = h[0], hi = h[1] & 0xffu;
        md5_iv(h);
#pragma unroll
        for (int b = 0; b < 6; b++) {
            uint32_t m[16];
#pragma unroll
            for (int j = 0; j < 16; j++) m[j] = p.rep[16 * b + j];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int w = (21 * r) >> 2, s = 8 * ((21 * r) & 3);
                const int j0 = w - 16 * b, j1 = w + 1 - 16 * b;
                if (j0 >= 0 && j0 < 16) m[j0] |= lo << s;
                if (j1 >= 0 && j1 < 16) m[j1] |= (s ? lo >> (32 - s) : 0u) | (hi << s);
            }
            md5_compress(h, m);
        }
    }
    {
        /* k = MD5(h[0:5] || LE32(0)): 9 bytes; all 16 bytes of k are the RC4 key of block 0 */
        uint32_t m[16];
#pragma unroll
        for (int j = 0; j < 16; j++) m[j] = 0u;
        m[0] = h[0];
        m[1] = h[1] & 0xffu;
        m[2] = 0x8000u;
        m[14] = 72u;
        md5_iv(k);
        md5_compress(k, m);
    }
}

/* Types 3 / 4: three or four SHA-1 compressions (salt || pw16 is one block up to 19 characters, two from 20). */
DEVI void key_sha1(const dprf_oldoffice_params &p, const cand &c, uint32_t k[4]) {
    uint32_t h[5];
    {
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
    /* k = SHA1(h || LE32(0)): 24 bytes */
    uint32_t w[16] = {h[0], h[1], h[2], h[3], h[4], 0u, 0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 192u};
    uint32_t s[5];
    sha1_iv(s);
    sha1_compress(s, w);
    /* the RC4 key, LE-packed: 40-bit keys are the first five bytes zero-extended to 16 (a 16-byte key, not a 5-byte
     * one: the schedule differs) */
    k[0] = bswap32(s[0]);
    if (p.key_bytes == 5u) {
        k[1] = bswap32(s[1]) & 0xffu;
        k[2] = 0u;
        k[3] = 0u;
    } else {
        k[1] = bswap32(s[1]);
        k[2] = bswap32(s[2]);
        k[3] = bswap32(s[3]);
    }
}

template <int MODE, bool SHA1>
DEVI void oldoffice_key(const dprf_enum &e, const dprf_oldoffice_params &p, const uint8_t *cs, uint32_t g,
                        uint32_t k[4]) {
    cand c;
    get_candidate<MODE, true>(e, cs, g, c);
    if (SHA1) key_sha1(p, c, k);
    else key_md5(p, c, k);
}
}  // namespace

/* Batches of 64 candidates per workgroup; even, since the 128-thread block counts OLDOFFICE_BATCHES / 2 candidates
 * per thread.  Measured on MI355X (tools/bench_oldoffice.py, two alternating passes, G cand/s, MD5 / SHA-1 family):
 * 8 / 16 / 32 batches 7.77 / 7.93 / 8.00 and 8.46 / 8.66 / 8.77 under the max-ilp scheduler, 16 / 32 / 64 batches
 * 8.04 / 8.07 / 8.05 and 9.01 / 9.10 / 9.12 under the default one (Makefile SCHED_OLDOFFICE), so 32 -- close to
 * k_pdf_r24's 36 for R2, the other family with one KSA per candidate. */
#ifndef OLDOFFICE_BATCHES
#define OLDOFFICE_BATCHES 32
#endif
#ifndef OLDOFFICE_PRIO
#define OLDOFFICE_PRIO 3
#endif
/* 1: the KSA as the generated asm block (rc4_dev.h rc4_ksa_asm<16>); 0: the C++ rc4_ksa<16> (A/B builds) */
#ifndef OLDOFFICE_KSA_ASM
#define OLDOFFICE_KSA_ASM 1
#endif
/* dprf_results.pad_ bit of this kernel's LDS-address assumption (1, 2, 4, 8 are taken: dprf_params.h) */
#define OLDOFFICE_ERR_LDS 16u

template <int MODE, bool SHA1>
__global__ void __launch_bounds__(128, 5)   /* 18 waves per CU (9 workgroups): <= 102 VGPRs */
k_oldoffice(dprf_enum e, dprf_oldoffice_params p, dprf_results *R_, uint32_t cap, uint32_t stop_on_first) {
    constexpr uint32_t NBAT = OLDOFFICE_BATCHES;
    static_assert(NBAT % 2 == 0, "block_prologue counts NBAT / 2 candidates per thread of the 128-thread block");
    __shared__ __attribute__((aligned(16))) uint8_t S[RC4_WAVE_BYTES];
    __shared__ __attribute__((aligned(16))) uint32_t aux[64 + 4];
    uint8_t *cs = (uint8_t *)aux;                         /* charset, 256 B */
    uint32_t *flag = aux + 64;
    if (!block_prologue<false>(e, nullptr, R_, stop_on_first, cs, nullptr, flag, NBAT / 2)) return;
    const uint32_t base = blockIdx.x * (64u * NBAT);
    const uint32_t left = e.count - base;                 /* > 0: grid = ceil(count / (64 * NBAT)) */
    const uint32_t nb = left >= 64u * NBAT ? (uint32_t)NBAT : (left + 63u) / 64u;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t *keyx = (uint32_t *)S;                       /* [4][64] words, only between the two barriers */
    if (threadIdx.x >= 64u) {
        /* key wave */
        uint32_t k[4];
        {
            const uint32_t g0 = base + lane;
            oldoffice_key<MODE, SHA1>(e, p, cs, g0 < e.count ? g0 : e.count - 1, k);
        }
#pragma unroll 1
        for (uint32_t b = 0; b < nb; b++) {
            __syncthreads();                              /* the RC4 wave is done with batch b-1's S-box */
#pragma unroll
            for (int q = 0; q < 4; q++) keyx[64 * q + lane] = k[q];
            __syncthreads();                              /* batch b's keys are in LDS */
            if (b + 1u < nb) {
                const uint32_t g0 = base + 64u * (b + 1u) + lane;
                oldoffice_key<MODE, SHA1>(e, p, cs, g0 < e.count ? g0 : e.count - 1, k);
            }
        }
        return;
    }
    /* RC4 wave */
    __builtin_amdgcn_s_setprio(OLDOFFICE_PRIO);
    /* the asm KSA needs the S-box area at an LDS address with zero low 16 bits (rc4_ksa_asm); S is this kernel's
     * first LDS object, at 0 -- checked, and a launch that ever breaks it fails loudly instead of computing wrong */
    const uint32_t sbase = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(__attribute__((address_space(3))) uint8_t *)S);
    if (OLDOFFICE_KSA_ASM && (sbase & 0xffffu) != 0u) {
        if (lane == 0) atomicOr(&R_->pad_, OLDOFFICE_ERR_LDS);
        for (uint32_t b = 0; b < nb; b++) { __syncthreads(); __syncthreads(); }   /* keep the key wave's barriers */
        return;
    }
#pragma unroll 1
    for (uint32_t b = 0; b < nb; b++) {
        __syncthreads();
        __syncthreads();
        uint32_t k[4];
#pragma unroll
        for (int q = 0; q < 4; q++) k[q] = keyx[64 * q + lane];
        if (OLDOFFICE_KSA_ASM) rc4_ksa_asm<16>(sbase, sbase + (lane << 2), k);
        else rc4_ksa<16>(S, lane << 2, k);
        /* one continuous keystream over encryptedVerifier || encryptedVerifierHash, then the hash of the verifier
         * against all 16 / 20 bytes of the decrypted hash: no prefilter */
        bool ok;
        if (SHA1) {
            uint32_t d[9];
#pragma unroll
            for (int j = 0; j < 4; j++) d[j] = p.ev[j];
#pragma unroll
            for (int j = 0; j < 5; j++) d[4 + j] = p.evh[j];
            rc4_prga<36>(S, lane << 2, d);
            uint32_t w[16] = {bswap32(d[0]), bswap32(d[1]), bswap32(d[2]), bswap32(d[3]), 0x80000000u, 0, 0, 0,
                              0, 0, 0, 0, 0, 0, 0, 128u};
            uint32_t s[5];
            sha1_iv(s);
            sha1_compress(s, w);
            ok = true;
#pragma unroll
            for (int j = 0; j < 5; j++) ok = ok && s[j] == bswap32(d[4 + j]);
        } else {
            uint32_t d[8];
#pragma unroll
            for (int j = 0; j < 4; j++) { d[j] = p.ev[j]; d[4 + j] = p.evh[j]; }
            rc4_prga<32>(S, lane << 2, d);
            uint32_t m[16];
#pragma unroll
            for (int j = 0; j < 16; j++) m[j] = 0u;
            m[0] = d[0]; m[1] = d[1]; m[2] = d[2]; m[3] = d[3];
            m[4] = 0x80u;
            m[14] = 128u;
            uint32_t s[4];
            md5_iv(s);
            md5_compress(s, m);
            ok = s[0] == d[4] && s[1] == d[5] && s[2] == d[6] && s[3] == d[7];
        }
        /* the lane index recomputed here (v_mbcnt), as k_pdf_r24 does: not held in a register across the KSA */
        uint32_t lid;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lid));
        const uint32_t g = base + 64u * b + lid;
        if (g < e.count && ok) report_hit(e, R_, e.start + g, cap, stop_on_first);
    }
}

/* ------------------------------------------------------------------ launcher */
hipError_t launch_oldoffice(const dprf_enum &e, const dprf_oldoffice_params &p, dprf_results *R, uint32_t cap,
                            uint32_t stop, hipStream_t s) {
    /* the host refuses candidates longer than a slot: no long-list mode */
    if (e.mode > 1u || (p.sha1 && p.key_bytes != 5u && p.key_bytes != 16u)) return hipErrorInvalidValue;
    const auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, GRID(e.count, 64u * OLDOFFICE_BATCHES), dim3(128), 0, s, e, p, R, cap, stop);
    };
    if (p.sha1) go(e.mode == 0 ? k_oldoffice<0, true> : k_oldoffice<1, true>);
    else go(e.mode == 0 ? k_oldoffice<0, false> : k_oldoffice<1, false>);
    return hipGetLastError();
}
