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
#include "rc4_wg.h"

/* The file is compiled three times (Makefile): the password kernel k_oldoffice; with DPRF_PART_KEY40 the 40-bit key
 * search k_key40_oldoffice, in an object of its own (the two share the verdict stage); and with DPRF_PART_COLLIDE the
 * password search against a known key, k_collide_oldoffice at the end of the file, in an object of its own again. */
#if !defined(DPRF_PART_KEY40) && !defined(DPRF_PART_COLLIDE)
namespace {
/* ------------------------------------------------------------------ RC4 key of one candidate */
/* key_md5 and key_sha1 have twins that stop at the five key bytes, collide_md5 and collide_sha1 at the end of the file:
 * with the two functions here split at that point and shared, k_oldoffice's object no longer compared equal to the
 * measured one, so they stay as they are -- a fix here is due there too. */
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
#endif /* !DPRF_PART_KEY40 && !DPRF_PART_COLLIDE */

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

/* The verdict of one lane under its 16-byte RC4 key k, by the RC4 wave of the key search (k_key40_oldoffice): the KSA,
 * one continuous keystream over encryptedVerifier || encryptedVerifierHash, then the hash of the verifier against all
 * 16 / 20 bytes of the decrypted hash: no prefilter.  The stage has a twin: k_oldoffice below keeps it written out --
 * built on this function its object no longer compared equal to the measured one -- so a fix here is due there too. */
template <bool SHA1>
DEVI bool oldoffice_verdict(uint8_t *S, uint32_t sbase, uint32_t lane, const dprf_oldoffice_params &p,
                            const uint32_t k[4]) {
    if (OLDOFFICE_KSA_ASM) rc4_ksa_asm<16>(sbase, sbase + (lane << 2), k);
    else rc4_ksa<16>(S, lane << 2, k);
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
    return ok;
}

#if !defined(DPRF_PART_KEY40) && !defined(DPRF_PART_COLLIDE)
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

#elif defined(DPRF_PART_KEY40)
/* ------------------------------------------------------------------ 40-bit key search */
/* dprf_search_key40 (include/dprf.h "40-bit key search"): the candidate is the 40 bits of key the document has.  Index
 * i = e.start + g stands for five bytes b0..b4, i written big-endian (rc4_wg_key40):
 *   k_key40_oldoffice<false, W>   types 0 / 1: the bytes are h[0:5] of the second MD5; k = MD5(b0..b4 || LE32(0)), then
 *                                 k_oldoffice's verdict stage
 *   k_key40_oldoffice<true, 1>    type 3: the RC4 key is b0..b4 || 11 x 00 -- nothing is hashed before the KSA
 * W = 2: k_oldoffice's workgroup (rc4_wg.h rc4_wg_run), the key wave running the one MD5 compression of batch b + 1
 * behind the RC4 wave's batch b.  W = 1: a 64-thread workgroup without a key wave (rc4_wg_run1); with KEY40_MD5_WAVES 1
 * the MD5 family hashes in the RC4 wave itself (the A/B of DESIGN.md 4g).  LDS: the S-box area and the skip flag,
 * 16,400 B per workgroup: 9 per CU either way. */
#ifndef KEY40_MD5_WAVES
#define KEY40_MD5_WAVES 2
#endif
/* The 16-byte RC4 key of key index i */
template <bool SHA1>
DEVI void key40_key(uint64_t i, uint32_t k[4]) {
    uint32_t b[4];
    rc4_wg_key40(i, b);
    if (SHA1) {
#pragma unroll
        for (int q = 0; q < 4; q++) k[q] = b[q];
    } else {
        /* k = MD5(b0..b4 || LE32(0)): 9 bytes, one compression; all 16 bytes of k are the RC4 key */
        uint32_t m[16];
#pragma unroll
        for (int j = 0; j < 16; j++) m[j] = 0u;
        m[0] = b[0];
        m[1] = b[1];
        m[2] = 0x8000u;
        m[14] = 72u;
        md5_iv(k);
        md5_compress(k, m);
    }
}

template <bool SHA1, int WAVES>
__global__ void __launch_bounds__(64 * WAVES, WAVES == 2 ? 5 : 3)   /* 9 workgroups per CU */
k_key40_oldoffice(dprf_enum e, dprf_oldoffice_params p, dprf_results *R_, uint32_t cap, uint32_t stop_on_first) {
    constexpr uint32_t NBAT = OLDOFFICE_BATCHES;
    __shared__ __attribute__((aligned(16))) key40_lds L;
    uint8_t *S = L.S;
    /* per = keys per thread of the block: 64 * NBAT keys; no charset to stage */
    if (!block_prologue<false, true, false>(e, nullptr, R_, stop_on_first, nullptr, nullptr, L.flag, NBAT / WAVES)) return;
    /* RC4 wave: the verdict of batch b under the lane's key k */
    const auto stage = [&](const rc4_wg &w, uint32_t sbase, uint32_t b, const uint32_t k[4]) {
        const bool ok = oldoffice_verdict<SHA1>(S, sbase, w.lane, p, k);
        const uint32_t g = w.base + 64u * b + rc4_wg_lane_id();
        if (g < e.count && ok) report_hit(e, R_, e.start + g, cap, stop_on_first);
    };
    if constexpr (WAVES == 2)
        rc4_wg_run<NBAT, OLDOFFICE_PRIO>(e, S, OLDOFFICE_KSA_ASM, R_, OLDOFFICE_ERR_LDS,
                                         [&](uint32_t g, uint32_t k[4]) { key40_key<SHA1>(e.start + g, k); }, stage);
    else
        rc4_wg_run1<NBAT>(e, S, OLDOFFICE_KSA_ASM, R_, OLDOFFICE_ERR_LDS,
                          [&](const rc4_wg &w, uint32_t sbase, uint32_t b) {
                              uint32_t k[4];
                              key40_key<SHA1>(e.start + (w.base + 64u * b + rc4_wg_lane_id()), k);
                              stage(w, sbase, b, k);
                          });
}

hipError_t launch_key40_oldoffice(const dprf_enum &e, const dprf_oldoffice_params &p, dprf_results *R, uint32_t cap,
                                  uint32_t stop, hipStream_t s) {
    /* the host refuses type 4 (a 128-bit key): dprf_doc.cpp check_key40 */
    if (e.mode != DPRF_ENUM_KEY40 || (p.sha1 && p.key_bytes != 5u)) return hipErrorInvalidValue;
    const dim3 grid = GRID(e.count, 64u * OLDOFFICE_BATCHES);
    if (p.sha1)
        hipLaunchKernelGGL((k_key40_oldoffice<true, 1>), grid, dim3(64), 0, s, e, p, R, cap, stop);
    else
        hipLaunchKernelGGL((k_key40_oldoffice<false, KEY40_MD5_WAVES>), grid, dim3(64 * KEY40_MD5_WAVES), 0, s, e, p, R,
                           cap, stop);
    return hipGetLastError();
}
#else /* DPRF_PART_COLLIDE */
/* ------------------------------------------------------------------ password for a known 40-bit key */
/* dprf_ctx_set_key40 (include/dprf.h "password for a known key"): a candidate verifies when the 40 bits of key it
 * derives are the key the context was given --
 *   k_collide_oldoffice<MODE, false>   types 0 / 1: collide_md5, then h[0:5] == K; the third MD5 is not computed
 *   k_collide_oldoffice<MODE, true>    type 3: collide_sha1, then s[0:5] == K
 * Neither encryptedVerifier nor encryptedVerifierHash is read and no RC4 runs: no S-box, no key wave.  The shape is
 * k_pdf_r5's: a 256-thread block, COLLIDE_OO_PER candidates per thread 256 apart, 272 B of LDS (charset, skip flag).
 * k0 / k1: the key's bytes 0..3 as an LE word and its byte 4 (dprf_doc.h key40_words). */
#ifndef COLLIDE_OO_PER
#define COLLIDE_OO_PER 4
#endif
namespace {
/* The first two stages of key_md5 (top of the file), its twin: k_oldoffice keeps key_md5 whole -- split and shared, its
 * object no longer compared equal to the measured one -- so a fix there is due here too.  Eight MD5 compressions at
 * most (the first message is one block up to 27 characters, two from 28). */
DEVI void collide_md5(const dprf_oldoffice_params &p, const cand &c, uint32_t h[4]) {
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
    /* h = MD5((h[0:5] || salt) x 16): 336 bytes, six blocks of p.rep with the five bytes OR-ed in: copy r of them
     * starts at byte 21 r -- a compile-time word and shift */
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
/* key_sha1 up to its second digest, its twin likewise: s = SHA1(SHA1(salt || pw16) || LE32(0)), two or three SHA-1
 * compressions (salt || pw16 is one block up to 19 characters, two from 20) */
DEVI void collide_sha1(const dprf_oldoffice_params &p, const cand &c, uint32_t s[5]) {
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
    /* SHA1(h || LE32(0)): 24 bytes */
    uint32_t w[16] = {h[0], h[1], h[2], h[3], h[4], 0u, 0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 192u};
    sha1_iv(s);
    sha1_compress(s, w);
}
}  // namespace
template <int MODE, bool SHA1>
__global__ void __launch_bounds__(256, 4)
k_collide_oldoffice(dprf_enum e, dprf_oldoffice_params p, uint32_t k0, uint32_t k1, dprf_results *R_, uint32_t cap,
                    uint32_t stop_on_first) {
    constexpr uint32_t PER = COLLIDE_OO_PER;
    __shared__ __attribute__((aligned(16))) uint32_t aux[64 + 4];
    uint8_t *cs = (uint8_t *)aux;                         /* charset, 256 B */
    if (!block_prologue<false>(e, nullptr, R_, stop_on_first, cs, nullptr, aux + 64, PER)) return;
    const uint32_t base = blockIdx.x * (256u * PER);
#pragma unroll 1
    for (uint32_t k = 0; k < PER; k++) {
        if (base + 256u * k >= e.count) break;                       /* uniform */
        const uint32_t g0 = base + 256u * k + threadIdx.x;
        const bool valid = g0 < e.count;
        const uint32_t g = valid ? g0 : e.count - 1u;
        cand c;
        get_candidate<MODE, true>(e, cs, g, c);
        bool ok;
        if (SHA1) {
            uint32_t s[5];
            collide_sha1(p, c, s);
            ok = bswap32(s[0]) == k0 && (bswap32(s[1]) & 0xffu) == k1;
        } else {
            uint32_t h[4];
            collide_md5(p, c, h);
            ok = h[0] == k0 && (h[1] & 0xffu) == k1;
        }
        if (valid && ok) report_hit(e, R_, e.start + g, cap, stop_on_first);
    }
}

hipError_t launch_collide_oldoffice(const dprf_enum &e, const dprf_oldoffice_params &p, const uint32_t key[2],
                                    dprf_results *R, uint32_t cap, uint32_t stop, hipStream_t s) {
    /* the host refuses type 4 (a 128-bit key) and candidates longer than a slot (dprf_doc.cpp check_set_key40) */
    if (e.mode > 1u || (p.sha1 && p.key_bytes != 5u)) return hipErrorInvalidValue;
    const auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, GRID(e.count, 256u * COLLIDE_OO_PER), dim3(256), 0, s, e, p, key[0], key[1], R, cap,
                           stop);
    };
    if (p.sha1) go(e.mode == 0 ? k_collide_oldoffice<0, true> : k_collide_oldoffice<1, true>);
    else go(e.mode == 0 ? k_collide_oldoffice<0, false> : k_collide_oldoffice<1, false>);
    return hipGetLastError();
}
#endif /* DPRF_PART_KEY40 / DPRF_PART_COLLIDE */
