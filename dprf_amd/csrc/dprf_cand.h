/* dprf_cand.h -- the candidate source and the block prologue of the one-candidate-per-lane kernels (device side).
 *
 * The only definition of: the candidate a lane verifies (`cand`) and the two ways to it (on-device enumeration of a
 * keyspace index, or a packed slot), the per-block skip decision that makes stop_on_first report the lowest hit, the
 * slot-to-message builder and the GRID macro of the launchers.  Every kernel source but dprf_kernels_r6.hip (its own
 * runtime-loop enumeration) and dprf_kernels_spell.hip (it writes slots, it reads none) includes it.  Everything here
 * is inlined: the text is shared, each object keeps the machine code it had with a copy of its own.
 */
#ifndef DPRF_CAND_H
#define DPRF_CAND_H
#include "dev_crypto.h"
#include "dprf_params.h"
#include "dprf_hits.h"

/* ------------------------------------------------------------------ candidate source */
struct cand {
    uint32_t w[DPRF_SLOT_WORDS];   /* LE-packed bytes (UTF-16LE code units for the Office formats) */
    uint32_t len;                  /* bytes */
};

/* Keyspace index start+g -> candidate, itertools.product order (brute_force.py:205): the digit at
 * position pwlen-1 varies fastest.  UTF16: emit UTF-16LE code units (Office; ASCII charset only). */
template <bool UTF16>
DEVI void range_candidate(const dprf_enum &e, const uint8_t *cs, uint32_t g, cand &c) {
#pragma unroll
    for (int j = 0; j < DPRF_SLOT_WORDS; j++) c.w[j] = 0;
    uint32_t rem = g, carry = 0;
#pragma unroll
    for (int p = DPRF_MAX_RANGE_LEN - 1; p >= 0; --p) {
        if ((uint32_t)p < e.pwlen) {
            uint32_t q = e.cslen == 1 ? rem : fastdiv(rem, e.div_m, e.div_s);
            uint32_t r = rem - q * e.cslen;
            uint32_t d = (uint32_t)e.sdig[p] + r + carry;
            carry = d >= e.cslen ? 1u : 0u;
            d -= carry ? e.cslen : 0u;
            rem = q;
            uint32_t ch = cs[d];
            if (UTF16) c.w[p >> 1] |= ch << (16 * (p & 1));
            else c.w[p >> 2] |= ch << (8 * (p & 3));
        }
    }
    c.len = UTF16 ? 2 * e.pwlen : e.pwlen;
}

/* CLAMP: the host never packs more than a slot; the clamp keeps the message builders inside their arrays whatever
 * the length byte holds. */
template <bool CLAMP = true>
DEVI void list_candidate(const dprf_enum &e, uint32_t g, cand &c) {
    const uint64_t slot = e.start + g;
    const uint4 *s = (const uint4 *)(e.slots + slot * DPRF_SLOT_WORDS);
#pragma unroll
    for (int q = 0; q < DPRF_SLOT_WORDS / 4; q++) {
        uint4 v = s[q];
        c.w[4 * q + 0] = v.x; c.w[4 * q + 1] = v.y; c.w[4 * q + 2] = v.z; c.w[4 * q + 3] = v.w;
    }
    const uint32_t len = e.lens[slot];
    c.len = !CLAMP || len < 4u * DPRF_SLOT_WORDS ? len : 4u * DPRF_SLOT_WORDS;
}

template <int MODE, bool UTF16, bool CLAMP = true>
DEVI void get_candidate(const dprf_enum &e, const uint8_t *cs, uint32_t g, cand &c) {
    if (MODE == 0) range_candidate<UTF16>(e, cs, g, c);
    else list_candidate<CLAMP>(e, g, c);
}

/* ------------------------------------------------------------------ block prologue */
/* Stage the charset (and optionally the AES tables) into LDS and decide once per block whether it runs.
 * With stop_on_first a block is skipped only when its LOWEST candidate index lies above the lowest hit
 * known so far (R->first, and across devices the call's, dprf_hits.h): every index below the final `first` is
 * then verified whatever order the workgroups are dispatched in, so the reported hit is the lowest of the call
 * unconditionally (a boolean stop flag would let a late-dispatched lower block skip itself).  `per` = candidates
 * per thread.
 * COUNT: this kernel's skipped blocks are counted in R->skipped (the verifying kernel of a format; the
 * KDF kernels of Office/ODF skip exactly the blocks their check kernel skips and do not count).
 * STAGE_CS false: the kernel has no charset in LDS, or stages it itself (cs is not touched). */
template <bool AES, bool COUNT = true, bool STAGE_CS = true>
DEVI bool block_prologue(const dprf_enum &e, const dprf_aes_tables *T, dprf_results *R, uint32_t stop_on_first,
                         uint8_t *cs, aes_lds *L, uint32_t *flag, uint32_t per = 1) {
    const uint32_t tid = threadIdx.x;
    if (STAGE_CS)
        for (uint32_t k = tid; k < 64; k += blockDim.x) ((uint32_t *)cs)[k] = ((const uint32_t *)e.charset)[k];
    if (AES) {
        for (uint32_t k = tid; k < 256; k += blockDim.x) { L->te[k] = T->te0[k]; L->td[k] = T->td0[k]; }
        for (uint32_t k = tid; k < 64; k += blockDim.x) {
            L->sb[k] = ((const uint32_t *)T->sbox)[k];
            L->isb[k] = ((const uint32_t *)T->inv_sbox)[k];
        }
    }
    if (tid == 0) {
        uint32_t skip = 0u;
        if (stop_on_first) {
            const uint32_t off = blockIdx.x * blockDim.x * per;
            skip = e.start + off > lowest_known(e, R) ? 1u : 0u;
            if (skip && COUNT) {
                const uint32_t n = e.count - off < blockDim.x * per ? e.count - off : blockDim.x * per;
                atomicAdd(&R->skipped, (unsigned long long)n);
            }
        }
        *flag = skip;
    }
    __syncthreads();
    return *flag == 0;
}

/* ------------------------------------------------------------------ slot -> message */
/* BE message words of `len` candidate bytes (LE-packed) placed after `pre` bytes already in m[],
 * pre a multiple of 4 and <= 16, with the 0x80 terminator.  Static indices only.  A candidate that fills its whole
 * 64-byte slot (Office: 32 UTF-16 units; ODF: 64 bytes) has its terminator in the word after the slot (round 5: until
 * then it was dropped, and such a password was never found). */
template <int PREW>
DEVI void be_append(uint32_t m[32], const cand &c) {
#pragma unroll
    for (int j = 0; j < DPRF_SLOT_WORDS; j++)
        m[PREW + j] = bswap32((c.w[j] & le_keep_mask(j, c.len)) | le_pad80(j, c.len));
#pragma unroll
    for (int j = PREW + DPRF_SLOT_WORDS; j < 32; j++) m[j] = 0;
    m[PREW + DPRF_SLOT_WORDS] = c.len == 4u * DPRF_SLOT_WORDS ? 0x80000000u : 0u;
}

#define GRID(n, b) dim3(((n) + (b) - 1) / (b))
#endif
