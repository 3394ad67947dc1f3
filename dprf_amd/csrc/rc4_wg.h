/* rc4_wg.h -- the two-wave RC4 workgroup of k_pdf_r24 (dprf_kernels.hip), device side.  Requires rc4_dev.h,
 * dprf_params.h, dprf_hits.h and dev_crypto.h (bswap32).  k_pdf_r24_owner and k_oldoffice (dprf_kernels_oldoffice.hip) have the same frame
 * written out: built on this header each measured below its rate (HISTORY.md), so a change to the protocol here is due
 * in both of them too.
 *
 * One workgroup = one RC4 wave (threads 0-63) + one key wave (threads 64-127) over NBAT batches of 64 candidates.  The
 * RC4 wave owns the workgroup's 16 KiB S-box area S (rc4_dev.h, one 256-byte box per lane) and only runs KSAs and
 * PRGAs; the key wave hashes.  The waves swap per-lane words through S while no box is live in it, between a barrier
 * after the last S-box access and one after the writes (rc4_wg_put / rc4_wg_get).  The why and the measurements are at
 * k_pdf_r24.  Everything here is inlined into the kernel that uses it.
 */
#ifndef DPRF_RC4_WG_H
#define DPRF_RC4_WG_H
#include "rc4_dev.h"

/* The workgroup's share of the launch: candidates base + 64 b + lane for b in [0, nb), nb >= 1 (the grid is
 * ceil(count / (64 * NBAT))); the last batch may be partial */
struct rc4_wg {
    uint32_t base, nb, lane;
};
template <uint32_t NBAT>
DEVI rc4_wg rc4_wg_geometry(const dprf_enum &e) {
    static_assert(NBAT % 2 == 0, "block_prologue counts NBAT / 2 candidates per thread of the 128-thread block");
    rc4_wg w;
    w.base = blockIdx.x * (64u * NBAT);
    const uint32_t left = e.count - w.base;
    w.nb = left >= 64u * NBAT ? (uint32_t)NBAT : (left + 63u) / 64u;
    /* threadIdx.x & 63, read as the wave's own lane count (128 threads = two waves of 64): written the first way
     * k_pdf_r24<1,3,16> takes one VGPR more than it had with the frame written out in the kernel */
    w.lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    return w;
}
/* Candidate of this lane in batch b for a hashing wave: clamped to the launch's last one (its result is never
 * reported: the RC4 wave tests the unclamped index) */
DEVI uint32_t rc4_wg_cand(const dprf_enum &e, const rc4_wg &w, uint32_t b) {
    const uint32_t g0 = w.base + 64u * b + w.lane;
    return g0 < e.count ? g0 : e.count - 1;
}

/* [N][64] words of a lane through the exchange area at word offset OFF of S */
template <int N, int OFF = 0>
DEVI void rc4_wg_put(uint8_t *S, uint32_t lane, const uint32_t (&v)[N]) {
    uint32_t *x = (uint32_t *)S + OFF;
#pragma unroll
    for (int q = 0; q < N; q++) x[64 * q + lane] = v[q];
}
template <int N, int OFF = 0>
DEVI void rc4_wg_get(const uint8_t *S, uint32_t lane, uint32_t (&v)[N]) {
    const uint32_t *x = (const uint32_t *)S + OFF;
#pragma unroll
    for (int q = 0; q < N; q++) v[q] = x[64 * q + lane];
}

/* The lane index recomputed (v_mbcnt), opaque so LLVM cannot hoist base + lane out of the batch loop: a register holding
 * it across the KSAs was the one value k_pdf_r24 spilled to scratch */
DEVI uint32_t rc4_wg_lane_id() {
    uint32_t lid;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lid));
    return lid;
}

/* RC4 wave: the asm KSA needs the S-box area at an LDS address with zero low 16 bits (rc4_ksa_asm); S is the kernel's
 * first LDS object, at 0 -- checked, and a launch that ever breaks it fails loudly instead of computing wrong: bit
 * `err` of dprf_results.pad_ is raised, the key wave's `barriers` barriers are kept and false is returned. */
DEVI bool rc4_wg_sbox_base(const uint8_t *S, bool ksa_asm, dprf_results *R, uint32_t lane, uint32_t err,
                           uint32_t barriers, uint32_t &sbase) {
    sbase = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(__attribute__((address_space(3))) const uint8_t *)S);
    if (ksa_asm && (sbase & 0xffffu) != 0u) {
        if (lane == 0) atomicOr(&R->pad_, err);
        for (uint32_t k = 0; k < barriers; k++) __syncthreads();
        return false;
    }
    return true;
}

/* The plain two-barrier protocol: the key wave runs key(g, k) -- the RC4 key of candidate g into k[4] -- for batch
 * b + 1 while the RC4 wave runs stage(w, sbase, b, k) on batch b with lane `w.lane`'s key; the keys change hands
 * through S between two barriers at each batch boundary.  PRIO: the RC4 wave's issue priority (s_setprio). */
template <uint32_t NBAT, int PRIO, class Key, class Stage>
DEVI void rc4_wg_run(const dprf_enum &e, uint8_t *S, bool ksa_asm, dprf_results *R, uint32_t err, Key key,
                     Stage stage) {
    const rc4_wg w = rc4_wg_geometry<NBAT>(e);
    uint32_t k[4];
    if (threadIdx.x >= 64u) {
        /* key wave */
        key(rc4_wg_cand(e, w, 0u), k);
#pragma unroll 1
        for (uint32_t b = 0; b < w.nb; b++) {
            __syncthreads();                              /* the RC4 wave is done with batch b-1's S-box */
            rc4_wg_put<4>(S, w.lane, k);
            __syncthreads();                              /* batch b's keys are in LDS */
            if (b + 1u < w.nb) key(rc4_wg_cand(e, w, b + 1u), k);
        }
        return;
    }
    /* RC4 wave */
    __builtin_amdgcn_s_setprio(PRIO);
    uint32_t sbase;
    if (!rc4_wg_sbox_base(S, ksa_asm, R, w.lane, err, 2u * w.nb, sbase)) return;
#pragma unroll 1
    for (uint32_t b = 0; b < w.nb; b++) {
        __syncthreads();
        __syncthreads();
        rc4_wg_get<4>(S, w.lane, k);
        stage(w, sbase, b, k);
    }
}

/* LDS of a key-search workgroup: the S-box area first (LDS address 0: rc4_wg_sbox_base), then block_prologue's skip
 * flag -- 16,400 B, 9 workgroups per CU */
struct key40_lds {
    uint8_t S[RC4_WAVE_BYTES];
    uint32_t flag[4];
};
/* 40-bit key search (include/dprf.h): key index i stands for its five bytes written big-endian, b0 = i >> 32 first.
 * The LE key words of b0..b4, zero-extended to 16 bytes */
DEVI void rc4_wg_key40(uint64_t i, uint32_t k[4]) {
    k[0] = bswap32((uint32_t)(i >> 8));
    k[1] = (uint32_t)i & 0xffu;
    k[2] = 0u;
    k[3] = 0u;
}

/* The frame without a key wave, for a 64-thread workgroup whose RC4 keys need no hashing (the 40-bit key search: the
 * key is the candidate index): stage(w, sbase, b) on batch b, no barrier and no exchange.  The geometry is the same,
 * so block_prologue counts NBAT candidates per thread of the 64-thread block. */
template <uint32_t NBAT, class Stage>
DEVI void rc4_wg_run1(const dprf_enum &e, uint8_t *S, bool ksa_asm, dprf_results *R, uint32_t err, Stage stage) {
    const rc4_wg w = rc4_wg_geometry<NBAT>(e);
    uint32_t sbase;
    if (!rc4_wg_sbox_base(S, ksa_asm, R, w.lane, err, 0u, sbase)) return;
#pragma unroll 1
    for (uint32_t b = 0; b < w.nb; b++) stage(w, sbase, b);
}
#endif
