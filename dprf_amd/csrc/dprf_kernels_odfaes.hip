/* dprf_kernels_odfaes.hip -- ODF 1.2 password verification at the manifest's PBKDF2 iteration count (AES-256-CBC,
 * SHA-256; include/dprf.h "ODF 1.2 at the manifest's iteration count"), two launches per batch:
 *   k_odf_aes_kdf<MODE>  sk = SHA256(pw); key = PBKDF2-HMAC-SHA1(sk, salt, iterations, 32): two output blocks, the
 *                        iteration count a kernel argument; leaves the 32-byte AES-256 key of every candidate in HBM,
 *                        in the column layout k_odt_check reads
 *   k_odt_check          dprf_kernels.hip's, launched as it stands: AES-256-CBC over the stream's 1024 bytes, SHA-256,
 *                        all eight checksum words compared
 * k_odt_kdf (dprf_kernels.hip) is this KDF with the count fixed at 1024, the reference verifier's constant
 * (odt_password_verifier.c:85); at that count the two agree on every candidate (tests/test_odf12_iter_gpu.py).
 *
 * A translation unit of its own: the ODF 1.2 object that bench.py measures and the ODF 1.0 / 1.1 object keep their
 * machine code.  The candidate source and the block prologue are dprf_cand.h's.
 */
#include "dev_crypto.h"
#include "dprf_params.h"
#include "dprf_launch.h"
#include "dprf_hits.h"
#include "dprf_cand.h"

/* ================================================================== KDF */
/* k_odt_kdf's loop body with a run-time trip count: the same two sha1_compress_pre per iteration, so the same
 * registers (96 VGPRs) and waves per SIMD.  The two output blocks run one after the other, as there. */
#ifndef ODF_AES_KDF_WAVES
#define ODF_AES_KDF_WAVES 5
#endif
#define ODF_AES_KDF_THREADS 256
template <int MODE>
__global__ void __launch_bounds__(ODF_AES_KDF_THREADS, ODF_AES_KDF_WAVES)
k_odf_aes_kdf(dprf_enum e, dprf_odf_aes_params p, dprf_results *R, uint32_t stop_on_first, uint32_t *keys) {
    __shared__ uint8_t cs[256];
    __shared__ uint32_t flag;
    if (!block_prologue<false, false>(e, nullptr, R, stop_on_first, cs, nullptr, &flag)) return;
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.count) return;
    /* start key = SHA256(password): one block up to 55 bytes, two from 56; a candidate that fills its 64-byte slot has
     * its 0x80 in the first word of the second block (be_append) */
    uint32_t sk[8];
    if constexpr (MODE == 2) {
        /* long list: from k_long_prehash, in the lane's own key column */
#pragma unroll
        for (int k = 0; k < 8; k++) sk[k] = keys[(size_t)k * e.count + g];
    } else {
        cand c;
        get_candidate<MODE, false>(e, cs, g, c);
        uint32_t m[32], b0[16], b1[16];
        be_append<0>(m, c);
#pragma unroll
        for (int j = 0; j < 16; j++) { b0[j] = m[j]; b1[j] = m[16 + j]; }
        const bool two = c.len > 55u;
        if (!two) b0[15] = c.len * 8u;
        b1[15] = c.len * 8u;
        sha256_iv(sk);
        sha256_compress(sk, b0);
        if (two) sha256_compress(sk, b1);
    }
    /* the key column for the stores; long list: hidden from LLVM, which otherwise keeps the loads' eight addresses
     * live through PBKDF2 for the stores (k_odt_kdf) */
    uint32_t gk = g;
    if constexpr (MODE == 2) asm volatile("" : "+v"(gk));
    /* PBKDF2-HMAC-SHA1(sk, salt, iterations, 32): the HMAC key is the 32-byte start key, so eight pad words carry it;
     * ipad/opad midstates and their message-independent round parts once per candidate */
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
    const sha1_pre_t ipre = sha1_pre(ist), opre = sha1_pre(ost);
#pragma unroll
    for (int blkno = 1; blkno <= 2; blkno++) {
        uint32_t u[5], t[5];
        {
            /* both messages are 20 bytes: salt | INT(blkno), then the inner digest */
            const uint32_t m[5] = {p.salt[0], p.salt[1], p.salt[2], p.salt[3], (uint32_t)blkno};
            uint32_t s[5];
            sha1_compress_pre(ist, ipre, m, s);
            sha1_compress_pre(ost, opre, s, u);
        }
        t[0] = u[0]; t[1] = u[1]; t[2] = u[2]; t[3] = u[3]; t[4] = u[4];
        for (uint32_t it = 1; it < p.iterations; it++) {
            uint32_t s[5];
            sha1_compress_pre(ist, ipre, u, s);
            sha1_compress_pre(ost, opre, s, u);
            /* two-input ops of the loop in 8-byte encodings (dev_crypto.h xor2_e64) */
            t[0] = xor2_e64(t[0], u[0]); t[1] = xor2_e64(t[1], u[1]); t[2] = xor2_e64(t[2], u[2]);
            t[3] = xor2_e64(t[3], u[3]); t[4] = xor2_e64(t[4], u[4]);
        }
        /* each block's key words go out as soon as they are known: T_1's five, then the first three of T_2 */
        if (blkno == 1) {
#pragma unroll
            for (int k = 0; k < 5; k++) keys[(size_t)k * e.count + gk] = t[k];
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) keys[(size_t)(5 + k) * e.count + gk] = t[k];
        }
    }
}

/* ================================================================== the check, and the launcher */
/* k_odt_check is defined in dprf_kernels.hip (the ODF 1.2 object); declared here, the launch below goes through that
 * object's host stub.  Its block size is its launch bound there: a launch with more threads fails with an error. */
#define ODF_AES_CHECK_THREADS 512
__global__ void k_odt_check(dprf_enum e, dprf_odt_params p, const dprf_aes_tables *T, dprf_results *R, uint32_t cap,
                            uint32_t stop_on_first, const uint32_t *keys);

hipError_t launch_odf_aes(const dprf_enum &e, const dprf_odf_aes_params &kp, const dprf_odt_params &p,
                          const dprf_aes_tables *T, dprf_results *R, uint32_t cap, uint32_t stop, hipStream_t s,
                          uint32_t *keys, hipEvent_t mid) {
    const dim3 grid = GRID(e.count, ODF_AES_KDF_THREADS), block(ODF_AES_KDF_THREADS);
    if (e.mode == 0) hipLaunchKernelGGL(k_odf_aes_kdf<0>, grid, block, 0, s, e, kp, R, stop, keys);
    else if (e.mode == 1) hipLaunchKernelGGL(k_odf_aes_kdf<1>, grid, block, 0, s, e, kp, R, stop, keys);
    else hipLaunchKernelGGL(k_odf_aes_kdf<2>, grid, block, 0, s, e, kp, R, stop, keys);
    if (mid) (void)hipEventRecord(mid, s);
    hipLaunchKernelGGL(k_odt_check, GRID(e.count, ODF_AES_CHECK_THREADS), dim3(ODF_AES_CHECK_THREADS), 0, s, e, p, T, R,
                       cap, stop, (const uint32_t *)keys);
    return hipGetLastError();
}
