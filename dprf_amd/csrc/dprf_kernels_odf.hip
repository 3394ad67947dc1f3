/* dprf_kernels_odf.hip -- ODF 1.0 / 1.1 password verification (Blowfish-CFB, SHA-1; include/dprf.h "ODF 1.0/1.1"),
 * two launches per batch as k_odt_kdf + k_odt_check:
 *   k_odf_bf_kdf<MODE>   sk = SHA1(pw); key = PBKDF2-HMAC-SHA1(sk, salt, iterations, 16): one output block, the
 *                        iteration count a kernel argument; leaves the 16-byte Blowfish key of every candidate in HBM
 *   k_odf_bf_check       the Blowfish key schedule over the candidate's own 4 KiB of S-boxes in LDS, the 128 block
 *                        encryptions of CFB decryption, SHA-1 over the 1024 plaintext bytes, all five words compared
 * No reference verifier exists for this format: the definition is pinned by tests/odf_legacy_model.py, whose Blowfish
 * is checked against libcrypto (tests/test_odf_legacy_model.py).
 *
 * A translation unit of its own: the other kernel objects keep their machine code.  The candidate source and the block
 * prologue are dprf_cand.h's.
 */
#include "dev_crypto.h"
#include "dprf_params.h"
#include "dprf_launch.h"
#include "dprf_hits.h"
#include "dprf_cand.h"
#include "blowfish_init.h"

/* ================================================================== KDF */
/* k_odt_kdf's loop with one output block: the same two sha1_compress_pre per iteration, so the same registers and
 * waves per SIMD */
#ifndef ODF_KDF_WAVES
#define ODF_KDF_WAVES 5
#endif
#define ODF_KDF_THREADS 256
template <int MODE>
__global__ void __launch_bounds__(ODF_KDF_THREADS, ODF_KDF_WAVES)
k_odf_bf_kdf(dprf_enum e, dprf_odf_params p, dprf_results *R, uint32_t stop_on_first, uint32_t *keys) {
    __shared__ uint8_t cs[256];
    __shared__ uint32_t flag;
    /* the charset is staged here, not by the prologue: in the prologue the same loop gets another schedule */
    for (uint32_t k = threadIdx.x; k < 64; k += blockDim.x) ((uint32_t *)cs)[k] = ((const uint32_t *)e.charset)[k];
    if (!block_prologue<false, false, false>(e, nullptr, R, stop_on_first, cs, nullptr, &flag)) return;
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= e.count) return;
    /* start key = SHA1(password): one block up to 55 bytes, two from 56; a candidate that fills its 64-byte slot has
     * its 0x80 in the first word of the second block */
    uint32_t sk[5];
    {
        cand c;
        get_candidate<MODE, false>(e, cs, g, c);
        uint32_t b0[16], b1[16];
#pragma unroll
        for (int j = 0; j < DPRF_SLOT_WORDS; j++) {
            b0[j] = bswap32((c.w[j] & le_keep_mask(j, c.len)) | le_pad80(j, c.len));
            b1[j] = 0u;
        }
        const bool two = c.len > 55u;
        b1[0] = c.len == 4u * DPRF_SLOT_WORDS ? 0x80000000u : 0u;
        if (!two) b0[15] = c.len * 8u;
        b1[15] = c.len * 8u;
        sha1_iv(sk);
        sha1_compress(sk, b0);
        if (two) sha1_compress(sk, b1);
    }
    /* PBKDF2-HMAC-SHA1(sk, salt, iterations, 16): the HMAC key is the 20-byte start key, so five pad words carry it */
    uint32_t ist[5], ost[5];
    {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = 0x36363636u ^ (j < 5 ? sk[j] : 0u);
        sha1_iv(ist); sha1_compress(ist, w);
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = 0x5c5c5c5cu ^ (j < 5 ? sk[j] : 0u);
        sha1_iv(ost); sha1_compress(ost, w);
    }
    const sha1_pre_t ipre = sha1_pre(ist), opre = sha1_pre(ost);
    uint32_t u[5], t[4];
    {
        /* both messages are 20 bytes: salt | INT(1), then the inner digest */
        const uint32_t m[5] = {p.salt[0], p.salt[1], p.salt[2], p.salt[3], 1u};
        uint32_t s[5];
        sha1_compress_pre(ist, ipre, m, s);
        sha1_compress_pre(ost, opre, s, u);
    }
    t[0] = u[0]; t[1] = u[1]; t[2] = u[2]; t[3] = u[3];
    for (uint32_t it = 1; it < p.iterations; it++) {
        uint32_t s[5];
        sha1_compress_pre(ist, ipre, u, s);
        sha1_compress_pre(ost, opre, s, u);
        /* two-input ops of the loop in 8-byte encodings (dev_crypto.h xor2_e64) */
        t[0] = xor2_e64(t[0], u[0]); t[1] = xor2_e64(t[1], u[1]); t[2] = xor2_e64(t[2], u[2]); t[3] = xor2_e64(t[3], u[3]);
    }
    /* the key bytes are the first 16 of T_1: as BE words they are Blowfish's key words as they stand */
#pragma unroll
    for (int k = 0; k < 4; k++) keys[(size_t)k * e.count + g] = t[k];
}

/* ================================================================== Blowfish check */
/* One candidate per lane, its four S-boxes (1,024 words) in LDS, P (18 words) in registers.  A CU's 160 KiB hold the
 * boxes of at most 39 candidates; a workgroup is ODF_BF_CANDS = 32 lanes with 128 KiB, one per CU.  Word j of lane l's
 * boxes is bf_box[j * 32 + l]: a ds_read_b32 of 32 lanes banks by (address / 4) mod 32, so whatever the 32 data-
 * dependent indices j are, the lanes fall on 32 distinct banks -- no lookup ever conflicts, and no lane touches another
 * lane's column, so the kernel has no barrier after its prologue.
 *
 * The key schedule is 521 block encryptions in a chain (each starts from the last one's output and reads the
 * subkeys the earlier ones replaced): 8,336 Feistel rounds, each waiting for its four lookups.  The 128 encryptions of
 * CFB decryption have constant inputs (iv and ciphertext) and are independent: they run eight at a time, one SHA-1
 * message block's worth, so that their lookups overlap. */
#define ODF_BF_CANDS 32
/* The KDF kernel's blocks are whole multiples of the check kernel's and it looks at the lowest hit earlier, so every
 * candidate it skips the check kernel skips too: no check block reads a key that was not written. */
static_assert(ODF_KDF_THREADS % ODF_BF_CANDS == 0, "a KDF block is whole check blocks (block_prologue)");
__shared__ uint32_t bf_box[1024 * ODF_BF_CANDS];
__device__ const uint32_t bf_init[BF_INIT_WORDS] = BF_INIT_TABLE;

namespace {
/* F(x) = ((S0[x >> 24] + S1[x >> 16 & 255]) ^ S2[x >> 8 & 255]) + S3[x & 255] over the lane's column */
DEVI uint32_t bf_f(uint32_t lane, uint32_t x) {
    const uint32_t a = bf_box[lane + ((x >> 24) << 5)];
    const uint32_t b = bf_box[lane + ((256u + ((x >> 16) & 255u)) << 5)];
    const uint32_t c = bf_box[lane + ((512u + ((x >> 8) & 255u)) << 5)];
    const uint32_t d = bf_box[lane + ((768u + (x & 255u)) << 5)];
    return ((a + b) ^ c) + d;
}
/* N independent block encryptions, round by round */
template <int N>
DEVI void bf_encrypt(const uint32_t (&P)[18], uint32_t lane, uint32_t (&l)[N], uint32_t (&r)[N]) {
#pragma unroll
    for (int q = 0; q < N; q++) l[q] ^= P[0];
#pragma unroll
    for (int i = 1; i <= 16; i += 2) {
#pragma unroll
        for (int q = 0; q < N; q++) r[q] = xor3(r[q], bf_f(lane, l[q]), P[i]);
#pragma unroll
        for (int q = 0; q < N; q++) l[q] = xor3(l[q], bf_f(lane, r[q]), P[i + 1]);
    }
#pragma unroll
    for (int q = 0; q < N; q++) {
        const uint32_t t = r[q] ^ P[17];
        r[q] = l[q];
        l[q] = t;
    }
}
}  // namespace

__global__ void __launch_bounds__(ODF_BF_CANDS)
k_odf_bf_check(dprf_enum e, dprf_odf_params p, dprf_results *R, uint32_t cap, uint32_t stop_on_first,
               const uint32_t *keys) {
    __shared__ uint32_t flag;
    if (!block_prologue<false, true, false>(e, nullptr, R, stop_on_first, nullptr, nullptr, &flag)) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t g = blockIdx.x * blockDim.x + lane;
    if (lane >= ODF_BF_CANDS || g >= e.count) return;
    /* the subkeys start as the digits of pi; the key's four words are XORed over P cyclically */
    uint32_t P[18];
    {
        uint32_t key[4];
#pragma unroll
        for (int k = 0; k < 4; k++) key[k] = keys[(size_t)k * e.count + g];
#pragma unroll
        for (int i = 0; i < 18; i++) P[i] = bf_init[i] ^ key[i & 3];
    }
#pragma unroll 8
    for (uint32_t j = 0; j < 1024u; j++) bf_box[lane + (j << 5)] = bf_init[18 + j];
    /* 521 encryptions of the running block replace P, then the boxes, pair by pair */
    uint32_t l[1] = {0u}, r[1] = {0u};
#pragma unroll
    for (int i = 0; i < 18; i += 2) {
        bf_encrypt<1>(P, lane, l, r);
        P[i] = l[0];
        P[i + 1] = r[0];
    }
#pragma unroll 1
    for (uint32_t j = 0; j < 1024u; j += 2) {
        bf_encrypt<1>(P, lane, l, r);
        bf_box[lane + (j << 5)] = l[0];
        bf_box[lane + ((j + 1u) << 5)] = r[0];
    }
    /* CFB decryption: pt_i = ct_i ^ E(ct_(i-1)), ct_(-1) = iv, hashed as it is produced */
    uint32_t st[5];
    sha1_iv(st);
#pragma unroll 1
    for (uint32_t b = 0; b < DPRF_ODF_CONTENT_WORDS / 16; b++) {
        const uint32_t *x = p.x + 16u * b;
        uint32_t cl[8], cr[8], w[16];
#pragma unroll
        for (int q = 0; q < 8; q++) { cl[q] = x[2 * q]; cr[q] = x[2 * q + 1]; }
        bf_encrypt<8>(P, lane, cl, cr);
#pragma unroll
        for (int q = 0; q < 8; q++) { w[2 * q] = cl[q] ^ x[2 * q + 2]; w[2 * q + 1] = cr[q] ^ x[2 * q + 3]; }
        sha1_compress(st, w);
    }
    {
        uint32_t w[16] = {0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4u * DPRF_ODF_CONTENT_WORDS * 8u};
        sha1_compress(st, w);
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 5; k++) ok = ok && st[k] == p.checksum[k];
    if (ok) report_hit(e, R, e.start + g, cap, stop_on_first);
}

/* ------------------------------------------------------------------ launcher */
hipError_t launch_odf(const dprf_enum &e, const dprf_odf_params &p, dprf_results *R, uint32_t cap, uint32_t stop,
                      hipStream_t s_kdf, hipStream_t s_check, uint32_t *keys, hipEvent_t mid) {
    /* the host refuses candidates longer than a slot: no long-list mode */
    if (e.mode > 1u || p.iterations == 0u || p.x == nullptr || (s_check != s_kdf && !mid)) return hipErrorInvalidValue;
    const dim3 grid = GRID(e.count, ODF_KDF_THREADS), block(ODF_KDF_THREADS);
    if (e.mode == 0) hipLaunchKernelGGL(k_odf_bf_kdf<0>, grid, block, 0, s_kdf, e, p, R, stop, keys);
    else hipLaunchKernelGGL(k_odf_bf_kdf<1>, grid, block, 0, s_kdf, e, p, R, stop, keys);
    if (mid) (void)hipEventRecord(mid, s_kdf);
    if (s_check != s_kdf) {
        const hipError_t r = hipStreamWaitEvent(s_check, mid, 0);
        if (r != hipSuccess) return r;
    }
    hipLaunchKernelGGL(k_odf_bf_check, GRID(e.count, ODF_BF_CANDS), dim3(ODF_BF_CANDS), 0, s_check, e, p, R, cap, stop, keys);
    return hipGetLastError();
}
