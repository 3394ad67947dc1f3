/* dprf_kernels_hybrid.hip -- hybrid windows (dprf_search_hybrid): a word of the context's table with a mask around it.
 *
 * k_spell_hybrid is k_spell_mask (dprf_kernels.hip) with one more digit at the most significant end of the mixed
 * radix: candidate g of the chunk takes its mask digits as there -- the chunk start's digits from the arguments, g
 * added with carries, the last position fastest -- and what the digit loop leaves over after the last position,
 * rem + carry, is the word increment: word a.w0 + rem + carry of the table, spelled before mask position a.word_at.
 * The host's window check keeps every live lane's word below a.nwords.
 *
 * The table stays in HBM from dprf_ctx_set_words on (dprf_params.h): converted bytes packed back to back, u32 byte
 * offsets.  Word indices do not decrease with g, so a block's 256 candidates use one contiguous run of at most 256
 * words, from lane 0's word to the last live lane's: at most 16 KB of bytes.  Those two lanes publish the run's ends,
 * the block copies the run's offsets and bytes into LDS with consecutive u32 loads, and every lane then spells its
 * word from LDS -- no lane gathers bytes from global memory.  LDS per block: the mask kernel's 27,264 B (records 512,
 * pool 8,192 + 2,048, tile 16,512) + offsets 1,028 + run 16,388 + the two ends 8 = 44,688 B (44,704 as the compiler
 * lays it out), so three blocks (12 waves) fit a CU's 160 KB.  Tile layout, trunc rule and read-out are
 * k_spell_symbols', so the list-mode kernels of every family verify the slots unchanged.
 *
 * An object of its own (Makefile), so the other kernel objects keep their machine code.
 */
#include "dev_crypto.h"
#include "dprf_params.h"
#include "dprf_launch.h"

DEVI uint32_t hyb_fastdiv(uint32_t n, uint32_t m, uint32_t s) {
    const uint32_t t = __umulhi(n, m);
    return (t + ((n - t) >> 1)) >> s;
}

/* One position of the mask, going from the last to the first: takes the position's digit out of rem / carry and
 * returns the pool entry of its symbol (k_spell_mask's loop body). */
DEVI uint32_t hyb_digit(const uint32_t *rec, int p, uint32_t &rem, uint32_t &carry) {
    const uint32_t r0 = rec[4 * p], radix = r0 & 0xffffu;
    const uint32_t q = radix == 1u ? rem : hyb_fastdiv(rem, rec[4 * p + 1], rec[4 * p + 2]);
    uint32_t d = (r0 >> 16) + (rem - q * radix) + carry;
    carry = d >= radix ? 1u : 0u;
    d -= carry ? radix : 0u;
    rem = q;
    return (rec[4 * p + 3] + d) & (DPRF_MASK_POOL - 1u);
}

__global__ void __launch_bounds__(256)
k_spell_hybrid(dprf_hybrid_args a, const uint32_t *tab, const uint32_t *wblob, const uint32_t *woff, uint32_t *slots,
               uint8_t *lens) {
    constexpr uint32_t ST = 258;
    __shared__ uint32_t rec[DPRF_MASK_POOL_AT];
    __shared__ uint32_t pw[DPRF_MASK_POOL];
    __shared__ uint32_t plw[DPRF_MASK_POOL / 4];
    __shared__ uint32_t tile[DPRF_SLOT_WORDS * ST];
    __shared__ uint32_t soff[DPRF_HYB_RUN + 1];
    __shared__ uint32_t run[DPRF_HYB_RUN_WORDS];
    __shared__ uint32_t ends[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t n = a.m.npos < DPRF_MAX_RANGE_LEN ? a.m.npos : DPRF_MAX_RANGE_LEN;
    const uint32_t np = a.m.npool < DPRF_MASK_POOL ? a.m.npool : DPRF_MASK_POOL;
    if (tid < DPRF_MASK_REC_WORDS * n) {
        uint32_t v = tab[tid];
        if ((tid & 3u) == 0u) {
            uint32_t sw = 0;
#pragma unroll
            for (uint32_t j = 0; j < DPRF_MAX_RANGE_LEN / 4; j++) sw = (tid >> 4) == j ? a.m.sdig[j] : sw;
            v |= ((sw >> (8u * ((tid >> 2) & 3u))) & 0xffu) << 16;
        }
        rec[tid] = v;
    }
    for (uint32_t k = tid; k < np; k += 256u) pw[k] = tab[DPRF_MASK_POOL_AT + k];
    for (uint32_t k = tid; k < (np + 3u) >> 2; k += 256u) plw[k] = tab[DPRF_MASK_LENS_AT + k];
#pragma unroll
    for (int j = 0; j < DPRF_SLOT_WORDS; j++) tile[j * ST + tid] = 0u;
    __syncthreads();
    const uint32_t base = blockIdx.x * 256u;
    const uint32_t g = base + tid;
    const bool live = g < a.m.count;
    const uint32_t lim = a.m.trunc < 4u * DPRF_SLOT_WORDS ? a.m.trunc : 4u * DPRF_SLOT_WORDS;
    const uint8_t *pl = (const uint8_t *)plw;
    /* first pass over the digits: the mask part's length, and the word index from what is left over */
    uint32_t mtotal = 0, w = 0;
    if (live) {
        uint32_t rem = g, carry = 0;
        for (int p = (int)n - 1; p >= 0; --p) mtotal += pl[hyb_digit(rec, p, rem, carry)];
        w = a.w0 + rem + carry;
        w = w < a.nwords ? w : a.nwords - 1u;
        const uint32_t left = a.m.count - base;                  /* live lanes of the block: 1..256 of them */
        if (tid == 0u) ends[0] = w;
        if (tid == (left < 256u ? left : 256u) - 1u) ends[1] = w;
    }
    __syncthreads();
    /* the run lane 0's word .. the last live lane's word: its nw + 1 offsets and its bytes, as whole u32 words from
     * the one that holds the run's first byte */
    const uint32_t wlo = ends[0];
    const uint32_t span = ends[1] >= wlo ? ends[1] - wlo + 1u : 1u;
    const uint32_t nw = span < DPRF_HYB_RUN ? span : DPRF_HYB_RUN;
    for (uint32_t k = tid; k <= nw; k += 256u) soff[k] = woff[wlo + k];
    const uint32_t b0 = woff[wlo], b1 = woff[wlo + nw];
    const uint32_t a0 = b0 >> 2;                                 /* first u32 of the blob the run touches */
    uint32_t nu = b1 > 4u * a0 ? (b1 - 4u * a0 + 3u) >> 2 : 0u;
    nu = nu < DPRF_HYB_RUN_WORDS ? nu : DPRF_HYB_RUN_WORDS;
    nu = a0 < a.bwords ? (nu < a.bwords - a0 ? nu : a.bwords - a0) : 0u;
    for (uint32_t k = tid; k < nu; k += 256u) run[k] = wblob[a0 + k];
    __syncthreads();
    if (live) {
        const uint32_t wi = w - wlo < DPRF_HYB_RUN ? w - wlo : DPRF_HYB_RUN - 1u;
        const uint32_t o0 = soff[wi], o1 = soff[wi + 1u];
        uint32_t wl = o1 > o0 ? o1 - o0 : 0u;
        wl = wl < 4u * DPRF_SLOT_WORDS ? wl : 4u * DPRF_SLOT_WORDS;
        /* the word's first byte in run[]; kept inside run[] whatever the offsets say */
        uint32_t src = o0 - 4u * a0;
        src = src <= 4u * DPRF_HYB_RUN_WORDS - 4u * DPRF_SLOT_WORDS ? src : 0u;
        const uint8_t *rb = (const uint8_t *)run;
        uint8_t *tb = (uint8_t *)tile;
        const uint32_t total = mtotal + wl;
        /* second pass, right to left from the end (k_spell_symbols): the positions behind the word, the word, the
         * positions before it */
        uint32_t rem = g, carry = 0, pos = total;
        for (int p = (int)n - 1; p >= -1; --p) {
            if ((uint32_t)(p + 1) == a.word_at) {
                pos -= wl;
                for (uint32_t j = 0; j < wl; j++)
                    if (pos + j < lim) tb[4u * (((pos + j) >> 2) * ST + tid) + ((pos + j) & 3u)] = rb[src + j];
            }
            if (p < 0) break;
            const uint32_t en = hyb_digit(rec, p, rem, carry);
            const uint32_t k = pl[en], sy = pw[en];
            pos -= k;
            for (uint32_t j = 0; j < k; j++)
                if (pos + j < lim) tb[4u * (((pos + j) >> 2) * ST + tid) + ((pos + j) & 3u)] = (uint8_t)(sy >> (8u * j));
        }
        lens[g] = (uint8_t)(total < lim ? total : lim);
    }
    __syncthreads();
    uint4 *out = (uint4 *)(slots + (size_t)base * DPRF_SLOT_WORDS);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t u = 256u * q + tid, sl = u >> 2, w0 = 4u * (u & 3u);
        if (base + sl < a.m.count)
            out[u] = make_uint4(tile[w0 * ST + sl], tile[(w0 + 1) * ST + sl], tile[(w0 + 2) * ST + sl],
                                tile[(w0 + 3) * ST + sl]);
    }
}

hipError_t launch_spell_hybrid(const dprf_hybrid_args &a, const uint32_t *tab, const uint32_t *wblob,
                               const uint32_t *woff, uint32_t *slots, uint8_t *lens, hipStream_t s) {
    hipLaunchKernelGGL(k_spell_hybrid, dim3((a.m.count + 255u) / 256u), dim3(256), 0, s, a, tab, wblob, woff, slots,
                       lens);
    return hipGetLastError();
}
