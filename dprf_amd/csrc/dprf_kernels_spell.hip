/* dprf_kernels_spell.hip -- the device spellers: index g of a chunk -> the candidate's bytes in a list slot, for the
 * list-mode kernels of every family to verify.  Five candidate sources, one block of 256 lanes per 256 candidates:
 *   k_spell_symbols  symbol windows (dprf_search_symbols)                   uniform radix over one symbol table
 *   k_spell_mask     mask windows (dprf_search_mask)                        a radix and a symbol list per position
 *   k_spell_hybrid   hybrid windows (dprf_search_hybrid)                    a word of the context's table in a mask
 *   k_spell_rules    rule windows (dprf_search_rules, dprf_spell_rules)     a rule of the call applied to a word
 *   k_spell_combine  combinator windows (dprf_search_combine, dprf_spell_combine)  a left word, then a right word
 * What they share is written once, here and in the helpers below.
 *
 * The slot tile.  A block's 256 slots sit in LDS as [word][slot] with a row stride of ST = 258 words; lane t owns
 * column t and assembles its candidate there byte by byte (col_byte).  258 rather than 256 so that the byte stores of
 * one word index and the 16-byte read-outs both spread over the banks.  The tile is cleared first (tile_clear), so
 * every byte a lane does not store is zero.
 *
 * The trunc rule.  Bytes at or past lim = min(trunc, 64) are never written (put_byte; PDF R2-R4 hash 32 bytes,
 * pdf...c:137): the slot stays zero there and lens[g] = min(total, lim), as dprf_verify_list packs a truncated
 * candidate.
 *
 * The read-out (read_out).  16-byte piece u = 256 q + tid of the block's 16 KB of slots is slot u / 4, words
 * 4 (u % 4) .., so every store instruction of the block writes 4 KB of consecutive memory; pieces of slots at or past
 * the chunk's count are not stored.
 *
 * The digits.  The chunk start's digits come from the host, g is added with carries, the last position fastest
 * (itertools.product order, brute_force.py:205), as range_candidate does it.  The mask kernels read a record per
 * position {radix | start digit << 16, fastdiv magic, shift, base into the pool} and the pool entry base + digit
 * (LE-packed symbol word, byte count), staged into LDS once per block (stage_mask, mask_digit): every lane of a wave
 * reads the same record (an LDS broadcast) and the radix-1 test is wave-uniform.  The digits are walked twice, once
 * for the candidate's length and once to store each symbol's bytes right to left from its end -- no digit array.
 *
 * The word run (stage_run, find_word).  The word table stays in HBM from dprf_ctx_set_words on (dprf_params.h):
 * converted bytes packed back to back, u32 byte offsets.  Word indices do not decrease with g, so a block's 256
 * candidates use one contiguous run of at most 256 words, from lane 0's word to the last live lane's: at most 16 KB of
 * bytes.  Those two lanes publish the run's ends, the block copies the run's nw + 1 offsets and its bytes -- whole u32
 * words from the one that holds the run's first byte -- into LDS with consecutive loads, and every lane then takes its
 * word from LDS: no lane gathers bytes from global memory.  The clamps: the run is at most DPRF_HYB_RUN words and
 * DPRF_HYB_RUN_WORDS u32 of bytes and ends inside the blob (bwords); a lane's word index is kept inside soff[], its
 * length is at most a slot and its first byte lies a slot or more before the end of run[], whatever the offsets say.
 * The host validates the tables, but memory safety here does not depend on that.
 *
 * LDS per block, as the compiler lays it out, and what fits a CU's 160 KB:
 *   k_spell_symbols  table 2,048 + tile 16,512                                      = 18,560 B   8 blocks
 *   k_spell_mask     records 512 + pool 8,192 + 2,048 + tile 16,512                 = 27,264 B   6 blocks (24 waves)
 *   k_spell_hybrid   the mask kernel's + offsets 1,028 + run 16,388 + ends 8        = 44,704 B   3 blocks (12 waves)
 *   k_spell_rules    two tiles 33,024 + offsets 1,028 + run 16,388 + ends 8         = 50,452 B   3 blocks (12 waves)
 *   k_spell_combine  tile 16,512 + left offsets 1,028 + run 16,388 + ends 8
 *                    + right entries 1,024 + run 16,388 (+ 28 alignment)              = 51,376 B   3 blocks (12 waves)
 * No kernel uses scratch (resource_gate.py).  k_spell_combine: 37 VGPRs.
 */
#include "dev_crypto.h"
#include "dprf_params.h"
#include "dprf_launch.h"

namespace {
constexpr uint32_t ST = 258;
constexpr uint32_t TW = DPRF_SLOT_WORDS * ST;                /* words of one tile */

/* The helpers take the kernels' LDS arrays by reference, as arrays: inlined, they address LDS as the kernel's own
 * code would.  A tile parameter is TW words or, for k_spell_rules, two tiles of which tile 0 is meant. */

/* byte `at` of lane tid's column, as a byte index into the tile */
DEVI uint32_t col_byte(uint32_t tid, uint32_t at) { return 4u * ((at >> 2) * ST + tid) + (at & 3u); }

DEVI void tile_clear(uint32_t (&tile)[TW], uint32_t tid) {
#pragma unroll
    for (int j = 0; j < DPRF_SLOT_WORDS; j++) tile[j * ST + tid] = 0u;
}

DEVI void put_byte(uint32_t (&tile)[TW], uint32_t tid, uint32_t at, uint32_t lim, uint32_t v) {
    if (at < lim) ((uint8_t *)tile)[col_byte(tid, at)] = (uint8_t)v;
}

/* the k bytes of the LE-packed symbol word sy at pos */
DEVI void put_symbol(uint32_t (&tile)[TW], uint32_t tid, uint32_t pos, uint32_t lim, uint32_t sy, uint32_t k) {
    for (uint32_t j = 0; j < k; j++) put_byte(tile, tid, pos + j, lim, sy >> (8u * j));
}

template <uint32_t N>
DEVI void read_out(const uint32_t (&tile)[N], uint32_t tid, uint32_t base, uint32_t count, uint32_t *slots) {
    uint4 *out = (uint4 *)(slots + (size_t)base * DPRF_SLOT_WORDS);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t u = 256u * q + tid, sl = u >> 2, w0 = 4u * (u & 3u);
        if (base + sl < count)
            out[u] = make_uint4(tile[w0 * ST + sl], tile[(w0 + 1) * ST + sl], tile[(w0 + 2) * ST + sl],
                                tile[(w0 + 3) * ST + sl]);
    }
}

/* The mask table into LDS: the records of the n positions, each with its start digit from a.sdig, and the pool. */
DEVI void stage_mask(const dprf_mask_args &a, const uint32_t *tab, uint32_t tid, uint32_t n,
                     uint32_t (&rec)[DPRF_MASK_POOL_AT], uint32_t (&pw)[DPRF_MASK_POOL],
                     uint32_t (&plw)[DPRF_MASK_POOL / 4]) {
    const uint32_t np = a.npool < DPRF_MASK_POOL ? a.npool : DPRF_MASK_POOL;
    if (tid < DPRF_MASK_REC_WORDS * n) {
        uint32_t v = tab[tid];
        if ((tid & 3u) == 0u) {
            /* position tid / 4: its start digit is byte (tid / 4) % 4 of a.sdig[tid / 16] (static indices only) */
            uint32_t sw = 0;
#pragma unroll
            for (uint32_t j = 0; j < DPRF_MAX_RANGE_LEN / 4; j++) sw = (tid >> 4) == j ? a.sdig[j] : sw;
            v |= ((sw >> (8u * ((tid >> 2) & 3u))) & 0xffu) << 16;
        }
        rec[tid] = v;
    }
    for (uint32_t k = tid; k < np; k += 256u) pw[k] = tab[DPRF_MASK_POOL_AT + k];
    for (uint32_t k = tid; k < (np + 3u) >> 2; k += 256u) plw[k] = tab[DPRF_MASK_LENS_AT + k];
}

/* One position of the mask, going from the last to the first: takes the position's digit out of rem / carry and
 * returns the pool entry of its symbol.  A literal takes no division: q = rem, digit 0, and a carry passes through. */
DEVI uint32_t mask_digit(const uint32_t (&rec)[DPRF_MASK_POOL_AT], int p, uint32_t &rem, uint32_t &carry) {
    const uint32_t r0 = rec[4 * p], radix = r0 & 0xffffu;
    const uint32_t q = radix == 1u ? rem : fastdiv(rem, rec[4 * p + 1], rec[4 * p + 2]);
    uint32_t d = (r0 >> 16) + (rem - q * radix) + carry;
    carry = d >= radix ? 1u : 0u;
    d -= carry ? radix : 0u;
    rem = q;
    return (rec[4 * p + 3] + d) & (DPRF_MASK_POOL - 1u);
}

struct word_run {
    uint32_t wlo;                                            /* the run's first word */
    uint32_t a0;                                             /* first u32 of the blob the run touches */
};

/* The block's word run into soff[] / run[], up to the barrier after which every lane may read them.  w is the live
 * lane's word, clamped to the table by the caller. */
DEVI word_run stage_run(bool live, uint32_t w, uint32_t tid, uint32_t base, uint32_t count, uint32_t bwords,
                        const uint32_t *wblob, const uint32_t *woff, uint32_t (&ends)[2],
                        uint32_t (&soff)[DPRF_HYB_RUN + 1], uint32_t (&run)[DPRF_HYB_RUN_WORDS]) {
    if (live) {
        const uint32_t left = count - base;                  /* live lanes of the block: 1..256 of them */
        if (tid == 0u) ends[0] = w;
        if (tid == (left < 256u ? left : 256u) - 1u) ends[1] = w;
    }
    __syncthreads();
    const uint32_t wlo = ends[0];
    const uint32_t span = ends[1] >= wlo ? ends[1] - wlo + 1u : 1u;
    const uint32_t nw = span < DPRF_HYB_RUN ? span : DPRF_HYB_RUN;
    for (uint32_t k = tid; k <= nw; k += 256u) soff[k] = woff[wlo + k];
    const uint32_t b0 = woff[wlo], b1 = woff[wlo + nw];
    const uint32_t a0 = b0 >> 2;
    uint32_t nu = b1 > 4u * a0 ? (b1 - 4u * a0 + 3u) >> 2 : 0u;
    nu = nu < DPRF_HYB_RUN_WORDS ? nu : DPRF_HYB_RUN_WORDS;
    nu = a0 < bwords ? (nu < bwords - a0 ? nu : bwords - a0) : 0u;
    for (uint32_t k = tid; k < nu; k += 256u) run[k] = wblob[a0 + k];
    __syncthreads();
    return {wlo, a0};
}

/* Word w of the staged run: returns its first byte in run[] and yields its length wl. */
DEVI uint32_t find_word(const word_run &r, uint32_t w, const uint32_t (&soff)[DPRF_HYB_RUN + 1], uint32_t &wl) {
    const uint32_t wi = w - r.wlo < DPRF_HYB_RUN ? w - r.wlo : DPRF_HYB_RUN - 1u;
    const uint32_t o0 = soff[wi], o1 = soff[wi + 1u];
    wl = o1 > o0 ? o1 - o0 : 0u;
    wl = wl < 4u * DPRF_SLOT_WORDS ? wl : 4u * DPRF_SLOT_WORDS;
    const uint32_t src = o0 - 4u * r.a0;
    return src <= 4u * DPRF_HYB_RUN_WORDS - 4u * DPRF_SLOT_WORDS ? src : 0u;
}
}  // namespace

/* ================================================================== symbol windows */
/* Range mode over a charset whose symbols take several bytes (a --charset with non-ASCII characters: one symbol per
 * character, its UTF-8 -- for Office its UTF-16LE -- bytes), in itertools.product order over the symbols.  Its own
 * digit step: one radix for every position, the start digits as bytes of the dprf_enum. */
__global__ void __launch_bounds__(256)
k_spell_symbols(dprf_enum e, const uint32_t *symtab, uint32_t trunc, uint32_t *slots, uint8_t *lens) {
    __shared__ uint32_t sym[256], syl[256];
    __shared__ uint32_t tile[TW];
    const uint32_t tid = threadIdx.x;
    sym[tid] = symtab[tid];
    syl[tid] = symtab[256 + tid];
    tile_clear(tile, tid);
    __syncthreads();
    const uint32_t g = blockIdx.x * 256u + tid;
    const uint32_t n = e.pwlen < DPRF_MAX_RANGE_LEN ? e.pwlen : DPRF_MAX_RANGE_LEN;
    const uint32_t lim = trunc < 4u * DPRF_SLOT_WORDS ? trunc : 4u * DPRF_SLOT_WORDS;
    if (g < e.count) {
        uint32_t total = 0;
        for (int pass = 0; pass < 2; pass++) {
            uint32_t rem = g, carry = 0, pos = total;
            for (int p = (int)n - 1; p >= 0; --p) {
                const uint32_t q = e.cslen == 1 ? rem : fastdiv(rem, e.div_m, e.div_s);
                uint32_t d = (uint32_t)e.sdig[p] + (rem - q * e.cslen) + carry;
                carry = d >= e.cslen ? 1u : 0u;
                d -= carry ? e.cslen : 0u;
                rem = q;
                const uint32_t k = syl[d];
                if (pass == 0) {
                    total += k;
                } else {
                    pos -= k;
                    put_symbol(tile, tid, pos, lim, sym[d], k);
                }
            }
        }
        lens[g] = (uint8_t)(total < lim ? total : lim);
    }
    __syncthreads();
    read_out(tile, tid, blockIdx.x * 256u, e.count, slots);
}

/* ================================================================== mask windows */
/* A table and a radix per position (dprf_search_mask: "?u?l?l?d", a literal is a position of one symbol), in
 * itertools.product order over the positions' symbol lists.  Lanes differ only in the pool entry and in the symbol's
 * byte count. */
__global__ void __launch_bounds__(256)
k_spell_mask(dprf_mask_args a, const uint32_t *tab, uint32_t *slots, uint8_t *lens) {
    __shared__ uint32_t rec[DPRF_MASK_POOL_AT];
    __shared__ uint32_t pw[DPRF_MASK_POOL];
    __shared__ uint32_t plw[DPRF_MASK_POOL / 4];
    __shared__ uint32_t tile[TW];
    const uint32_t tid = threadIdx.x;
    const uint32_t n = a.npos < DPRF_MAX_RANGE_LEN ? a.npos : DPRF_MAX_RANGE_LEN;
    stage_mask(a, tab, tid, n, rec, pw, plw);
    tile_clear(tile, tid);
    __syncthreads();
    const uint32_t g = blockIdx.x * 256u + tid;
    const uint32_t lim = a.trunc < 4u * DPRF_SLOT_WORDS ? a.trunc : 4u * DPRF_SLOT_WORDS;
    if (g < a.count) {
        const uint8_t *pl = (const uint8_t *)plw;
        uint32_t total = 0;
        for (int pass = 0; pass < 2; pass++) {
            uint32_t rem = g, carry = 0, pos = total;
            for (int p = (int)n - 1; p >= 0; --p) {
                const uint32_t en = mask_digit(rec, p, rem, carry);
                const uint32_t k = pl[en];
                if (pass == 0) {
                    total += k;
                } else {
                    pos -= k;
                    put_symbol(tile, tid, pos, lim, pw[en], k);
                }
            }
        }
        lens[g] = (uint8_t)(total < lim ? total : lim);
    }
    __syncthreads();
    read_out(tile, tid, blockIdx.x * 256u, a.count, slots);
}

/* ================================================================== hybrid windows */
/* k_spell_mask with one more digit at the most significant end of the mixed radix: what the digit loop leaves over
 * after the last position, rem + carry, is the word increment: word a.w0 + rem + carry of the table, spelled before
 * mask position a.word_at.  The host's window check keeps every live lane's word below a.nwords. */
__global__ void __launch_bounds__(256)
k_spell_hybrid(dprf_hybrid_args a, const uint32_t *tab, const uint32_t *wblob, const uint32_t *woff, uint32_t *slots,
               uint8_t *lens) {
    __shared__ uint32_t rec[DPRF_MASK_POOL_AT];
    __shared__ uint32_t pw[DPRF_MASK_POOL];
    __shared__ uint32_t plw[DPRF_MASK_POOL / 4];
    __shared__ uint32_t tile[TW];
    __shared__ uint32_t soff[DPRF_HYB_RUN + 1];
    __shared__ uint32_t run[DPRF_HYB_RUN_WORDS];
    __shared__ uint32_t ends[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t n = a.m.npos < DPRF_MAX_RANGE_LEN ? a.m.npos : DPRF_MAX_RANGE_LEN;
    stage_mask(a.m, tab, tid, n, rec, pw, plw);
    tile_clear(tile, tid);
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
        for (int p = (int)n - 1; p >= 0; --p) mtotal += pl[mask_digit(rec, p, rem, carry)];
        w = a.w0 + rem + carry;
        w = w < a.nwords ? w : a.nwords - 1u;
    }
    const word_run r = stage_run(live, w, tid, base, a.m.count, a.bwords, wblob, woff, ends, soff, run);
    if (live) {
        uint32_t wl;
        const uint32_t src = find_word(r, w, soff, wl);
        const uint8_t *rb = (const uint8_t *)run;
        const uint32_t total = mtotal + wl;
        /* second pass: the positions behind the word, the word, the positions before it */
        uint32_t rem = g, carry = 0, pos = total;
        for (int p = (int)n - 1; p >= -1; --p) {
            if ((uint32_t)(p + 1) == a.word_at) {
                pos -= wl;
                for (uint32_t j = 0; j < wl; j++) put_byte(tile, tid, pos + j, lim, rb[src + j]);
            }
            if (p < 0) break;
            const uint32_t en = mask_digit(rec, p, rem, carry);
            const uint32_t k = pl[en];
            pos -= k;
            put_symbol(tile, tid, pos, lim, pw[en], k);
        }
        lens[g] = (uint8_t)(total < lim ? total : lim);
    }
    __syncthreads();
    read_out(tile, tid, base, a.m.count, slots);
}

/* ================================================================== rule windows */
/* include/dprf.h "rule mode" defines the language.  Candidate g of the chunk is rule (a.r0 + g) % R applied to word
 * a.w0 + (a.r0 + g) / R: the chunk start's word and rule index travel in the arguments, the division is a
 * multiply-high with the host's magic (a.r0 + g < 2^32: chunks hold at most 2^26 candidates, R at most 2^20).  The
 * rule table -- one u32 per function, R + 1 offsets -- is uploaded once per call and read from global memory: small,
 * call-constant, served from L2.
 *
 * The interpreter indexes the candidate at run-time positions, so the working copy lives in LDS (a private array
 * would go to scratch): the lane's column of the tile, unit j of lane t in word (j * U / 4) * ST + t, which keeps a
 * wave's accesses to one position conflict-free.  U is the unit width, a template parameter: 1 byte (ODF, PDF), 2
 * bytes (Office, a UTF-16 code unit); LIMIT = 64 / U units.  There are two tiles: out-of-place functions write the
 * other tile and the lane switches over; at the end every lane writes its column, cut at the format's truncation and
 * zero-padded, into tile 0 -- so neither tile is cleared first.  Neighbouring lanes run different rules, so the
 * functions are folded into four code paths that a wave walks once per function step:
 *   gather  r d p f { } q [ D x O i z Z y Y $ ^   out[j] = w[src(j)] over at most three segments (start, step, length;
 *                                                 a segment may be the constant unit, or read the output: p)
 *   map     l u c C t E s @                       one pass over the units: case by position, substitute, delete
 *   point   k K * T o . ,                         two units read, two written
 *   length  : ] '                                 nothing moves
 * Every position is masked to LIMIT - 1 before it addresses LDS and every length is clamped to LIMIT; word, rule and
 * function indices are clamped to the table sizes in the arguments.  44-47 VGPRs. */
namespace {
/* unit `pos` of lane tid's column in tile t; pos is masked into the column */
template <int U> DEVI uint32_t ru(const uint32_t *t, uint32_t tid, uint32_t pos) {
    pos &= 64u / U - 1u;
    if (U == 1) return ((const uint8_t *)t)[col_byte(tid, pos)];
    return ((const uint16_t *)t)[2u * ((pos >> 1) * ST + tid) + (pos & 1u)];
}
template <int U> DEVI void wu(uint32_t *t, uint32_t tid, uint32_t pos, uint32_t v) {
    pos &= 64u / U - 1u;
    if (U == 1) ((uint8_t *)t)[col_byte(tid, pos)] = (uint8_t)v;
    else ((uint16_t *)t)[2u * ((pos >> 1) * ST + tid) + (pos & 1u)] = (uint16_t)v;
}

DEVI bool ascii_letter(uint32_t v) { return ((v | 0x20u) - 0x61u) < 26u; }
/* case mode 1 lower, 2 upper, 3 toggle, 0 none; ASCII letters only */
DEVI uint32_t recase(uint32_t v, uint32_t mode) {
    if (!ascii_letter(v)) return v;
    return mode == 1u ? (v | 0x20u) : mode == 2u ? (v & ~0x20u) : mode == 3u ? (v ^ 0x20u) : v;
}
}  // namespace

enum { C_LEN = 0, C_GATHER = 1, C_MAP = 2, C_POINT = 3 };
enum { P_SWAP = 0, P_COPY = 1, P_SET = 2, P_TOGGLE = 3 };

template <int U>
__global__ void __launch_bounds__(256)
k_spell_rules(dprf_rules_args a, const uint32_t *fns, const uint32_t *roff, const uint32_t *wblob,
              const uint32_t *woff, uint32_t *slots, uint8_t *lens) {
    constexpr uint32_t LIMIT = 64u / U;
    __shared__ uint32_t tile[2 * TW];
    __shared__ uint32_t soff[DPRF_HYB_RUN + 1];
    __shared__ uint32_t run[DPRF_HYB_RUN_WORDS];
    __shared__ uint32_t ends[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t base = blockIdx.x * 256u;
    const uint32_t g = base + tid;
    const bool live = g < a.count;
    const uint32_t lim = a.trunc < 4u * DPRF_SLOT_WORDS ? a.trunc : 4u * DPRF_SLOT_WORDS;
    const uint32_t R = a.nrules ? a.nrules : 1u;
    uint32_t w = 0, rule = 0;
    if (live) {
        const uint32_t idx = a.r0 + g;
        const uint32_t q = R == 1u ? idx : fastdiv(idx, a.div_m, a.div_s);
        rule = idx - q * R;
        rule = rule < R ? rule : R - 1u;
        w = a.w0 + q;
        w = w < a.nwords ? w : a.nwords - 1u;
    }
    const word_run r = stage_run(live, w, tid, base, a.count, a.bwords, wblob, woff, ends, soff, run);
    if (live) {
        uint32_t wl;
        const uint32_t src = find_word(r, w, soff, wl);
        const uint8_t *rb = (const uint8_t *)run;
        uint8_t *tb = (uint8_t *)tile;
        for (uint32_t j = 0; j < wl; j++) tb[col_byte(tid, j)] = rb[src + j];
        uint32_t n = wl / U;                                     /* the candidate's length in units */
        uint32_t cur = 0;                                        /* the tile that holds it */
        /* the lane's rule: functions [f0, f0 + nf) of the table */
        const uint32_t f0 = roff[rule], f1 = roff[rule + 1u];
        uint32_t nf = f1 > f0 ? f1 - f0 : 0u;
        nf = nf < DPRF_RULE_FNS ? nf : DPRF_RULE_FNS;
        nf = f0 < a.nfns && nf <= a.nfns - f0 ? nf : 0u;
        for (uint32_t f = 0; f < nf; f++) {
            const uint32_t fw = fns[f0 + f];
            const uint32_t op = fw & 0xffu, N = (fw >> 8) & 0xffu, M = (fw >> 16) & 0xffu;
            uint32_t cls = C_LEN, m = n;
            /* gather: segments of l1, l2 and the rest units, unit t of a segment from a + s * (t >> sh); cst bit k: the
             * segment is the constant X; self: the second segment reads the output */
            uint32_t l1 = 0, l2 = 0, a1 = 0, a2 = 0, a3 = 0, s1 = 1, s2 = 1, sh = 0, cst = 0, self = 0, X = 0;
            /* map: case mode of every unit / of unit 0 (E: of every unit after a blank too), substitute X by Y,
             * delete X */
            uint32_t mall = 0, mfirst = 0, eflag = 0, sub = 0, del = 0, Y = 0;
            /* point: units pi and pj */
            uint32_t pi = 0, pj = 0, pmode = P_SWAP;
#define GATHER(m_, l1_, a1_, s1_, l2_, a2_, s2_, a3_) \
    do { cls = C_GATHER; m = (m_); l1 = (l1_); a1 = (a1_); s1 = (uint32_t)(s1_); l2 = (l2_); a2 = (a2_); \
         s2 = (uint32_t)(s2_); a3 = (a3_); } while (0)
#define POINT(i_, j_, mode_) do { cls = C_POINT; pi = (i_); pj = (j_); pmode = (mode_); } while (0)
#define MAP(all_, first_) do { cls = C_MAP; mall = (all_); mfirst = (first_); } while (0)
            switch (op) {
                case 'l': MAP(1, 1); break;
                case 'u': MAP(2, 2); break;
                case 'c': MAP(1, 2); break;
                case 'C': MAP(2, 1); break;
                case 't': MAP(3, 3); break;
                case 'E': MAP(1, 2); eflag = 1; break;
                case 's': MAP(0, 0); sub = 1; X = N; Y = M; break;
                case '@': MAP(0, 0); del = 1; X = N; break;
                case 'T': if (N < n) POINT(N, N, P_TOGGLE); break;
                case 'o': if (N < n) { POINT(N, N, P_SET); X = M; } break;
                case 'k': if (n >= 2u) POINT(0u, 1u, P_SWAP); break;
                case 'K': if (n >= 2u) POINT(n - 2u, n - 1u, P_SWAP); break;
                case '*': if (N < n && M < n) POINT(N, M, P_SWAP); break;
                case '.': if (N + 1u < n) POINT(N, N + 1u, P_COPY); break;
                case ',': if (N >= 1u && N < n) POINT(N, N - 1u, P_COPY); break;
                case ']': m = n - 1u; break;
                case '\'': if (N < n) m = N; break;
                case 'r': GATHER(n, n, n - 1u, -1, 0u, 0u, 1, 0u); break;
                case 'd': GATHER(2u * n, n, 0u, 1, n, 0u, 1, 0u); break;
                case 'p': GATHER(n * (N + 1u), n, 0u, 1, n * N, 0u, 1, 0u); self = 1; break;
                case 'f': GATHER(2u * n, n, 0u, 1, n, n - 1u, -1, 0u); break;
                case '{': GATHER(n, n - 1u, 1u, 1, 1u, 0u, 1, 0u); break;
                case '}': GATHER(n, 1u, n - 1u, 1, n - 1u, 0u, 1, 0u); break;
                case 'q': GATHER(2u * n, 2u * n, 0u, 1, 0u, 0u, 1, 0u); sh = 1; break;
                case '[': GATHER(n - 1u, n - 1u, 1u, 1, 0u, 0u, 1, 0u); break;
                case 'D': if (N < n) GATHER(n - 1u, N, 0u, 1, n - 1u - N, N + 1u, 1, 0u); break;
                case 'x': if (N + M <= n) GATHER(M, M, N, 1, 0u, 0u, 1, 0u); break;
                case 'O': if (N + M <= n) GATHER(n - M, N, 0u, 1, n - N - M, N + M, 1, 0u); break;
                case 'i': if (N <= n) { GATHER(n + 1u, N, 0u, 1, 1u, 0u, 0, N); cst = 2; X = M; } break;
                case 'z': GATHER(n + N, N, 0u, 0, n, 0u, 1, 0u); break;
                case 'Z': GATHER(n + N, n, 0u, 1, N, n - 1u, 0, 0u); break;
                case 'y': if (N <= n) GATHER(n + N, N, 0u, 1, n, 0u, 1, 0u); break;
                case 'Y': if (N <= n) GATHER(n + N, n, 0u, 1, N, n - N, 1, 0u); break;
                case '$': GATHER(n + 1u, n, 0u, 1, 1u, 0u, 0, 0u); cst = 2; X = N; break;
                case '^': GATHER(n + 1u, 1u, 0u, 0, n, 0u, 1, 0u); cst = 1; X = N; break;
                default: break;                                  /* ':' and anything unknown: unchanged */
            }
#undef GATHER
#undef POINT
#undef MAP
            /* the two global rules: a result that would be empty or longer than LIMIT leaves the candidate unchanged */
            if (m == 0u || m > LIMIT) { cls = C_LEN; m = n; }
            uint32_t *ct = tile + cur * TW;
            if (cls == C_GATHER) {
                uint32_t *dt = tile + (cur ^ 1u) * TW;
                for (uint32_t j = 0; j < m; j++) {
                    uint32_t t = j, sa = a1, ss = s1, k = 1u;
                    const uint32_t *from = ct;
                    if (j >= l1) { t = j - l1; sa = a2; ss = s2; k = 2u; from = self ? dt : ct; }
                    if (j >= l1 + l2) { t = j - l1 - l2; sa = a3; ss = 1u; k = 4u; from = ct; }
                    const uint32_t v = ru<U>(from, tid, sa + ss * (t >> sh));
                    wu<U>(dt, tid, j, (cst & k) ? X : v);
                }
                cur ^= 1u;
            } else if (cls == C_MAP) {
                uint32_t k = 0, prev = 0;
                for (uint32_t j = 0; j < n; j++) {
                    const uint32_t v = ru<U>(ct, tid, j);
                    const bool first = j == 0u || (eflag && prev == 0x20u);
                    uint32_t nv = recase(v, first ? mfirst : mall);
                    if (sub && v == X) nv = Y;
                    if (!(del && v == X)) { wu<U>(ct, tid, k, nv); k++; }
                    prev = v;
                }
                m = k ? k : n;                                   /* everything deleted: nothing was written */
            } else if (cls == C_POINT) {
                const uint32_t va = ru<U>(ct, tid, pi), vb = ru<U>(ct, tid, pj);
                const uint32_t tg = recase(va, 3u);
                const uint32_t na = pmode == P_SWAP ? vb : pmode == P_COPY ? vb : pmode == P_SET ? X : tg;
                const uint32_t nb = pmode == P_SWAP ? va : pmode == P_COPY ? vb : pmode == P_SET ? X : tg;
                wu<U>(ct, tid, pj, nb);
                wu<U>(ct, tid, pi, na);
            }
            n = m;
        }
        /* the lane's column into tile 0: cut at the format's truncation, zero behind the last byte */
        const uint32_t total = n * U;
        const uint32_t outlen = total < lim ? total : lim;
        const uint32_t *ct = tile + cur * TW;
#pragma unroll
        for (uint32_t j = 0; j < DPRF_SLOT_WORDS; j++) {
            uint32_t v = ct[j * ST + tid];
            const uint32_t keep = outlen > 4u * j ? outlen - 4u * j : 0u;
            v = keep >= 4u ? v : (keep == 0u ? 0u : v & ((1u << (8u * keep)) - 1u));
            tile[j * ST + tid] = v;
        }
        lens[g] = (uint8_t)outlen;
    }
    __syncthreads();
    read_out(tile, tid, base, a.count, slots);
}

/* ================================================================== combinator windows */
/* Candidate g of the chunk is left word a.l0 + (a.r0 + g) / N2 followed by right word (a.r0 + g) % N2 (N2 = a.nright):
 * the chunk start's two indices travel in the arguments and the division is the rules kernel's multiply-high
 * (a.r0 + g < 2^32: N2 < 2^31, a chunk holds at most 2^26 candidates).
 *
 * The left words of a block do not decrease with g: one contiguous run of at most 256 words, staged by stage_run as
 * the hybrid and rules kernels stage theirs.  The right words of a block are R0, R0 + 1, ... modulo N2, R0 being lane
 * 0's.  For N2 <= 256 the block may cycle through the table several times, so the whole table is staged and a lane's
 * entry is its right index; for N2 > 256 the block wraps at most once, so the words from R0 to the table's end and
 * then those from word 0 are staged, two byte ranges back to back in rrun[], and a lane's entry is (R - R0) mod N2.
 * Either way at most 256 words and 16 KB, copied with consecutive loads; no lane gathers word bytes from global memory.
 * An entry of rent[] is the word's first byte in rrun[] (bits 0-15) and its length (bits 16-23), written by the lane of
 * the same number and clamped where it is read: the length to a slot, the first byte to a slot or more before the end
 * of rrun[] -- whatever the offsets say, as in find_word.  R0 is recomputed by every lane from the block's base (a
 * block-uniform value), so the right run needs no published ends. */
__global__ void __launch_bounds__(256)
k_spell_combine(dprf_combine_args a, const uint32_t *lblob, const uint32_t *loff, const uint32_t *rblob,
                const uint32_t *roff, uint32_t *slots, uint8_t *lens) {
    __shared__ uint32_t tile[TW];
    __shared__ uint32_t soff[DPRF_HYB_RUN + 1];
    __shared__ uint32_t run[DPRF_HYB_RUN_WORDS];
    __shared__ uint32_t ends[2];
    __shared__ uint32_t rent[DPRF_HYB_RUN];
    __shared__ uint32_t rrun[DPRF_HYB_RUN_WORDS];
    const uint32_t tid = threadIdx.x;
    const uint32_t base = blockIdx.x * 256u;
    const uint32_t g = base + tid;
    const bool live = g < a.count;
    const uint32_t lim = a.trunc < 4u * DPRF_SLOT_WORDS ? a.trunc : 4u * DPRF_SLOT_WORDS;
    const uint32_t N2 = a.nright ? a.nright : 1u;
    tile_clear(tile, tid);
    /* lane 0's right word: the same value in every lane */
    const uint32_t idx0 = a.r0 + base;
    const uint32_t q0 = N2 == 1u ? idx0 : fastdiv(idx0, a.div_m, a.div_s);
    uint32_t R0 = idx0 - q0 * N2;
    R0 = R0 < N2 ? R0 : N2 - 1u;
    uint32_t L = 0, R = 0;
    if (live) {
        const uint32_t idx = a.r0 + g;
        const uint32_t q = N2 == 1u ? idx : fastdiv(idx, a.div_m, a.div_s);
        R = idx - q * N2;
        R = R < N2 ? R : N2 - 1u;
        L = a.l0 + q;
        L = L < a.nleft ? L : a.nleft - 1u;
    }
    {
        /* the right run: words [first, first + n1) and then [0, n2) of the table.  The roff[] reads below stay at or
         * under index N2: that roff[] holds a.nright + 1 offsets is the host's word (dprf_ctx_set_right_words uploads
         * both together), the one thing here no clamp guarantees -- as a.nwords and woff[] in stage_run */
        const uint32_t left = a.count > base ? a.count - base : 1u;
        const uint32_t nlive = left < 256u ? left : 256u;
        const bool whole = N2 <= DPRF_HYB_RUN;
        const uint32_t first = whole ? 0u : R0;
        const uint32_t n1 = whole ? N2 : (nlive < N2 - R0 ? nlive : N2 - R0);
        const uint32_t n2 = whole ? 0u : nlive - n1;
        const uint32_t b0 = roff[first], b1 = roff[first + n1];
        const uint32_t a0 = b0 >> 2;
        uint32_t nu1 = b1 > 4u * a0 ? (b1 - 4u * a0 + 3u) >> 2 : 0u;
        nu1 = nu1 < DPRF_HYB_RUN_WORDS ? nu1 : DPRF_HYB_RUN_WORDS;
        nu1 = a0 < a.rbwords ? (nu1 < a.rbwords - a0 ? nu1 : a.rbwords - a0) : 0u;
        const uint32_t c0 = roff[0], c1 = roff[n2];
        const uint32_t e0 = c0 >> 2;
        uint32_t nu2 = n2 && c1 > 4u * e0 ? (c1 - 4u * e0 + 3u) >> 2 : 0u;
        nu2 = nu2 < DPRF_HYB_RUN_WORDS - nu1 ? nu2 : DPRF_HYB_RUN_WORDS - nu1;
        nu2 = e0 < a.rbwords ? (nu2 < a.rbwords - e0 ? nu2 : a.rbwords - e0) : 0u;
        for (uint32_t k = tid; k < nu1; k += 256u) rrun[k] = rblob[a0 + k];
        for (uint32_t k = tid; k < nu2; k += 256u) rrun[nu1 + k] = rblob[e0 + k];
        uint32_t ent = 0u;
        if (tid < n1 + n2) {
            const bool one = tid < n1;
            const uint32_t wk = one ? first + tid : tid - n1;
            const uint32_t o0 = roff[wk], o1 = roff[wk + 1u];
            const uint32_t wl = o1 > o0 ? o1 - o0 : 0u;
            const uint32_t at = one ? o0 - 4u * a0 : 4u * nu1 + (o0 - 4u * e0);
            ent = (at & 0xffffu) | ((wl < 4u * DPRF_SLOT_WORDS ? wl : 4u * DPRF_SLOT_WORDS) << 16);
            ent = at < 0x10000u ? ent : 0u;
        }
        rent[tid] = ent;
    }
    /* the left run; its last barrier also covers the right run's stores and the cleared tile */
    const word_run r = stage_run(live, L, tid, base, a.count, a.lbwords, lblob, loff, ends, soff, run);
    if (live) {
        uint32_t wl;
        const uint32_t lsrc = find_word(r, L, soff, wl);
        const uint32_t d = N2 <= DPRF_HYB_RUN ? R : (R >= R0 ? R - R0 : R + (N2 - R0));
        const uint32_t ent = rent[d < DPRF_HYB_RUN ? d : DPRF_HYB_RUN - 1u];
        uint32_t rl = (ent >> 16) & 0xffu;
        rl = rl < 4u * DPRF_SLOT_WORDS ? rl : 4u * DPRF_SLOT_WORDS;
        uint32_t rsrc = ent & 0xffffu;
        rsrc = rsrc <= 4u * DPRF_HYB_RUN_WORDS - 4u * DPRF_SLOT_WORDS ? rsrc : 0u;
        const uint8_t *lb = (const uint8_t *)run, *rb = (const uint8_t *)rrun;
        for (uint32_t j = 0; j < wl; j++) put_byte(tile, tid, j, lim, lb[lsrc + j]);
        for (uint32_t j = 0; j < rl; j++) put_byte(tile, tid, wl + j, lim, rb[rsrc + j]);
        const uint32_t total = wl + rl;
        lens[g] = (uint8_t)(total < lim ? total : lim);
    }
    __syncthreads();
    read_out(tile, tid, base, a.count, slots);
}

/* ------------------------------------------------------------------ launchers (dprf_launch.h) */
static dim3 blocks_of(uint32_t count) { return dim3((count + 255u) / 256u); }

hipError_t launch_spell_symbols(const dprf_enum &e, const uint32_t *symtab, uint32_t trunc, uint32_t *slots,
                                uint8_t *lens, hipStream_t s) {
    hipLaunchKernelGGL(k_spell_symbols, blocks_of(e.count), dim3(256), 0, s, e, symtab, trunc, slots, lens);
    return hipGetLastError();
}
hipError_t launch_spell_mask(const dprf_mask_args &a, const uint32_t *tab, uint32_t *slots, uint8_t *lens,
                             hipStream_t s) {
    hipLaunchKernelGGL(k_spell_mask, blocks_of(a.count), dim3(256), 0, s, a, tab, slots, lens);
    return hipGetLastError();
}
hipError_t launch_spell_hybrid(const dprf_hybrid_args &a, const uint32_t *tab, const uint32_t *wblob,
                               const uint32_t *woff, uint32_t *slots, uint8_t *lens, hipStream_t s) {
    hipLaunchKernelGGL(k_spell_hybrid, blocks_of(a.m.count), dim3(256), 0, s, a, tab, wblob, woff, slots, lens);
    return hipGetLastError();
}
hipError_t launch_spell_rules(const dprf_rules_args &a, const uint32_t *fns, const uint32_t *roff,
                              const uint32_t *wblob, const uint32_t *woff, uint32_t *slots, uint8_t *lens,
                              hipStream_t s) {
    if (a.unit == 2u)
        hipLaunchKernelGGL(k_spell_rules<2>, blocks_of(a.count), dim3(256), 0, s, a, fns, roff, wblob, woff, slots,
                           lens);
    else
        hipLaunchKernelGGL(k_spell_rules<1>, blocks_of(a.count), dim3(256), 0, s, a, fns, roff, wblob, woff, slots,
                           lens);
    return hipGetLastError();
}
hipError_t launch_spell_combine(const dprf_combine_args &a, const uint32_t *lblob, const uint32_t *loff,
                                const uint32_t *rblob, const uint32_t *roff, uint32_t *slots, uint8_t *lens,
                                hipStream_t s) {
    hipLaunchKernelGGL(k_spell_combine, blocks_of(a.count), dim3(256), 0, s, a, lblob, loff, rblob, roff, slots, lens);
    return hipGetLastError();
}
