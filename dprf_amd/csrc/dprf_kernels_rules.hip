/* dprf_kernels_rules.hip -- rule windows (dprf_search_rules, dprf_spell_rules): a word of the context's table with a
 * rule of the call's rule table applied to it (include/dprf.h "rule mode" defines the language).
 *
 * Candidate g of the chunk is rule (a.r0 + g) % R applied to word a.w0 + (a.r0 + g) / R: the chunk start's word and
 * rule index travel in the arguments, the division is a multiply-high with the host's magic (a.r0 + g < 2^32: chunks
 * hold at most 2^26 candidates, R at most 2^20).  The rule table -- one u32 per function, R + 1 offsets -- is uploaded
 * once per call and read from global memory: small, call-constant, served from L2.
 *
 * Staging and read-out are k_spell_hybrid's (dprf_kernels_hybrid.hip): word indices do not decrease with g, so a
 * block's 256 candidates use one contiguous run of at most 256 words, which the block copies into LDS with consecutive
 * u32 loads, offsets included; the finished candidates leave through the ST = 258 lane-column tile with four uint4
 * stores per lane, so slots and lens are laid out as every other spelling kernel lays them out.
 *
 * The interpreter indexes the candidate at run-time positions, so the working copy lives in LDS (a private array
 * would go to scratch): one column of the tile per lane, unit j of lane t in word (j * U / 4) * ST + t, which keeps a
 * wave's accesses to one position conflict-free.  U is the unit width, a template parameter: 1 byte (ODF, PDF), 2
 * bytes (Office, a UTF-16 code unit); LIMIT = 64 / U units.  There are two tiles: out-of-place functions write the
 * other tile and the lane switches over; at the end every lane writes its column, cut at the format's truncation and
 * zero-padded, into tile 0.  Neighbouring lanes run different rules, so the functions are folded into four code paths
 * that a wave walks once per function step:
 *   gather  r d p f { } q [ D x O i z Z y Y $ ^   out[j] = w[src(j)] over at most three segments (start, step, length;
 *                                                 a segment may be the constant unit, or read the output: p)
 *   map     l u c C t E s @                       one pass over the units: case by position, substitute, delete
 *   point   k K * T o . ,                         two units read, two written
 *   length  : ] '                                 nothing moves
 * Every position is masked to LIMIT - 1 before it addresses LDS and every length is clamped to LIMIT; word, rule and
 * function indices are clamped to the table sizes in the arguments.  The host validates the tables, but memory safety
 * here does not depend on that.
 *
 * LDS per block: two tiles 2 x 16,512 + offsets 1,028 + run 16,388 + the two ends 8 = 50,448 B (50,452 as the compiler
 * lays it out), so three blocks (12 waves) fit a CU's 160 KB, as for k_spell_hybrid; 44-47 VGPRs, no scratch.
 *
 * An object of its own (Makefile), so the other kernel objects keep their machine code.
 */
#include "dev_crypto.h"
#include "dprf_params.h"
#include "dprf_launch.h"

namespace {
constexpr uint32_t ST = 258;
constexpr uint32_t TW = DPRF_SLOT_WORDS * ST;                /* words of one tile */

DEVI uint32_t rul_fastdiv(uint32_t n, uint32_t m, uint32_t s) {
    const uint32_t t = __umulhi(n, m);
    return (t + ((n - t) >> 1)) >> s;
}

/* unit `pos` of lane tid's column in tile t; pos is masked into the column */
template <int U> DEVI uint32_t ru(const uint32_t *t, uint32_t tid, uint32_t pos) {
    pos &= 64u / U - 1u;
    if (U == 1) return ((const uint8_t *)t)[4u * ((pos >> 2) * ST + tid) + (pos & 3u)];
    return ((const uint16_t *)t)[2u * ((pos >> 1) * ST + tid) + (pos & 1u)];
}
template <int U> DEVI void wu(uint32_t *t, uint32_t tid, uint32_t pos, uint32_t v) {
    pos &= 64u / U - 1u;
    if (U == 1) ((uint8_t *)t)[4u * ((pos >> 2) * ST + tid) + (pos & 3u)] = (uint8_t)v;
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
        const uint32_t q = R == 1u ? idx : rul_fastdiv(idx, a.div_m, a.div_s);
        rule = idx - q * R;
        rule = rule < R ? rule : R - 1u;
        w = a.w0 + q;
        w = w < a.nwords ? w : a.nwords - 1u;
        const uint32_t left = a.count - base;                    /* live lanes of the block: 1..256 of them */
        if (tid == 0u) ends[0] = w;
        if (tid == (left < 256u ? left : 256u) - 1u) ends[1] = w;
    }
    __syncthreads();
    /* the run lane 0's word .. the last live lane's word: its nw + 1 offsets and its bytes, as whole u32 words from
     * the one that holds the run's first byte (k_spell_hybrid's staging) */
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
        for (uint32_t j = 0; j < wl; j++) tb[4u * ((j >> 2) * ST + tid) + (j & 3u)] = rb[src + j];
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
    uint4 *out = (uint4 *)(slots + (size_t)base * DPRF_SLOT_WORDS);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t u = 256u * q + tid, sl = u >> 2, w0 = 4u * (u & 3u);
        if (base + sl < a.count)
            out[u] = make_uint4(tile[w0 * ST + sl], tile[(w0 + 1) * ST + sl], tile[(w0 + 2) * ST + sl],
                                tile[(w0 + 3) * ST + sl]);
    }
}

hipError_t launch_spell_rules(const dprf_rules_args &a, const uint32_t *fns, const uint32_t *roff,
                              const uint32_t *wblob, const uint32_t *woff, uint32_t *slots, uint8_t *lens,
                              hipStream_t s) {
    const dim3 grid((a.count + 255u) / 256u), block(256);
    if (a.unit == 2u)
        hipLaunchKernelGGL(k_spell_rules<2>, grid, block, 0, s, a, fns, roff, wblob, woff, slots, lens);
    else
        hipLaunchKernelGGL(k_spell_rules<1>, grid, block, 0, s, a, fns, roff, wblob, woff, slots, lens);
    return hipGetLastError();
}
