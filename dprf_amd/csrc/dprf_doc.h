/* dprf_doc.h -- the device-free half of the host library: what a document stream says (the six parsers), what the
 * library knows of each kernel family (one table), chunk planning, and everything that judges a candidate, a word, a
 * mask or a rule table without a device.  No device runtime here: a plain C++17 compiler builds dprf_doc.cpp, so the
 * parsers of untrusted text run in a stand-alone program (tests/host/doc_check.cpp).  dprf_host.cpp holds the device
 * half; the names the two share live in dprf_internal and stay out of the dynamic symbol table. */
#ifndef DPRF_DOC_H
#define DPRF_DOC_H
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/dprf.h"
#include "dprf_params.h"

/* R2-R4 launches per device alternate between this many streams (1 or 2).  Round 4: two processes sharing one GPU ran
 * R3/R4 1.7 % faster than one (profiles/bench_n2_rehearsal_r04g.json) -- a 2^25-candidate launch is 28.4 generations
 * of resident workgroups, and the next launch can fill the CUs its last, partial generation leaves idle.  Two streams
 * in one process: R4 612.7 -> 625.0 M, R3 40-bit 613.8 -> 626.6 M (three alternating runs each, profiles/
 * ab_r24_streams_r04h.txt), R2 (one 2^30-candidate launch per call) unchanged; 2^27-candidate launches on one stream
 * instead: +1.5 % (profiles/ab_r24_streams_r04i.txt).  A launch's event time then includes the overlap with its
 * neighbour, so bench.py quotes the R2-R4 floor fraction from wall time. */
#ifndef DPRF_R24_STREAMS
#define DPRF_R24_STREAMS 2
#endif
/* ODF 1.0 / 1.1: streams per device (1 or 2).  With 2 the KDF kernels of all launches run on `stream` and the Blowfish
 * checks on `stream2`, so that the check of launch k (one wave per CU, bound by LDS latency) may run beside the KDF of
 * launch k + 1 (VALU-bound, next to no LDS).  The key buffer has two halves, launch k using half k % 2; the KDF of
 * launch k + 2 waits for the check of launch k.  Measured on MI355X: 10.29 M cand/s with one stream, 10.43 M with two
 * (+1.4 %): the two kernels hardly overlap, and one stream stays the default (DESIGN.md 4f has the A/B). */
#ifndef DPRF_ODF_STREAMS
#define DPRF_ODF_STREAMS 1
#endif

namespace dprf_internal __attribute__((visibility("hidden"))) {

/* ------------------------------------------------------------------ errors */
/* Sets the calling thread's error text (dprf_last_error) and returns `code`. */
int fail(int code, const char *fmt, ...);

/* ------------------------------------------------------------------ kernel families */
enum kernel_kind { K_NONE, K_OFFICE, K_ODT, K_PDF_R24, K_PDF_R5, K_PDF_R6, K_AGILE_SHA1, K_AGILE_SHA512,
                   K_OLDOFFICE_MD5, K_OLDOFFICE_SHA1, K_ODF_BF, K_ODF_AES, K_COUNT };

/* Candidates per launch.  A device takes its next chunk from the call's shared cursor sized for about
 * `target_ms` of device time at the rate it measured on its last launch (`init` before the first), a
 * power of two in [lo, hi].  The floors keep whole waves of workgroups on the chip: Office's 2^19 is one
 * full generation of k_office_kdf (256 CUs x 32 waves x 64 lanes); R6's persistent workgroups drain at the
 * end of every launch, so its launches take ~3 s (dprf_doc.cpp).
 * Multi-device calls add guided self-scheduling (plan_chunk): a take is capped at remaining / (4 ndev) -- 2 ndev
 * for guided self-scheduling, times the MULTI_DEPTH = 2 launches each device keeps in flight -- so the chunks
 * shrink as the cursor runs out and the devices finish within about one `tail` chunk of each other;
 * never below `tail` (the smallest launch that still runs at nearly full rate), nor below total / ndev for a
 * call smaller than ndev tails, so a small call (a 20,000-candidate client payload) still spreads over every
 * device.  `gran` rounds capped takes up to whole workgroups. */
struct chunk_policy { uint32_t init, lo, hi; double target_ms; uint32_t tail, gran; };

/* What the library knows of one kernel family: one row per kernel_kind (FAMILIES in dprf_doc.cpp), read by everything
 * that used to decide per kind.  A new family adds its row, its parser and its case in launch(). */
struct family {
    kernel_kind kind;        /* the row's own index: the build fails when a row is missing or out of place */
    const char *name;        /* dprf_ctx_kernel, dprf_plan_chunk */
    const char *owner_name;  /* the PDF kinds: the name while the owner password is searched, else null */
    const char *key40_name;  /* the kinds with 40-bit documents: the name of their key search (dprf_search_key40), else null */
    const char *collide_name; /* ... and the name while a known key is set (dprf_ctx_set_key40), else null */
    chunk_policy policy;
    uint32_t trunc;          /* bytes at which the format's verifier cuts a candidate: 32, 127, ~0u for nowhere */
    uint32_t key_words;      /* words per candidate of the KDF -> check hand-off in HBM; 0: one kernel, no hand-off */
    uint32_t long_alg;       /* the long-list prehash (DPRF_LONG_*); 0: the family has no long-list mode */
    bool long_keys;          /* ... and whether that prehash writes keys for the family's kernels */
    const char *no_long;     /* no long-list mode: why a candidate over a slot is refused, else null */
    int streams;             /* streams per device */
};
extern const family FAMILIES[K_COUNT];
inline const family &fam(kernel_kind k) { return FAMILIES[k]; }
const char *kind_name(kernel_kind k, bool owner = false, bool collide = false);
/* owner: the owner-password kernels of the PDF families do about twice the work per candidate: the user family's
 * policy with the first chunk halved (the measured rate sizes the later ones).
 * collide: a known key is set (dprf_ctx_set_key40) and the password searches run the collider kernels, hashing only:
 * the password family's policy (dprf_doc.cpp policy() says what differs) */
/* iterations: the PBKDF2 count of a K_ODF_AES document (plan_iterations), 0 for every other one.  That family's row
 * describes 1024 iterations: the first launch, the floor and the tail scale by 1024 / iterations, rounded up to the
 * granularity, never above `hi` (the key buffer) nor below ODF_AES_GENERATION.  Past 1638 iterations the floor is no
 * power of two any more, so plan_chunk holds its doubling to `hi`. */
chunk_policy policy(kernel_kind k, bool owner = false, bool collide = false, uint32_t iterations = 0);
uint64_t round_up(uint64_t v, uint64_t g);
uint64_t plan_chunk(kernel_kind k, bool owner, double rate, uint64_t remaining, uint64_t total, int ndev, int inflight,
                    bool collide = false, uint32_t iterations = 0);
/* One resident generation of k_odf_aes_kdf at the occupancy it builds with: 256 CUs x 4 SIMDs x 5 waves x 64 lanes
 * (ODF_AES_KDF_WAVES where the kernel is defined) */
static const uint32_t ODF_AES_GENERATION = 256u * 4u * 5u * 64u;
/* The key search of a family (dprf_search_key40) plans with the password family's policy, owner = false: the measured
 * rate sizes the later chunks.  Its name, or null when the family has no 40-bit documents. */
inline const char *key40_name(kernel_kind k) { return fam(k).key40_name; }

/* ------------------------------------------------------------------ the document */
/* What a context knows without a device; dprf_ctx (dprf_host.cpp) has it as its base. */
struct dprf_doc {
    int fmt = 0, flags = 0;
    kernel_kind kind = K_NONE;
    dprf_office_params office{};
    dprf_agile_params agile{};        /* Office 2010 / 2013 (K_AGILE_*) */
    dprf_oldoffice_params oldoffice{};/* Office 97-2003 RC4 (K_OLDOFFICE_*) */
    dprf_odt_params odt{};
    dprf_pdf_params pdf{};            /* .owner: which password the searches verify (dprf_ctx_set_pdf_password) */
    bool has_key40 = false;           /* a known key is set (dprf_ctx_set_key40): the searches verify against it */
    uint8_t key40[5] = {};            /* ... its five bytes, in the order dprf_search_key40 reports */
    int pdf_o_len = 0, pdf_u_len = 0; /* decoded /O and /U lengths: what the owner check needs is tested when it is selected */
    std::vector<uint32_t> odt_words;  /* first min(len,1024) ciphertext bytes, BE words */
    dprf_odf_params odf{};            /* ODF 1.0 / 1.1 Blowfish (K_ODF_BF) */
    std::vector<uint32_t> odf_words;  /* iv || content[0:1024], BE words: the E_key inputs and the ciphertext in one run */
    dprf_odf_aes_params odfaes{};     /* ODF 1.2 at the manifest's count (K_ODF_AES): the KDF's half; odt / odt_words
                                         hold the check's */
    dprf_long_params lp{};            /* the long-list prehash of the format (set_long_params) */
    /* the word table of hybrid searches (dprf_ctx_set_words; the lanes hold the bytes): its size, and its longest
     * word before the clip to a slot, which decides whether a mask fits */
    uint64_t nwords = 0;
    uint64_t w_longest = 0, w_longest_idx = 0;
    /* the right table of combinator searches (dprf_ctx_set_right_words), kept as the table above is: that one is the
     * left table there */
    uint64_t nright = 0;
    uint64_t r_longest = 0, r_longest_idx = 0;
};

/* What policy() and plan_chunk() take as `iterations` for this document */
inline uint32_t plan_iterations(const dprf_doc *d) { return d->kind == K_ODF_AES ? d->odfaes.iterations : 0u; }

/* The field array of dprf_ctx_create: parse_verification_data's accepted shapes (brute_force.py:253-260) by tag and
 * field count, the tag's parser, and on success the long-list parameters.  Fills fmt, flags, kind and the params. */
int parse_document(dprf_doc *d, const char *const *fields, int nfields);
int check_pdf_password(const dprf_doc *d, int which);   /* DPRF_PDF_USER / DPRF_PDF_OWNER on this document */
/* dprf_search_key40 on this document: the window (start + count <= 2^40, computed without wrapping: DPRF_E_INVALID),
 * then the domain -- PDF R2, R3/R4 with a 5-byte key, Office 97-2003 types 0 / 1 / 3, or a never-matching context;
 * every other document is DPRF_E_DOMAIN with a message that says why it is not a 40-bit one */
int check_key40(const dprf_doc *d, uint64_t start, uint64_t count);
/* The domain half alone: DPRF_OK on a 40-bit document or a never-matching context, else DPRF_E_DOMAIN and the sentence */
int check_key40_domain(const dprf_doc *d);
/* dprf_ctx_set_key40 on this document (set: a key is given, not cleared): the domain, then DPRF_E_INVALID for a PDF in
 * owner mode -- a key collider finds the user password.  check_pdf_password refuses the other order. */
int check_set_key40(const dprf_doc *d, bool set);
/* The collider's compare words of the set key: LE words of its bytes 0..3 and byte 4, as MD5's h[0] and h[1] & 0xff */
inline void key40_words(const dprf_doc *d, uint32_t k[2]) {
    k[0] = (uint32_t)d->key40[0] | (uint32_t)d->key40[1] << 8 | (uint32_t)d->key40[2] << 16 | (uint32_t)d->key40[3] << 24;
    k[1] = d->key40[4];
}

const dprf_aes_tables &aes_tables();

/* ------------------------------------------------------------------ candidates, words, windows */
static const uint32_t SLOT_BYTES = 4 * DPRF_SLOT_WORDS;

void fastdiv_magic(uint32_t d, uint32_t &m, uint32_t &s);
int utf8_to_utf16le(const uint8_t *s, size_t n, uint8_t *out, size_t cap);
int convert_candidate(const dprf_doc *c, const uint8_t *pw, size_t len, const uint8_t **out, size_t *olen,
                      std::vector<uint8_t> &tmp);
const char *status_text(int code, const dprf_doc *c = nullptr, size_t len = 0);
int convert_word(const dprf_doc *c, const uint8_t *w, size_t len, const uint8_t **out, size_t *olen,
                 std::vector<uint8_t> &tmp);
const char *word_text(const uint8_t *w, size_t len);
int check_power_space(uint64_t start, uint64_t count, int radix, int pwlen);
int check_slot(const char *what, uint64_t longest, const char *detail = "");

/* The device table of a mask (dprf_params.h) and what the host keeps of it; shared by dprf_search_mask and
 * dprf_search_hybrid.  npos may be 0 (a hybrid search of the bare word). */
struct mask_tab {
    std::vector<uint32_t> tab;
    uint32_t radix[DPRF_MAX_PW_RANGE];
    uint32_t npool = 0, sum_longest = 0;   /* pool entries in use; the sum over the positions of the longest symbol */
};
int mask_symbol(const dprf_doc *c, const uint8_t *b, size_t n, uint32_t &w, uint32_t &len, int pos, int k);
int build_mask_tab(const dprf_doc *c, const uint8_t *sym, const uint32_t *sym_off, const uint32_t *pos_off, int npos,
                   mask_tab &m);
unsigned __int128 mask_space(const uint32_t *radix, int npos);
uint64_t start_digits(uint64_t v, const uint32_t *radix, int npos, uint32_t *sdig);

int check_rules(const dprf_doc *c, const char *who, const uint32_t *fns, const uint32_t *rule_off, int64_t nrules,
                uint64_t start, uint64_t count);
uint32_t rules_longest(const dprf_doc *c, const uint32_t *fns, const uint32_t *rule_off, int64_t nrules);

/* What dprf_search_combine and dprf_spell_combine refuse alike (include/dprf.h "combinator mode"); `who` names the
 * export: a missing table, a window above nwords * nright (in 128 bits: DPRF_E_INVALID), and two longest words that do
 * not share a slot after the format's cut (DPRF_E_PWLEN). */
int check_combine(const dprf_doc *c, const char *who, uint64_t start, uint64_t count);
/* The longest candidate of a combinator window, after the cut (check_combine has bounded it by a slot) */
uint32_t combine_longest(const dprf_doc *c);

}   // namespace dprf_internal
#endif
