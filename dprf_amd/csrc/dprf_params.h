/* dprf_params.h -- kernel-argument structs shared by the host (dprf_host.cpp) and the gfx950 kernels
 * (dprf_kernels*.hip).  Plain C layout; everything a kernel needs about one document is folded here
 * once per context, never per candidate.  Word conventions: "BE" = the 32-bit big-endian words that
 * SHA-1/SHA-2/AES operate on; "LE" = little-endian words (MD5, RC4 byte order, candidate bytes). */
#ifndef DPRF_PARAMS_H
#define DPRF_PARAMS_H
#include <stdint.h>

#define DPRF_SLOT_WORDS 16          /* list-mode candidate slot: 64 bytes, LE-packed */
#define DPRF_MAX_RANGE_LEN 32
#define DPRF_R6_MAX_LONG 176        /* PDF R6 candidates: data[(128 + 64 + 48) * 64] holds 64 x (pw || K[0:64]) only up
                                       to 176 bytes (pdf...c:228); longer ones abort the reference (stack smashing) */

/* Candidate source for one launch.  Range mode: candidate g of the launch is global keyspace index
 * start + g, spelled over charset in itertools.product order.  List mode: candidate g is slot
 * start + g of the device candidate buffer.  Long-list mode (round 4): candidate g is record start + g of a packed
 * blob of candidates longer than a slot -- k_long_prehash hashes the record's first message (Office H0, the ODF
 * start key, PDF R5's whole hash, R6's K0) into `keys`, and the format's kernels continue from there. */
#define DPRF_ENUM_KEY40 3           /* dprf_enum.mode: the candidate is the key (dprf_search_key40): key g of the launch
                                       is the 40-bit index start + g, its five bytes big-endian; only start and count
                                       are read */
struct dprf_enum {
    uint64_t start;
    uint32_t count;
    uint32_t mode;                  /* 0 range, 1 list, 2 long list, 3 key (DPRF_ENUM_KEY40) */
    uint32_t pwlen;                 /* range: fixed length (bytes); list / long list: longest candidate of the launch */
    uint32_t cslen;
    uint32_t div_m;                 /* u32 division by cslen: q = (mulhi(n,m) + ((n-mulhi)>>1)) >> s */
    uint32_t div_s;
    uint8_t sdig[DPRF_MAX_RANGE_LEN];   /* base-cslen digits of start, most significant first */
    uint8_t charset[256];
    const uint32_t *slots;          /* list: [n][DPRF_SLOT_WORDS] LE words; long list: the record blob (LE words) */
    const uint8_t *lens;            /* list: [n] byte lengths */
    const uint64_t *loff;           /* long list: [n] word offset of each record in the blob (16-byte aligned)    */
    const uint32_t *llen;           /* long list: [n] byte length of each record                                  */
    uint32_t *keys;                 /* long list: [8][count] prehash output (chunk-local), read by the next kernel */
    /* multi-device stop_on_first calls only (round 6, dprf_hits.h), else null: host-mapped words */
    unsigned long long *hit_mirror;         /* this device lane's lowest hit, lowered by its kernels             */
    const unsigned long long *xfirst;       /* the lowest hit any device of the call has reported (host-kept)    */
};

/* Long-list prehash (k_long_prehash): the first message of the format's verify() over a record of any length. */
#define DPRF_LONG_SHA1_SALT16 1     /* Office H0 = SHA1(salt[0:16] || UTF16LE(pw)) (msoffcrypto...c:94-101) -> keys[5] */
#define DPRF_LONG_SHA256 2          /* ODF start key = SHA256(pw) (odt...c:78-79)                       -> keys[8] */
#define DPRF_LONG_SHA256_SALT8 3    /* R6 K0 = SHA256(pw || salt8) (pdf...c:240-245)                    -> keys[8] */
#define DPRF_LONG_R5 4              /* R5: SHA256(pw[:127] || salt8) == U[0:32] (pdf...c:194-221)       -> hits    */
struct dprf_long_params {
    uint32_t alg;                   /* DPRF_LONG_*                                                          */
    uint32_t prefix[4];             /* SHA1_SALT16: the salt as BE words (message words 0..3)               */
    uint32_t suffix[2];             /* SALT8 / R5: the 8 salt bytes as LE words, appended after the record  */
    uint32_t target[8];             /* R5: U[0:32] as BE words                                              */
};

/* Mask windows (dprf_search_mask, k_spell_mask): a table and a radix per position.  The device table is uploaded once
 * per call: DPRF_MASK_REC_WORDS words per position {radix, fastdiv magic m, shift s, base of the position's symbols in
 * the pool}, then the pool's LE-packed symbol words, then its byte counts (one byte per entry).  Positions with
 * identical symbol lists share one run of the pool.  Only the chunk start's digits change per launch: they travel in
 * the kernel arguments. */
#define DPRF_MASK_POOL 2048         /* = DPRF_MAX_MASK_SYMBOLS (include/dprf.h) */
#define DPRF_MASK_REC_WORDS 4
#define DPRF_MASK_POOL_AT (DPRF_MASK_REC_WORDS * DPRF_MAX_RANGE_LEN)
#define DPRF_MASK_LENS_AT (DPRF_MASK_POOL_AT + DPRF_MASK_POOL)
#define DPRF_MASK_TAB_WORDS (DPRF_MASK_LENS_AT + DPRF_MASK_POOL / 4)
struct dprf_mask_args {
    uint32_t count;                 /* candidates of the launch */
    uint32_t npos;                  /* positions, 1..DPRF_MAX_RANGE_LEN */
    uint32_t npool;                 /* pool entries in use, <= DPRF_MASK_POOL */
    uint32_t trunc;                 /* bytes at or past it are never written (PDF R2-R4 32, R5 127, else ~0) */
    uint32_t sdig[DPRF_MAX_RANGE_LEN / 4];  /* the chunk start's mixed-radix digits, one byte per position (position p
                                               in byte p % 4 of word p / 4) */
};

/* Hybrid windows (dprf_search_hybrid, k_spell_hybrid): a word of the context's table spelled before mask position
 * word_at, the word being one more digit at the most significant end of the mask's mixed radix.  The word table lives
 * on the device from dprf_ctx_set_words on: the converted bytes of all words packed back to back (each clipped to a
 * slot's 64 bytes), and nwords + 1 u32 byte offsets.  A block's 256 candidates use one contiguous run of at most
 * DPRF_HYB_RUN words, which the block stages into LDS (dprf_kernels_spell.hip, "the word run"): at most 16 KB of bytes,
 * read as whole u32 words from the word that holds the run's first byte (up to 3 bytes of lead-in, hence one word
 * more).  Rule windows stage the same run. */
#define DPRF_HYB_RUN 256
#define DPRF_HYB_RUN_WORDS (DPRF_HYB_RUN * DPRF_SLOT_WORDS + 1)
struct dprf_hybrid_args {
    dprf_mask_args m;               /* the mask part; npos may be 0 here (the bare word) */
    uint32_t word_at;               /* the word is spelled before mask position word_at, 0..npos */
    uint32_t w0;                    /* the chunk start's word index */
    uint32_t nwords;                /* words in the table (>= 1) */
    uint32_t bwords;                /* u32 words the device blob holds (the staging loads stay below it) */
};

/* Rule windows (dprf_search_rules / dprf_spell_rules, k_spell_rules): a rule of the call's rule table applied to a word
 * of the context's table.  The rule table is uploaded once per call: one u32 per function (the function's character in
 * bits 0-7, its parameters in bits 8-15 and 16-23) and nrules + 1 offsets.  Candidate g of a launch is rule
 * (r0 + g) % nrules applied to word w0 + (r0 + g) / nrules; r0 + g stays below 2^32. */
#define DPRF_RULE_FNS 32            /* = DPRF_MAX_RULE_FNS (include/dprf.h) */
struct dprf_rules_args {
    uint32_t count;                 /* candidates of the launch */
    uint32_t trunc;                 /* bytes at or past it are never written (PDF R2-R4 32, R5 127, else ~0) */
    uint32_t unit;                  /* bytes per unit: 1, or 2 for Office (UTF-16 code units) */
    uint32_t w0;                    /* the chunk start's word index */
    uint32_t r0;                    /* the chunk start's rule index, < nrules */
    uint32_t nrules;                /* rules in the table (>= 1) */
    uint32_t div_m, div_s;          /* u32 division by nrules (fastdiv_magic; unused for nrules = 1) */
    uint32_t nfns;                  /* function words the device table holds */
    uint32_t nwords;                /* words in the word table (>= 1) */
    uint32_t bwords;                /* u32 words the device blob holds (the staging loads stay below it) */
};

/* Combinator windows (dprf_search_combine / dprf_spell_combine, k_spell_combine): a word of the context's left table
 * (dprf_ctx_set_words) followed by a word of its right table (dprf_ctx_set_right_words), both stored on the device as the
 * hybrid table is.  Candidate g of a launch is left word l0 + (r0 + g) / nright followed by right word (r0 + g) %
 * nright; r0 + g stays below 2^32 (nright < 2^31, a launch holds at most 2^26 candidates). */
struct dprf_combine_args {
    uint32_t count;                 /* candidates of the launch */
    uint32_t trunc;                 /* bytes at or past it are never written (PDF R2-R4 32, R5 127, else ~0) */
    uint32_t l0;                    /* the chunk start's left word index */
    uint32_t r0;                    /* the chunk start's right word index, < nright */
    uint32_t nleft;                 /* words in the left table (>= 1) */
    uint32_t nright;                /* words in the right table (>= 1, < 2^31) */
    uint32_t div_m, div_s;          /* u32 division by nright (fastdiv_magic; unused for nright = 1) */
    uint32_t lbwords, rbwords;      /* u32 words the left / right device blob holds (the staging loads stay below) */
};

/* Device results of one API call (accumulated over its launches). */
struct dprf_results {
    uint32_t nhits;                 /* total hits (may exceed cap) */
    uint32_t stop;                  /* set by a hit when stop_on_first */
    uint32_t cursor;                /* work cursor of persistent kernels (PDF R6), reset per launch */
    uint32_t pad_;                  /* error flags set by a kernel, 0 = none: 1 PDF R6 scheduler watchdog, 2 / 4 / 8 an
                                       asm block's LDS-address assumption broken (R2-R4 S-box area, ODF check table,
                                       R6 tables) */
    unsigned long long first;       /* lowest hit index (atomicMin), ~0 if none */
    unsigned long long skipped;     /* candidates of launched chunks NOT evaluated: stop_on_first blocks
                                       skipped above the lowest hit (rare: one atomic per skipped block, none
                                       per evaluated block -- a per-block counter on this line made every
                                       block's `first` load wait behind the atomics, -25 % on PDF R2) */
    unsigned long long hits[1];     /* [cap] */
};

/* AES tables, generated on the host from the GF(2^8) definition (FIPS 197 5.1.1) and copied to LDS by
 * each kernel that needs them. */
struct dprf_aes_tables {
    uint32_t te0[256];              /* forward T-table, BE column (S[x]*{02,01,01,03}) */
    uint32_t td0[256];              /* inverse T-table, BE column (Si[x]*{0e,09,0d,0b}) */
    uint8_t sbox[256];
    uint8_t inv_sbox[256];
};

/* Office: msoffcrypto_password_verifier.c:56-191 */
struct dprf_office_params {
    uint32_t salt[4];               /* BE words of salt[0:16] (:95) */
    uint32_t ev[4];                 /* encrypted verifier, BE */
    uint32_t evh[8];                /* encrypted verifier hash (32 B), BE */
    uint32_t hash_size;             /* byte of dec(evh) that must be 0 (:168) */
};

/* Office 2010 / 2013 Agile Encryption, password key encryptor (MS-OFFCRYPTO 2.3.4.11-2.3.4.13; include/dprf.h) */
struct dprf_agile_params {
    uint32_t salt[4];               /* BE words of the 16 salt bytes: the first hash's prefix and both CBC IVs */
    uint32_t evi[4];                /* encryptedVerifierHashInput (16 B), BE */
    uint32_t evh[8];                /* encryptedVerifierHashValue[0:32], BE */
    uint32_t spin;                  /* spinCount */
    uint32_t sha512;                /* 0: SHA-1 ("2010"), 1: SHA-512 ("2013") */
    uint32_t key_words;             /* keyBits / 32: 4 or 8 */
};

/* Office 97-2003 RC4 and RC4 CryptoAPI (MS-OFFCRYPTO 2.3.6 / 2.3.5; include/dprf.h "Office 97-2003") */
#define DPRF_OLDOFFICE_REP_WORDS 96
struct dprf_oldoffice_params {
    uint32_t sha1;                  /* 0: types 0 / 1 (MD5), 1: types 3 / 4 (SHA-1) */
    uint32_t key_bytes;             /* SHA-1: 5 (type 3, zero-extended to a 16-byte RC4 key) or 16 (type 4) */
    uint32_t salt[4];               /* SHA-1: BE words of the 16 salt bytes, the first message's prefix */
    uint32_t ev[4];                 /* encryptedVerifier, LE words (RC4 byte order) */
    uint32_t evh[5];                /* encryptedVerifierHash, LE words: 4 used by MD5, 5 by SHA-1 */
    uint32_t rep[DPRF_OLDOFFICE_REP_WORDS]; /* MD5: the padded 336-byte message (h[0:5] || salt) x 16 as LE words of
                                               six blocks, zeros where the five hash bytes of each copy go */
};

/* ODT: odt_password_verifier.c:51-126 */
struct dprf_odt_params {
    uint32_t checksum[8];           /* BE */
    uint32_t iv[4];                 /* BE */
    uint32_t salt[4];               /* BE */
    uint32_t enc_len;               /* bytes; multiple of 16 */
    uint32_t hash_len;              /* min(enc_len, 1024) */
    const uint32_t *enc;            /* device: first hash_len bytes of ciphertext, BE words */
};

/* ODF 1.0 / 1.1: Blowfish-CFB, SHA-1 (include/dprf.h "ODF 1.0/1.1") */
#define DPRF_ODF_CONTENT_WORDS 256  /* the first 1024 bytes of the encrypted entry */
#define DPRF_ODF_X_WORDS (2 + DPRF_ODF_CONTENT_WORDS)
struct dprf_odf_params {
    uint32_t checksum[5];           /* SHA-1 of the first 1024 plaintext bytes, BE */
    uint32_t salt[4];               /* BE */
    uint32_t iterations;            /* PBKDF2 count, 1..DPRF_ODF_MAX_ITER */
    const uint32_t *x;              /* device: iv || content[0:1024] as DPRF_ODF_X_WORDS BE words.  CFB block i is
                                       pt_i = (x[2i + 2], x[2i + 3]) ^ E_key(x[2i], x[2i + 1]), i = 0..127 */
};

/* ODF 1.2 at the manifest's iteration count (include/dprf.h "$odf$*1*1*"): what k_odf_aes_kdf reads of the document.
 * The check is k_odt_check's, on a dprf_odt_params with enc_len = hash_len = 1024. */
struct dprf_odf_aes_params {
    uint32_t salt[4];               /* BE */
    uint32_t iterations;            /* PBKDF2 count, 1..DPRF_ODF_MAX_ITER */
};

/* PDF: pdf_password_verifier.c:64-291 */
#define DPRF_PDF_TAIL_WORDS 64
#define DPRF_PDF_OSUF_WORDS 14
struct dprf_pdf_params {
    uint32_t R;                     /* 2..6 */
    uint32_t n;                     /* Length / 8 (R<=4) */
    uint32_t u[12];                 /* R<=4: U[0:32] LE words; R5/R6: U[0:32] BE words + salt BE */
    uint32_t h2[4];                 /* R3/R4: MD5(PAD || ID), LE (pdf...c:167) */
    uint32_t pad[8];                /* the 32-byte password padding, LE */
    uint32_t tail_blocks;           /* MD5 blocks after the first (initial hash, :352-402) */
    uint32_t tail[DPRF_PDF_TAIL_WORDS]; /* LE words of O||LE32(P)||ID[||FFFFFFFF] + MD5 padding,
                                           starting at message byte 32 */
    /* owner-password check (dprf_ctx_set_pdf_password; include/dprf.h "owner password"), filled once by parse_pdf */
    uint32_t owner;                 /* 0: the launchers pick the user kernels, 1: the owner kernels */
    uint32_t o[8];                  /* R<=4: O[0:32] LE words (the RC4 ciphertext of the padded user password);
                                       R5/R6: O[0:32] BE words (the owner hash) */
    uint32_t osuf[DPRF_PDF_OSUF_WORDS]; /* R5/R6: O[32:40] || U[0:48], LE words: the 56 message bytes after the
                                           candidate in the owner hash's first message */
};

#endif
