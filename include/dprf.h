/* dprf.h -- C ABI of libdprf.so, the MI355X (gfx950) brute-force verification engine.
 *
 * Drop-in boundary.  The reference engine (/root/reference/src/brute_force.py) verifies one candidate
 * per OS process: _brute_force() (brute_force.py:106-161) Popen()s one of three verifier executables
 * per password (_call_msoffcrypto_core :163-173, _call_odt_core :175-182, _call_pdf_core :184-197)
 * whose exit code is verify()'s verdict (msoffcrypto_password_verifier.c:52, odt_password_verifier.c:47,
 * pdf_password_verifier.c:60).  This library replaces that inner loop, the three executables and the
 * OpenSSL arithmetic under them with batched gfx950 kernels, one candidate per lane.
 *
 * Plain C types only; no torch or HIP types cross the boundary.  Every call returns DPRF_OK (0) or a
 * negative DPRF_E_* code and sets a thread-local message readable with dprf_last_error().  An error is
 * never reported as "found" (the reference conflates the two: any non-zero exit counts as a hit,
 * brute_force.py:140).
 *
 * Threading: a context spans a list of devices (one or all of the node's GPUs) and owns one host worker
 * thread and one HIP stream per device for the duration of a call: dprf_search_range / dprf_verify_list
 * fan the call out over the devices inside the library (the reference's 4 worker processes on one queue,
 * brute_force.py:70-73 / :92-95, become one worker thread per GPU on one shared chunk cursor).  Calls on
 * DIFFERENT contexts may run concurrently from different threads; calls on the SAME context are
 * serialised by the library (a second caller waits for the first call to return).
 * Every entry point leaves the calling thread's current HIP device as it found it (ABI 5): the library sets the
 * device of each GPU it serves from the calling thread and restores the caller's on return, so a torch user's
 * default device (torch.cuda.current_device()) is not moved by a call (client.py:94-108 treats the verifier as a
 * pure call).
 * Ownership: the caller owns every buffer it passes; they are read/written only during the call.
 */
#ifndef DPRF_H
#define DPRF_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPRF_ABI_VERSION 9

/* formats: the tag parse_verification_data extracts (brute_force.py:250) */
#define DPRF_FMT_OFFICE 1   /* "$office$*2007*..."  ECMA-376 Standard Encryption; "$office$*2010*..." and
                               "$office$*2013*..." Agile Encryption (below); "$oldoffice$..."
                               Office 97-2003 RC4 / RC4 CryptoAPI (below)                    */
#define DPRF_FMT_ODT 2      /* "$odt$*1.2*..."      ODF 1.2 AES-256-CBC / PBKDF2-HMAC-SHA1;
                               "$odf$*0*0*..."      ODF 1.0 / 1.1 Blowfish-CFB, SHA-1 (below);
                               "$odf$*1*1*..."      ODF 1.2 at the manifest's PBKDF2 count (below)  */
#define DPRF_FMT_PDF 3      /* "$pdf$*V*R*..."      PDF standard security handler R2..R6       */

/* error codes */
#define DPRF_OK 0
#define DPRF_E_INVALID (-1)      /* bad argument / malformed field array                          */
#define DPRF_E_DOMAIN (-2)       /* stream outside the parity domain: the reference's behaviour is
                                    undefined or an abort() there           */
#define DPRF_E_HIP (-3)          /* HIP runtime error (message has the hipError string)           */
#define DPRF_E_NODEVICE (-4)     /* no usable gfx950 device / bad device ordinal                  */
#define DPRF_E_PWLEN (-5)        /* candidate too long: over DPRF_MAX_PW bytes (list mode; no argv string can carry
                                    it to the reference), or a range length over DPRF_MAX_PW_RANGE; owner mode
                                    (ABI 9): a PDF R5/R6 list candidate over the 64-byte slot; Office Agile and
                                    Office 97-2003: a list candidate of more than 32 UTF-16 units; ODF
                                    1.0 / 1.1: a list candidate over the 64-byte slot                 */
#define DPRF_E_CHARSET (-6)      /* range charset invalid: empty, NUL, a repeated byte, or a byte >= 0x80
                                    for Office (its candidates are UTF-16LE of characters); symbols
                                    (dprf_search_symbols): empty, repeated, with a NUL byte or over 4
                                    bytes, or for Office not one valid UTF-8 character; a mask
                                    (dprf_search_mask): the same per position, a position with no or
                                    over 256 symbols, or over DPRF_MAX_MASK_SYMBOLS symbols in all  */

#define DPRF_ALL_DEVICES (-1)    /* dprf_ctx_create device argument: every gfx950 device visible    */
#define DPRF_MAX_DEVICES 64

/* context flags (dprf_ctx_flags) */
#define DPRF_FLAG_NEVER_MATCHES 1        /* reference verify() returns 0 for every candidate: (V,R)
                                            gate / Length%8 (pdf...c:89-101), ev/evh length (office
                                            ...c:163,168).  Searches still run and find nothing.   */
#define DPRF_FLAG_REF_NONDETERMINISTIC 2 /* a hex field starts with 00: the reference's str_to_uchar
                                            (BN_hex2bn/BN_bn2bin) decodes it short and reads
                                            uninitialised bytes; this library decodes it in full.   */

/* List mode takes every candidate the reference's verifiers hash (ABI 5; ABI 4 capped them at a 64-byte slot):
 * ODF and Office any length (odt...c:79 hashes strlen(password); msoffcrypto...c:75,287-296 converts any length to
 * UTF-16LE), PDF R2-R4 truncated at 32 bytes (pdf...c:137), R5 at 127 (:197-206), R6 whole up to DPRF_MAX_PW_R6.
 * Candidates up to 64 bytes after conversion run in 64-byte slots; longer ones go to a long sub-list (k_long_prehash
 * hashes their first message, the format's kernels continue from it) -- same verdicts, same list indices.
 * DPRF_MAX_PW: the reference receives a candidate as one argv string, which Linux caps at MAX_ARG_STRLEN (131,072
 * bytes with the NUL): a longer one never reaches its verifier (DPRF_E_PWLEN).
 * DPRF_MAX_PW_R6: 64 x (pw || K[0:64]) fills the reference's data[(128 + 64 + 48) * 64] (pdf...c:228) at 176 bytes; a
 * longer R6 candidate overflows it and the reference aborts ("stack smashing detected", recorded in
 * tests/golden/long_verdicts.json) -- an error, not a verdict, so DPRF_E_DOMAIN. */
#define DPRF_MAX_PW 131071
#define DPRF_MAX_PW_R6 176
#define DPRF_MAX_PW_RANGE 32   /* longest fixed length for dprf_search_range */
#define DPRF_MAX_MASK_SYMBOLS 2048   /* dprf_search_mask: symbols of a mask's distinct per-position lists, summed */

typedef struct dprf_ctx dprf_ctx;

typedef struct dprf_stats {
    uint64_t candidates;   /* candidates fully evaluated on the device                          */
    uint64_t launches;     /* verification-kernel launches                                      */
    double kernel_ms;      /* sum of HIP-event durations of those launches (on the ctx stream)  */
    double wall_ms;        /* host wall time of the call, first launch to last result copy      */
    uint32_t stopped_early;/* 1 if stop_on_first ended the search before the whole range        */
    uint32_t devices;      /* devices that took part in the call (ABI 3; was `reserved`)        */
    double main_kernel_ms; /* HIP-event time of the dominant kernel alone: the KDF kernel for Office/ODF
                              (their check kernel follows it on the same stream), else = kernel_ms  (ABI 2) */
    double hit_ms;         /* host time from the call's start to when the library first knew of a hit, -1 if none
                              (ABI 6): wall_ms - hit_ms is how long the call ran on after its answer existed */
} dprf_stats;
/* kernel_ms / main_kernel_ms are summed over the devices of a multi-device call (device time); wall_ms is
 * the call's wall time.  candidates / launches are totals over the devices.  PDF R2-R4 alternate consecutive
 * launches between two streams per device, so a launch's event time includes the tail of its neighbour on the other
 * stream: their kernel_ms sum can exceed the device time (the library's own chunk sizing times those launches from
 * completion to completion instead). */

/* Per-device record of the last dprf_search_range / dprf_verify_list call on a context (ABI 4): how the shared
 * chunk cursor split the call, so imbalance between devices is visible (the sums above hide it). */
typedef struct dprf_device_stats {
    int32_t device;        /* HIP ordinal                                                              */
    uint32_t launches;     /* chunks this device took                                                  */
    uint64_t candidates;   /* candidates launched on it (before stop_on_first block skips)             */
    double kernel_ms;      /* HIP-event device time of its launches                                    */
    double first_ms;       /* host time from the call's start to its first launch                      */
    double finish_ms;      /* host time from the call's start to when its last launch was retired      */
    uint64_t evaluated;    /* candidates it verified: `candidates` minus the stop_on_first skips (ABI 6) */
} dprf_device_stats;

/* ---- library ---- */
int dprf_abi_version(void);
const char *dprf_last_error(void);
int dprf_device_count(void);      /* gfx950 devices visible to this process */
/* HIP ordinals of the visible gfx950 devices (a non-gfx950 device may sit at any ordinal): writes up to
 * cap ordinals, returns how many there are (ABI 3) */
int dprf_device_list(int *ordinals, int cap);
/* Fingerprint of the sources, Makefile flags and compiler this library was built from (ABI 4): bench.py prints
 * it and tools/prof_summary.py records it, so a profile can be matched to the build it measured. */
const char *dprf_build_id(void);
/* The multi-device chunk policy as a pure function (ABI 4; no device work, usable without a GPU): the size of the
 * next chunk a device of an `ndev`-device call takes from the shared cursor, for the kernel family `kernel`
 * (dprf_ctx_kernel's names), the device's measured rate (candidates per device-ms, 0 = not measured yet), the
 * candidates still unassigned (`remaining`) and the call's size (`total`).  A target-time size (a power of two,
 * ~0.1-3 s of device time by family), capped for ndev > 1 at remaining / (4 ndev) -- guided self-scheduling over
 * the two launches each device keeps in flight, so
 * the chunks shrink as the call runs out and the devices finish together -- but not below the family's tail
 * floor, nor below total / ndev for a call smaller than ndev floors (every device gets a share).  `inflight`: the
 * device's launches still running; with ndev > 1 a device that has one does not take ahead while the remaining
 * work is less than a chunk for every device -- the call returns 0 and the worker first waits for its launch.
 * Returns 0 for an unknown family too. */
uint64_t dprf_plan_chunk(const char *kernel, double rate_per_ms, uint64_t remaining, uint64_t total, int ndev,
                         int inflight);

/* ---- context: one document, one or more devices ----
 * fields/nfields: the array parse_verification_data() returns (brute_force.py:245-264), i.e. the
 * stream split on '*' with fields[0] replaced by the format tag ("office", "oldoffice", "odt", "odf" or "pdf"); office
 * needs 8 fields, oldoffice 5 (below), odt 7, odf 12 (below), pdf 12.  The per-format field meaning is exactly the reference's argv mapping
 * (brute_force.py:163-197).  device: HIP device ordinal, or DPRF_ALL_DEVICES for every gfx950 device. */
int dprf_ctx_create(const char *const *fields, int nfields, int device, dprf_ctx **out);
/* The same over an explicit device list (ABI 3).  An ordinal may repeat: {0,0} runs two streams and two
 * worker threads on device 0 (used to test the multi-device path on one GPU). */
int dprf_ctx_create_devices(const char *const *fields, int nfields, const int *devices, int ndev, dprf_ctx **out);
int dprf_ctx_devices(const dprf_ctx *ctx, int *ordinals, int cap);   /* returns the device count */
int dprf_ctx_destroy(dprf_ctx *ctx);
int dprf_ctx_format(const dprf_ctx *ctx);
int dprf_ctx_flags(const dprf_ctx *ctx);
const char *dprf_ctx_kernel(const dprf_ctx *ctx);   /* kernel family name, e.g. "pdf_r24" */
/* Per-device records of the context's last search / verify call (ABI 4): writes up to cap entries, returns the
 * number of devices of that call (0 before the first call). */
int dprf_ctx_last_call_devices(const dprf_ctx *ctx, dprf_device_stats *out, int cap);

/* ---- Office 2010 / 2013 Agile Encryption (MS-OFFCRYPTO 2.3.4.11-2.3.4.13, password key encryptor) ----
 * An office stream whose version field is exactly "2010" or "2013" is an Agile stream (office2john.py prints it for
 * every password-protected .docx / .xlsx / .pptx of Office 2010 and later); any other version field is read as the
 * 2007 Standard Encryption stream, as before.  Fields: ["office", version, spinCount, keyBits, saltSize, salt,
 * encryptedVerifierHashInput, encryptedVerifierHashValue[0:32]].  H = SHA-1 (20 bytes) for "2010", SHA-512 (64 bytes)
 * for "2013"; kb = keyBits / 8.
 *   h = H(salt || UTF16LE(pw));  for i in 0 .. spinCount-1: h = H(LE32(i) || h)
 *   key1 = H(h || fe a7 d2 76 3b 4b 9e 79), key2 = H(h || d7 aa 0f 6d 30 61 34 4e), each cut to kb bytes; where H is
 *   shorter than kb (SHA-1 with 256 bits) padded with 0x36 up to kb
 *   vin = AES-CBC-decrypt(key1, iv = salt, encryptedVerifierHashInput)           (16 bytes)
 *   vhv = AES-CBC-decrypt(key2, iv = salt, encryptedVerifierHashValue[0:32])     (32 bytes)
 *   the candidate verifies when H(vin)[0:n] == vhv[0:n], n = 20 for "2010", 32 for "2013"
 * There is no reference verifier for this format; the definition is pinned by the public example hashes of hashcat
 * modes 9500 / 9600 (tests/golden/agile_vectors.json).  Accepted domain, anything else DPRF_E_DOMAIN with a message
 * naming the field: spinCount decimal in 0..DPRF_AGILE_MAX_SPIN; keyBits 128 or 256 (no AES-192); saltSize 16 with 32
 * hex digits of salt; 32 hex digits of encryptedVerifierHashInput; 64 of encryptedVerifierHashValue.  An Agile context
 * sets no flag.  dprf_ctx_kernel returns "office_agile_sha1" or "office_agile_sha512", families dprf_plan_chunk knows:
 * a caller detects Agile support with dprf_plan_chunk("office_agile_sha512", 0, 1, 1, 1, 0) != 0 (DPRF_ABI_VERSION is
 * unchanged: no export or struct changed).  Range, symbol, mask and list modes work as for the 2007 stream (ASCII
 * range charset, one valid UTF-8 character per symbol, empty or invalid UTF-8 list candidate DPRF_E_DOMAIN), except
 * that a list candidate of more than 32 UTF-16 units (the 64-byte slot) is DPRF_E_PWLEN, reported per candidate by
 * dprf_list_status: long Agile candidates are not supported yet. */
#define DPRF_AGILE_MAX_SPIN 10000000

/* ---- Office 97-2003 binary documents: RC4 (MS-OFFCRYPTO 2.3.6) and RC4 CryptoAPI (2.3.5) ----
 * The stream office2john.py prints for a password-protected .doc / .xls: "$oldoffice$<type>*salt*ev*evh" (hashcat and
 * current John write "$oldoffice$*<type>*..."; parse_verification_data takes both).  dprf_ctx_create takes
 * fields[0] == "oldoffice" with nfields == 5: ["oldoffice", type, salt, encryptedVerifier, encryptedVerifierHash] --
 * salt and encryptedVerifier 32 hex digits each, encryptedVerifierHash 32 hex digits for types 0 / 1 and 40 for types
 * 3 / 4.  dprf_ctx_format returns DPRF_FMT_OFFICE (the reference's document type 1; candidates are UTF-16 units as for
 * the other Office streams).  pw16 is the candidate in UTF-16LE, no terminator, no truncation; RC4 is one continuous
 * keystream over both encrypted fields.
 *   types 0, 1 (RC4, 40 bits of key material; the type only records the container, .xls / .doc):
 *     h = MD5(pw16)
 *     h = MD5((h[0:5] || salt) x 16)                              (336 bytes)
 *     k = MD5(h[0:5] || 00 00 00 00)                              (block 0; all 16 bytes are the RC4 key)
 *     d = RC4(k, encryptedVerifier || encryptedVerifierHash)      (32 bytes)
 *     the candidate verifies when MD5(d[0:16]) == d[16:32]
 *   types 3, 4 (RC4 CryptoAPI, 40-bit / 128-bit key):
 *     h = SHA1(salt || pw16)
 *     k = SHA1(h || 00 00 00 00)                                  (block 0)
 *     key = k[0:5] || eleven 00 bytes (type 3: a 16-byte RC4 key, not a 5-byte one)   or   k[0:16] (type 4)
 *     d = RC4(key, encryptedVerifier || encryptedVerifierHash)    (36 bytes)
 *     the candidate verifies when SHA1(d[0:16]) == d[16:36]
 * All 16 / 20 bytes are compared.  In types 0 / 1 only 40 bits of the first hash survive, so distinct passwords can
 * verify: a search may return more than one hit.
 * There is no reference verifier for this stream; the definition is pinned by the public example hashes of hashcat
 * modes 9700 / 9800 (tests/golden/oldoffice_vectors.json: types 1 and 3).  No public type-4 vector is known: type 4
 * differs from type 3 in the key cut alone and rests on the specification text.
 * Accepted domain, anything else DPRF_E_DOMAIN with a message naming the field: type "0", "1", "3" or "4"; the three
 * hex fields of exactly the lengths above.  Such a context sets no flag; dprf_ctx_set_pdf_password on it is
 * DPRF_E_INVALID.  dprf_ctx_kernel returns "office_rc4_md5" (types 0, 1) or "office_rc4_sha1" (types 3, 4), families
 * dprf_plan_chunk knows: a caller detects the support with dprf_plan_chunk("office_rc4_md5", 0, 1, 1, 1, 0) != 0
 * (DPRF_ABI_VERSION is unchanged: no export or struct changed).  Range, symbol, mask, list, hybrid and rule modes work
 * as for the 2007 stream (ASCII range charset, one valid UTF-8 character per symbol, empty or invalid UTF-8 list
 * candidate DPRF_E_DOMAIN), except that a list candidate of more than 32 UTF-16 units (the 64-byte slot) is
 * DPRF_E_PWLEN, reported per candidate by dprf_list_status: long Office 97-2003 candidates are not supported yet.
 * Types 0, 1 and 3 carry 40 bits of RC4 key: dprf_search_key40 (below, "40-bit key search") searches the keys themselves,
 * and dprf_ctx_set_key40 ("password for a known key") turns a found key into a password.
 * Not done: PowerPoint 97-2003 (.ppt), XOR obfuscation, list candidates over 32 UTF-16 units, John's type 5, decrypting
 * the document body. */

/* ---- ODF 1.0 / 1.1: Blowfish in CFB mode, SHA-1 (OpenOffice.org, StarOffice, Apache OpenOffice, LibreOffice < 3.5
 * and its "ODF 1.0/1.1" setting) ----
 * The stream odt2hashes.py prints for a package whose manifest names the algorithm "Blowfish CFB"; it is the one John's
 * odf2john and hashcat mode 18600 use:
 *   $odf$*0*0*<iterations>*16*<checksum, 40 hex>*8*<iv, 16 hex>*16*<salt, 32 hex>*0*<content, 2048 hex>
 * cipher 0 = Blowfish, checksum type 0 = SHA-1, key size 16, IV length 8, salt length 16, the "inplace" flag 0, and the
 * first 1024 bytes of the encrypted entry.  dprf_ctx_create takes fields[0] == "odf" with nfields == 12: ["odf", "0",
 * "0", iterations, "16", checksum, "8", iv, "16", salt, "0", content] (parse_verification_data cuts a ":::" tail off
 * the last field).  dprf_ctx_format returns DPRF_FMT_ODT (the reference's document type 2; candidates are raw bytes,
 * as for the ODF 1.2 stream).
 *   sk  = SHA1(pw)                                   pw: the candidate's bytes as given (UTF-8)
 *   key = PBKDF2-HMAC-SHA1(P = sk (20 bytes), S = salt, c = iterations, dkLen = 16)        (one output block)
 *   pt  = Blowfish-CFB64-decrypt(key (16 bytes), iv, content[0:1024]):
 *         pt_i = ct_i XOR E_key(ct_(i-1)), ct_(-1) = iv, 128 blocks of 8 bytes, big-endian halves
 *   the candidate verifies when SHA1(pt) == checksum, all 20 bytes
 * CFB decryption uses Blowfish's encrypt direction only, and every E_key input is a constant of the document.
 * There is no reference verifier for this stream and no public test vector of it is at hand: the definition rests on
 * tests/odf_legacy_model.py -- hashlib's SHA-1 and PBKDF2, and a Blowfish of its own whose initial words (the digits
 * of pi, computed there), key schedule and CFB output are checked against libcrypto (BF_set_key, BF_cfb64_encrypt) and
 * Schneier's zero-key vector.
 * Accepted domain, anything else DPRF_E_DOMAIN with a message naming the field: cipher "0" and checksum type "0"; key
 * size "16", IV length "8", salt length "16", inplace "0"; the hex fields of exactly the lengths above; iterations a
 * decimal in 1..DPRF_ODF_MAX_ITER (a kernel argument; real files say 1024).  The AES spelling of the same stream,
 * "$odf$*1*1*...", is the next section's; the mixed pairs (cipher 1 with checksum type 0, and the reverse) are
 * refused.  Such a context sets no
 * flag; dprf_ctx_set_pdf_password on it is DPRF_E_INVALID.  dprf_ctx_kernel returns "odf_bf_sha1", a family
 * dprf_plan_chunk knows: a caller detects the support with dprf_plan_chunk("odf_bf_sha1", 0, 1, 1, 1, 0) != 0
 * (DPRF_ABI_VERSION is unchanged: no export or struct changed).  Range, symbol, mask, list, hybrid and rule modes work
 * as for the "$odt$" stream (raw bytes, rule unit = byte), except that a list candidate over the 64-byte slot is
 * DPRF_E_PWLEN, reported per candidate by dprf_list_status: long ODF 1.0/1.1 candidates are not supported yet.
 * Not done: content shorter than 1024 bytes (old OpenOffice builds wrote a defective SHA-1 for some lengths),
 * StarOffice / OpenOffice.org 1.x packages (.sxw, .sxc), candidates over 64 bytes, decrypting the document (the
 * "$odf$*1*1*" spelling is done: below). */
#define DPRF_ODF_MAX_ITER 10000000

/* ---- ODF 1.2 at the manifest's iteration count: AES-256-CBC, SHA-256, PBKDF2 with any count (LibreOffice 3.5 to
 * 5.x wrote 1024, LibreOffice since then writes 100000) ----
 * The "$odt$" stream above has no field for the PBKDF2 count, and the reference verifier runs 1024 whatever the manifest
 * says (odt_password_verifier.c:85).  The stream that carries the count is the AES spelling of the stream of the last
 * section, John's odf2john / hashcat mode 18400; odt2hashes.py prints it for an AES-256-CBC package whose count is not
 * 1024:
 *   $odf$*1*1*<iterations>*32*<checksum, 64 hex>*16*<iv, 32 hex>*16*<salt, 32 hex>*0*<content, 2048 hex>
 * cipher 1 = AES-256-CBC, checksum type 1 = SHA-256, key size 32, IV length 16, salt length 16, inplace 0, and the first
 * 1024 bytes of the encrypted entry.  dprf_ctx_create takes fields[0] == "odf" with nfields == 12: ["odf", "1", "1",
 * iterations, "32", checksum, "16", iv, "16", salt, "0", content].  dprf_ctx_format returns DPRF_FMT_ODT.
 *   sk  = SHA256(pw)                                   pw: the candidate's bytes as given
 *   key = PBKDF2-HMAC-SHA1(P = sk (32 bytes), S = salt, c = iterations, dkLen = 32)        (two output blocks)
 *   pt  = AES-256-CBC-decrypt(key, iv, content[0:1024])
 *   the candidate verifies when SHA256(pt) == checksum, all 32 bytes
 * At iterations = 1024 this is the "$odt$" stream's check of a document of at least 1024 encrypted bytes, and the two
 * contexts report the same hits.  No public test vector of this stream is at hand: the definition rests on the model of
 * tests/test_odf12_iter_model.py (hashlib's SHA-256 and PBKDF2, the test generator's AES-CBC), whose verdicts at
 * iterations = 1024 equal the oracle's and the reference verifier's on the "$odt$" stream of the same document.
 * Accepted domain, anything else DPRF_E_DOMAIN with a message naming the field (and, since the reference's own spelling
 * of such a document is "$odt$", saying so): key size "32", IV length "16", salt length "16", inplace "0"; the hex
 * fields of exactly the lengths above; iterations a decimal in 1..DPRF_ODF_MAX_ITER (a kernel argument).  Such a
 * context sets no flag.  dprf_ctx_kernel returns "odf_aes_sha256", a family dprf_plan_chunk knows: a caller detects the
 * support with dprf_plan_chunk("odf_aes_sha256", 0, 1, 1, 1, 0) != 0 (DPRF_ABI_VERSION is unchanged: no export or struct
 * changed).  dprf_plan_chunk answers for 1024 iterations; a context plans its own launches by its count (the first
 * launch, the floor and the tail are the row's times 1024 / iterations, never below one resident generation of the KDF
 * kernel).  Range, symbol, mask, list, hybrid and rule modes work as for the "$odt$" stream (raw bytes, rule unit =
 * byte), list candidates of any length included.
 * Not done: Argon2id key derivation and AES-256-GCM (LibreOffice 24.2's optional "wholesome" encryption), content shorter
 * than 1024 bytes, decrypting the document. */

/* ---- owner password (ABI 9): which of a PDF's two passwords the searches verify ----
 * A PDF carries a user password (opens the document) and an owner password (lifts the print / copy / edit
 * restrictions; often the only one set).  A context verifies the user password (/U: pdf...c:115-191) unless the owner
 * check is selected here; from then on dprf_search_range, dprf_search_symbols, dprf_search_mask and dprf_verify_list
 * verify the chosen password, with hit indices, stop_on_first, multi-device chunks, the cross-device stop, stats and
 * dprf_list_status as before.  Selecting DPRF_PDF_USER again restores the user check exactly.  The setter takes the
 * context's call mutex (it waits for a running call).
 *
 * The reference has no owner verifier ("Further work", pdf...c:20; its R6 hash takes an ownerkey it always passes as
 * NULL); the owner check is ISO 32000-1 Algorithms 3 and 7 and ISO 32000-2 Algorithms 12 and 2.B, with the byte
 * truncation the user check of the same revision applies.  PAD is the 32-byte padding string.
 *   R2-R4  h = MD5((pw[:32] || PAD)[:32]); for R >= 3, 50 x h = MD5(h) over ALL 16 bytes whatever Length is (the user
 *          key's rounds hash h[0:n]); key = h[0:n], n = 5 for R2, else Length / 8.
 *          R2: x = RC4(key, O[0:32]).  R3/R4: x = O[0:32], then for i = 19 down to 0: x = RC4(key XOR i, x).
 *          x is a padded user password: the candidate verifies exactly when x passes the user check as a 32-byte
 *          candidate -- the same initial MD5 over x || O || P || ID [|| FFFFFFFF], the same 50 rounds over h[0:n], the
 *          same RC4 passes, the same compare (32 bytes of U for R2, 16 for R3/R4).  x may hold any byte, 0x00 included;
 *          it never leaves the device.
 *   R5     SHA-256(pw[:127] || O[32:40] || U[0:48]) == O[0:32].
 *   R6     the hardened hash (pdf...c:226-291) with validation salt O[32:40] and udata = U[0:48]:
 *          K = SHA-256(pw || salt || udata), every round's data = 64 x (pw || K[0:bs] || udata); result == O[0:32].
 *          The password is hashed whole, as in user mode.
 * Errors (neither changes the mode): DPRF_E_INVALID -- the context is not PDF, or `which` is unknown; DPRF_E_DOMAIN --
 * O shorter than 32 bytes (R2-R4), or O or U shorter than 48 bytes (R5/R6; the user check needs 40 bytes of U only).
 * A DPRF_FLAG_NEVER_MATCHES context stays never-matching.  In owner mode dprf_ctx_kernel returns "pdf_r24_owner",
 * "pdf_r5_owner" or "pdf_r6_owner", families dprf_plan_chunk knows (the user family's policy, first chunk halved).
 * Candidate lengths in owner mode: range, symbols and mask as before; list mode R2-R4 as before (first 32 bytes); list
 * mode R5/R6 up to the 64-byte slot -- a longer candidate is DPRF_E_PWLEN (dprf_list_status reports it per candidate):
 * long owner candidates are not supported yet (the long-list prehash appends the 8 salt bytes, not salt || U[0:48]). */
#define DPRF_PDF_USER 0
#define DPRF_PDF_OWNER 1
int dprf_ctx_set_pdf_password(dprf_ctx *ctx, int which);   /* default DPRF_PDF_USER */
int dprf_ctx_pdf_password(const dprf_ctx *ctx);

/* ---- range mode: brute_force.py -pr N (init_rangebased_brute_force :60-79, _generate :199-219) ----
 * Verifies candidates [start, start+count) of charset^pwlen in itertools.product order (leftmost
 * character most significant).  The symbols are the charset's BYTES, all distinct (a repeated byte would
 * verify candidates twice: DPRF_E_CHARSET): for PDF and ODF a byte >= 0x80 is a raw candidate byte, as the
 * reference's argv carries it; Office takes ASCII only.  A caller whose alphabet has multi-byte UTF-8
 * characters uses dprf_search_symbols.
 * Writes up to `cap` hit indices, ascending, to hits[]; *nhits = total number of hits found (may exceed cap).
 * stats may be NULL.
 * Multi-device: the devices take contiguous chunks of the range from one shared cursor in increasing
 * order (chunks sized for ~0.1-1 s of device time at the rate measured on that device), so a fast device
 * takes more and every index below the last chunk taken is covered.
 * stop_on_first != 0: the search ends once no unverified index lies below the lowest hit found so far;
 * hits[0] is then the LOWEST verifying index of the whole range, unconditionally (every candidate below
 * it is verified on some device; a kernel block is skipped only if its lowest index is above it).  A
 * multi-device call pushes a hit to the launches already running on the other devices (ABI 6): a host thread
 * polls every lane's host-mapped hit word and publishes the minimum to a word every launch reads beside its own
 * device's (dprf_hits.h), so their blocks above it skip within ~0.2 ms -- as the reference's workers stop at
 * their next candidate once `found` is set (brute_force.py:111-114, :140-147).  The same holds in list mode. */
int dprf_search_range(dprf_ctx *ctx, const uint8_t *charset, int cslen, int pwlen, uint64_t start,
                      uint64_t count, int stop_on_first, uint64_t *hits, int64_t cap, int64_t *nhits,
                      dprf_stats *stats);

/* ---- range mode over multi-byte symbols (ABI 7): a --charset with non-ASCII characters ----
 * Verifies indices [start, start+count) of sym^pwlen in itertools.product order over SYMBOLS (the last position
 * fastest, brute_force.py:205), symbol k being the bytes sym[sym_off[k] .. sym_off[k+1]) -- a charset's characters
 * in UTF-8, each 1-4 bytes, all distinct, no NUL byte (DPRF_E_CHARSET).  For Office each symbol must be one valid
 * UTF-8 character and goes in as its UTF-16LE, as iconv converts the whole password (msoffcrypto...c:275-336).  The
 * device spells every candidate into a list slot and the list-mode kernels verify it: a candidate's bytes are the
 * concatenation of its symbols' (PDF R2-R4 hash the first 32, pdf...c:137).  DPRF_E_PWLEN: pwlen outside
 * 1..DPRF_MAX_PW_RANGE, or a candidate could exceed a 64-byte slot after conversion and truncation (the caller
 * spells such windows itself and uses dprf_verify_list).  hits[] are indices relative to `start`; the rest is as
 * dprf_search_range (stop_on_first, multi-device chunks and the cross-device stop). */
int dprf_search_symbols(dprf_ctx *ctx, const uint8_t *sym, const uint32_t *sym_off, int nsym, int pwlen,
                        uint64_t start, uint64_t count, int stop_on_first, uint64_t *hits, int64_t cap,
                        int64_t *nhits, dprf_stats *stats);

/* ---- mask mode (ABI 8): a symbol list per position ("?u?l?l?l?d?d", "Inv-?d?d?d?d") ----
 * Verifies indices [start, start+count) of the product of npos symbol lists in itertools.product order (the last
 * position fastest): position p takes the symbols pos_off[p] .. pos_off[p+1]) of one flat list (npos+1 offsets), and
 * symbol k of that list is the bytes sym[sym_off[k] .. sym_off[k+1]).  A literal is a position of one symbol.  With
 * the same list at every position the enumeration is dprf_search_symbols'.  The symbol rules are dprf_search_symbols',
 * per position: 1-4 bytes, no NUL, distinct within the position (the same symbol may appear at several positions),
 * for Office one valid UTF-8 character each, which goes in as its UTF-16LE.
 * DPRF_E_CHARSET: a broken symbol rule, a position with no symbol or with more than 256, or more than
 * DPRF_MAX_MASK_SYMBOLS symbols in all once positions with identical lists are counted once.
 * DPRF_E_PWLEN: npos outside 1..DPRF_MAX_PW_RANGE, or the longest candidate -- the sum over the positions of the
 * position's longest symbol, after the format's truncation (PDF R2-R4 32 bytes, R5 127) -- exceeds a 64-byte slot.
 * DPRF_E_INVALID: start + count exceeds the keyspace, the product of the positions' symbol counts (computed without
 * wrapping: a keyspace of 2^64 or more takes any window below 2^64).
 * The device spells every candidate into a list slot (k_spell_mask) and the list-mode kernels verify it; the
 * position records and the symbol pool go to each device once per call, and only the chunk start's mixed-radix digits
 * change per launch.  hits[] are indices relative to `start`; stop_on_first, multi-device chunks and the cross-device
 * stop are as dprf_search_range's. */
int dprf_search_mask(dprf_ctx *ctx, const uint8_t *sym, const uint32_t *sym_off, const uint32_t *pos_off, int npos,
                     uint64_t start, uint64_t count, int stop_on_first, uint64_t *hits, int64_t cap,
                     int64_t *nhits, dprf_stats *stats);

/* ---- list mode: client payloads (init_listbased_brute_force :82-104, client.py:105) ----
 * Candidate k is blob[offsets[k] .. offsets[k+1]) (n+1 offsets).  Hits are list indices. */
int dprf_verify_list(dprf_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, int64_t n,
                     int stop_on_first, uint64_t *hits, int64_t cap, int64_t *nhits, dprf_stats *stats);
/* dprf_verify_list rejects the whole call if one candidate is one the reference cannot verify (NUL; empty or
 * invalid-UTF-8 Office password; PDF R6 over DPRF_MAX_PW_R6 bytes: DPRF_E_DOMAIN / DPRF_E_INVALID; over DPRF_MAX_PW
 * bytes: DPRF_E_PWLEN).  This host-only check (no
 * device work) writes 0 or that DPRF_E_* code per candidate to status[n] (may be NULL) and returns the
 * number of invalid candidates, so a caller can drop them and verify the rest -- the reference fails
 * such a candidate alone, in its own verifier process (brute_force.py:163-197).  (ABI 3) */
int dprf_list_status(const dprf_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, int64_t n, int8_t *status);

/* ---- hybrid mode: a word table times a mask ("Summer" x "?w?d?d?d?d!", "?d?d?d?d-?w") ----
 * Additive to ABI 9 (no struct or earlier export changes, DPRF_ABI_VERSION stays 9): a caller detects it by looking
 * the symbol dprf_search_hybrid up.
 *
 * The table: word k is blob[offsets[k] .. offsets[k+1]) (n+1 offsets), in the caller's order; a word may repeat (a
 * wordlist's duplicates are verified twice).  dprf_ctx_set_words validates and converts all words once -- Office:
 * UTF-8 to UTF-16LE, any number of characters; the other formats: the bytes as given -- and uploads the table to
 * every device of the context, where it stays until it is replaced, cleared (n = 0) or the context is destroyed.  It
 * waits for a call in flight on the context, like dprf_ctx_set_pdf_password.  The whole table is refused, and the
 * previous one stays, on: an empty word, a word with a NUL byte, an Office word that is not valid UTF-8
 * (DPRF_E_DOMAIN); n >= 2^32 or converted words of 2^32 bytes or more in all (DPRF_E_INVALID).  The message names the
 * first offending word's index.  dprf_words_status is the host-only check of the same rules: 0 or the DPRF_E_* code
 * per word into status[n] (may be NULL), returning the number of refused words, so a caller can drop them and keep
 * the rest.  dprf_ctx_words returns the number of words held (0: no table). */
int dprf_ctx_set_words(dprf_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, int64_t n);
int64_t dprf_ctx_words(const dprf_ctx *ctx);
int dprf_words_status(const dprf_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, int64_t n, int8_t *status);

/* The search: a mask of npos positions, 0 <= npos <= DPRF_MAX_PW_RANGE, given and checked as dprf_search_mask's
 * (with npos = 0 the three mask arguments may be NULL), of keyspace M = the product of the positions' symbol counts
 * (1 for npos = 0); word_at in 0..npos says before which mask position the word is spelled: 0 prepends it, npos
 * appends it.  Candidate i of the keyspace N * M (N words) is word i / M with mask index i % M, the mask part spelled
 * as dprf_search_mask spells it (the last position fastest): the word is the slowest digit wherever it stands.  The
 * bytes are the concatenation in spelling order, and the format's truncation applies to the whole candidate (PDF
 * R2-R4 32 bytes, R5 127).
 * Errors beyond dprf_search_mask's: DPRF_E_INVALID -- no table set, word_at outside 0..npos, or start + count above
 * N * M (computed without wrapping); DPRF_E_PWLEN -- min(the longest converted word + the sum over the positions of
 * the position's longest symbol, the truncation) exceeds a 64-byte slot (the message names the word).  Where the
 * truncation is at most 64 bytes (R2-R4) a word of any length is accepted.  A refused call leaves no per-device
 * record, and the context still serves.
 * The device spells every candidate into a list slot (k_spell_hybrid) from the table it holds; per call only the mask
 * table goes up, per launch only the chunk start's word index and mask digits.  hits[] relative to `start`,
 * stop_on_first (the lowest verifying index), multi-device chunks, the cross-device stop, stats, owner mode and
 * DPRF_FLAG_NEVER_MATCHES contexts are as dprf_search_mask's.  Long candidates stay unsupported for Agile and owner
 * R5/R6 as above: they do not fit the slot. */
int dprf_search_hybrid(dprf_ctx *ctx, const uint8_t *sym, const uint32_t *sym_off, const uint32_t *pos_off, int npos,
                       int word_at, uint64_t start, uint64_t count, int stop_on_first, uint64_t *hits, int64_t cap,
                       int64_t *nhits, dprf_stats *stats);

/* ---- rule mode: a word table times word-mangling rules ("password" -> "Password1", "p@ssw0rd", "drowssap") ----
 * Additive to ABI 9 (DPRF_ABI_VERSION stays 9): a caller detects it by looking the symbol dprf_search_rules up.
 *
 * The language.  A rule is a sequence of 1..DPRF_MAX_RULE_FNS functions applied left to right to a word of the
 * context's table (dprf_ctx_set_words).  A word is a sequence of units: for ODF and PDF a unit is a byte of the word as
 * given, for Office (2007 and Agile) a UTF-16 code unit of the converted word.  LIMIT is 64 units for ODF and PDF and
 * 32 units for Office: the 64-byte list slot.  The format's truncation applies to the result (PDF R2-R4 cut at 32
 * bytes, R5 at 127).  Case functions touch ASCII letters only, in both unit widths.  A rule that splits a surrogate
 * pair yields a candidate that no typed password spells; it is verified like any other candidate.
 * Two rules hold for every function: a function whose result would be longer than LIMIT leaves the candidate
 * unchanged, and so does a function whose result would be empty.  Together they keep every candidate at 1..LIMIT
 * units with no NUL, as dprf_ctx_set_words guarantees for the words.
 * N and M are positions, written 0-9A-Z in rule text, with the values 0..35; X and Y are one unit given as one byte,
 * 0x01..0xFF (Office: 0x01..0x7F, which becomes that UTF-16 unit).  w is the candidate, n its length, w[a:b] a
 * half-open slice, rev reversal; a function whose condition does not hold leaves the candidate unchanged:
 *   :        w                                    l / u    A-Z -> a-z / a-z -> A-Z in every unit
 *   c / C    l then unit 0 upper-cased / u then unit 0 lower-cased
 *   t        toggle the case of every letter      TN       toggle unit N, if N < n
 *   E        l, then upper-case unit 0 and every unit that follows a 0x20
 *   r        rev w                                d        w + w
 *   pN       w repeated N + 1 times               f        w + rev w
 *   {  /  }  w[1:n] + w[0:1]  /  w[n-1:n] + w[0:n-1]
 *   q        every unit twice                     k / K    swap units 0, 1 / units n-2, n-1, if n >= 2
 *   *NM      swap units N and M, if N < n and M < n
 *   $X / ^X  w + X / X + w                        [ / ]    w[1:n] / w[0:n-1]
 *   DN       delete unit N, if N < n              xNM      w[N:N+M], if N + M <= n
 *   ONM      w[0:N] + w[N+M:n], if N + M <= n     iNX      w[0:N] + X + w[N:n], if N <= n
 *   oNX      unit N := X, if N < n                'N       w[0:N], if N < n
 *   zN / ZN  w[0] x N + w  /  w + w[n-1] x N
 *   yN / YN  w[0:N] + w  /  w + w[n-N:n], if N <= n
 *   sXY      every unit equal to X becomes Y      @X       every unit equal to X is deleted
 *   .N / ,N  unit N := unit N+1, if N + 1 < n  /  unit N := unit N-1, if 1 <= N < n
 * These are hashcat's functions of the same names; its reject, memory and arithmetic functions are not included.
 *
 * The compiled form: one uint32 per function -- the function's own ASCII character in bits 0-7, the first parameter in
 * bits 8-15, the second in bits 16-23 (N and M as their values, X and Y as the byte), everything else 0.  Rule k is
 * fns[rule_off[k] .. rule_off[k+1]) (nrules + 1 offsets).  Candidate i of the keyspace N * R (N words, R rules) is
 * rule i % R applied to word i / R: the word is the slowest digit, as in hybrid mode.
 *
 * dprf_search_rules verifies indices [start, start + count).  The rule table goes to each device once per call, per
 * launch only the chunk start's word and rule index; the device applies the rules (k_spell_rules) and the list-mode
 * kernels verify the slots.  hits[] relative to `start`, stop_on_first (the lowest verifying index), multi-device
 * chunks, the cross-device stop, stats, owner mode, DPRF_FLAG_NEVER_MATCHES contexts and the per-device records are
 * as dprf_search_hybrid's.
 * dprf_spell_rules writes the candidates themselves: slot k of slots[count * 64] holds the bytes of candidate start + k
 * after the format's cut (Office: UTF-16LE), zero-padded, and lens[k] their number -- exactly what a search would
 * verify, spelled by the same kernel on the context's first device; no verification kernel runs.  count <= 2^20.
 * Errors (a refused call leaves no per-device record, and the context still serves):
 * DPRF_E_INVALID -- a null argument, no word table, nrules outside 1..DPRF_MAX_RULES, offsets not ascending, a rule of
 * 0 or more than DPRF_MAX_RULE_FNS functions, more than DPRF_MAX_RULE_WORDS functions in all, start + count above
 * N * R (computed without wrapping); for dprf_spell_rules also count above 2^20 or a never-matching context.
 * DPRF_E_CHARSET (the message names the rule and the function) -- an unknown function byte, a position over 35, an X
 * or Y of 0, for Office an X or Y of 0x80 or more, non-zero unused parameter bits.
 * DPRF_E_PWLEN (the message names the word) -- the table's longest converted word exceeds 64 bytes, for every family
 * including PDF R2-R4: a rule may move a word's tail to the front, so a clipped copy is not enough. */
#define DPRF_MAX_RULES      (1 << 20)   /* rules per call                       */
#define DPRF_MAX_RULE_FNS   32          /* functions per rule                   */
#define DPRF_MAX_RULE_WORDS (1 << 22)   /* encoded functions per call, in all   */
int dprf_search_rules(dprf_ctx *ctx, const uint32_t *fns, const uint32_t *rule_off, int64_t nrules, uint64_t start,
                      uint64_t count, int stop_on_first, uint64_t *hits, int64_t cap, int64_t *nhits,
                      dprf_stats *stats);
int dprf_spell_rules(dprf_ctx *ctx, const uint32_t *fns, const uint32_t *rule_off, int64_t nrules, uint64_t start,
                     uint64_t count, uint8_t *slots, uint8_t *lens);

/* ---- combinator mode: a word table times a second word table ("summer" + "2024", "Anna" + "Maria") ----
 * Additive to ABI 9 (DPRF_ABI_VERSION stays 9): a caller detects it by looking the symbol dprf_search_combine up.
 * This is hashcat's -a 1.
 *
 * The tables.  The left table is the context's word table (dprf_ctx_set_words, unchanged).  The right table is a second
 * one with the same validation, conversion, storage and life cycle: Office words go from UTF-8 to UTF-16LE, the other
 * formats keep their bytes, a word is stored clipped to a 64-byte slot, and the table goes to every device of the
 * context, where it stays until it is replaced, cleared (n = 0) or the context is destroyed.  dprf_ctx_set_right_words
 * refuses what dprf_ctx_set_words refuses, and n >= 2^31 as DPRF_E_INVALID (the device divides a right index plus a
 * chunk's candidate index as 32 bits); a refused table leaves the previous one in place.  It takes the context's call
 * mutex.  Neither setter touches the other table.  dprf_ctx_right_words returns the number of right words held (0: no
 * table); dprf_words_status serves both tables.
 *
 * The keyspace.  With N1 left and N2 right words, candidate i of the keyspace N1 * N2 is left word i / N2 followed by
 * right word i % N2: the left word is the slowest digit, as the word is in hybrid and rule mode.  The bytes are the
 * concatenation, and the format's truncation applies to the whole candidate (PDF R2-R4 32 bytes, R5 127).
 *
 * dprf_search_combine verifies indices [start, start + count).  Nothing but the chunk start's two word indices goes up
 * per launch; the device spells every candidate into a list slot from the two tables it holds (k_spell_combine) and
 * the list-mode kernels verify the slots.  hits[] relative to `start`, stop_on_first (the lowest verifying index),
 * multi-device chunks, the cross-device stop, stats, the per-device records, owner mode, a set key40 and
 * DPRF_FLAG_NEVER_MATCHES contexts are as dprf_search_hybrid's.
 * dprf_spell_combine is the counterpart of dprf_spell_rules: slot k of slots[count * 64] holds the bytes of candidate
 * start + k after the format's cut (Office: UTF-16LE), zero-padded, and lens[k] their number, spelled by the same
 * kernel on the context's first device; no verification kernel runs.  count <= 2^20.
 * Errors (a refused call leaves no per-device record, and the context still serves):
 * DPRF_E_INVALID -- a null argument, either table missing (the message says which), start + count above N1 * N2
 * (computed in 128 bits); for dprf_spell_combine also count above 2^20 or a never-matching context.
 * DPRF_E_PWLEN -- min(the longest converted left word + the longest converted right word, the truncation) exceeds a
 * 64-byte slot; the message names both words by index and gives their converted lengths.  Where the truncation is at
 * most 64 bytes (R2-R4) tables of any word lengths are accepted.
 * Not done: a mask around the pair, more than two tables, candidates over 64 bytes. */
int dprf_ctx_set_right_words(dprf_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, int64_t n);
int64_t dprf_ctx_right_words(const dprf_ctx *ctx);
int dprf_search_combine(dprf_ctx *ctx, uint64_t start, uint64_t count, int stop_on_first, uint64_t *hits, int64_t cap,
                        int64_t *nhits, dprf_stats *stats);
int dprf_spell_combine(dprf_ctx *ctx, uint64_t start, uint64_t count, uint8_t *slots, uint8_t *lens);

/* ---- 40-bit key search: the candidate is the RC4 key itself ----
 * Additive to ABI 9 (DPRF_ABI_VERSION stays 9): a caller detects it by looking the symbol dprf_search_key40 up.
 * Four of the families protect the document with only 40 bits of RC4 key, however long the password is, so the keys
 * form a smaller space than any serious password space and can be searched to the end: DPRF_KEY40_SPACE = 2^40 keys.
 * A password mode can fail on a long or unusual password; a key search cannot, and it returns the key, which is what
 * decrypts the document (hashcat modes 10410 / 9710 / 9810).  A password search of at least 2^40 candidates already
 * yields a colliding password of such a document in expectation, but with no bound and no completeness, and it pays for
 * hashing a key search does not need.
 * A key index i lies in [0, 2^40) and stands for the five bytes b0..b4 of i written big-endian: b0 = i >> 32,
 * b4 = i & 0xff, hex spelling "%010x" of i.  That is the order itertools.product(range(256), repeat=5) gives, as in range
 * mode: the leftmost byte is the most significant.  A key may hold any byte, 00 included.  PAD is the 32-byte padding
 * string of the PDF standard.  What the five bytes are, and when index i verifies:
 *   PDF R2                            the 5-byte RC4 key (5 bytes of an MD5; the reference uses a 5-byte key whatever
 *                                     Length says, pdf_password_verifier.c:161-163):
 *                                       RC4(b0..b4, PAD) == U[0:32]                                     (:184-189)
 *   PDF R3 / R4 with Length / 8 == 5  the same 5-byte key k:
 *                                       c = RC4(k, MD5(PAD || ID)); c = RC4(k XOR x, c) for x = 1..19   (:164-176)
 *                                       c[0:16] == U[0:16]
 *   Office 97-2003 types 0 / 1        h[0:5] of the second MD5 of the password hash:
 *                                       k = MD5(b0..b4 || 00 00 00 00)   (all 16 bytes are the RC4 key)
 *                                       d = RC4(k, encryptedVerifier || encryptedVerifierHash)
 *                                       MD5(d[0:16]) == d[16:32]
 *   Office 97-2003 type 3             the five key bytes of RC4 CryptoAPI's 40-bit key:
 *                                       key = b0..b4 || eleven 00 bytes   (a 16-byte RC4 key)
 *                                       d = RC4(key, encryptedVerifier || encryptedVerifierHash)   (36 bytes)
 *                                       SHA1(d[0:16]) == d[16:36]
 * Every other document is refused with DPRF_E_DOMAIN and a message that names why it is not a 40-bit one: PDF R3 / R4
 * with a 16-byte key, R5, R6, Office 97-2003 type 4, Office 2007, Agile, and both ODF streams.
 * The user / owner selection of a PDF context has no effect: there is one file key, and it is checked against /U.
 * hits[] holds key indices, absolute and ascending, as range mode reports; stop_on_first, multi-device chunks, the
 * cross-device stop, stats and the per-device records behave as dprf_search_range's.  A DPRF_FLAG_NEVER_MATCHES context
 * answers "no hit" without device work.  dprf_ctx_kernel keeps returning the password family; the key searches have
 * names of their own that dprf_plan_chunk knows ("pdf_r24_key40", "office_rc4_md5_key40", "office_rc4_sha1_key40"),
 * planned with the password family's policy.
 * Errors (the context still serves after a refused call): DPRF_E_INVALID -- a null argument, or start + count above
 * 2^40 (computed without wrapping); DPRF_E_DOMAIN -- the context is not one of the four families above.
 * Not done: decrypting the document with the key, key lengths other than 40 bits. */
#define DPRF_KEY40_SPACE (1ull << 40)
int dprf_search_key40(dprf_ctx *ctx, uint64_t start, uint64_t count, int stop_on_first, uint64_t *hits, int64_t cap,
                      int64_t *nhits, dprf_stats *stats);

/* ---- password for a known key: the searches verify against five key bytes ----
 * Additive to ABI 9 (DPRF_ABI_VERSION stays 9): a caller detects it by looking the symbol dprf_ctx_set_key40 up.
 * dprf_search_key40 ends with a key, and a key cannot be typed into a viewer.  A context of one of the four 40-bit
 * families can be given that key -- five bytes K = b0..b4 in the order dprf_search_key40 reports -- and from then on a
 * candidate verifies exactly when its key derivation yields K (hashcat's collider-#2 modes 10420 / 9720 / 9820).  Any
 * such password opens the document; it need not be the one the document was saved with.  Nothing of /U,
 * encryptedVerifier or encryptedVerifierHash is read, and no RC4 runs: the check is the hashing alone.  PAD is the
 * 32-byte padding string of the PDF standard, pw16 the candidate in UTF-16LE:
 *   PDF R2                            h = MD5((pw[:32] || PAD)[:32] || O || LE32(P) || ID [|| FFFFFFFF if R >= 4 and
 *                                     !EncryptMetadata]);  h[0:5] == K
 *   PDF R3 / R4 with Length / 8 == 5  the same h, then 50 x h = MD5(h[0:5]);  h[0:5] == K
 *   Office 97-2003 types 0 / 1        h = MD5(pw16); h = MD5((h[0:5] || salt) x 16);  h[0:5] == K  (the third MD5 of the
 *                                     password check is not computed)
 *   Office 97-2003 type 3             h = SHA1(salt || pw16); k = SHA1(h || 00 00 00 00);  k[0:5] == K
 * Truncation and candidate lengths are those of the family's password search: PDF cuts at 32 bytes, Office takes at
 * most 32 UTF-16 units in a slot and more is DPRF_E_PWLEN.
 * While a key is set dprf_search_range, dprf_search_symbols, dprf_search_mask, dprf_verify_list, dprf_search_hybrid,
 * dprf_search_rules and dprf_search_combine verify against K, with hit indices, stop_on_first, multi-device chunks,
 * the cross-device stop, stats, the per-device records and dprf_list_status as before.  Several candidates of one
 * window may verify -- that is the purpose -- and all are reported, ascending.  key == NULL clears the key and
 * restores the document check exactly.  dprf_search_key40, dprf_spell_rules and dprf_spell_combine are unaffected by
 * the selection.  The setter takes the context's call mutex (it waits for a running call).  dprf_ctx_key40 returns 1
 * and writes the five bytes (key may be NULL) when a key is set, else 0.
 * Errors (neither changes the selection, and the context still serves): DPRF_E_DOMAIN -- the document is not a 40-bit
 * one, with dprf_search_key40's sentence; DPRF_E_INVALID -- a PDF context in owner mode: a key collider finds the user
 * password.  dprf_ctx_set_pdf_password(ctx, DPRF_PDF_OWNER) while a key is set is DPRF_E_INVALID likewise.  A
 * DPRF_FLAG_NEVER_MATCHES context accepts a key and finds nothing, without device work.
 * While a key is set dprf_ctx_kernel returns "pdf_r24_collide", "office_rc4_md5_collide" or "office_rc4_sha1_collide",
 * families dprf_plan_chunk knows (the password family's policy with a ceiling of 2^31 candidates per launch; the
 * measured rate sizes the later chunks).
 * Not done: a server / client protocol that carries the key, key lengths other than 40 bits. */
int dprf_ctx_set_key40(dprf_ctx *ctx, const uint8_t *key);   /* five bytes; NULL clears */
int dprf_ctx_key40(const dprf_ctx *ctx, uint8_t *key);       /* 1 and the five bytes if set, 0 if not */

#ifdef __cplusplus
}
#endif
#endif
