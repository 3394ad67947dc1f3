/* dprf_launch.h -- host-side launchers of the verification kernels (internal to libdprf.so). */
#ifndef DPRF_LAUNCH_H
#define DPRF_LAUNCH_H
#include <hip/hip_runtime.h>
#include "dprf_params.h"

/* keys: device scratch of >= 8 * e.count words (Agile: 16) (the derived keys handed from the KDF to the check kernel);
 * mid: if non-null, recorded on s between the KDF kernel and the check kernel (dominant-kernel timing) */
hipError_t launch_office(const dprf_enum &e, const dprf_office_params &p, const dprf_aes_tables *T,
                         dprf_results *R, uint32_t cap, uint32_t stop, hipStream_t s, uint32_t *keys,
                         hipEvent_t mid);
/* Agile (dprf_kernels_agile.hip): keys holds 16 * e.count words (two keys of up to 8 words); e.mode 0 or 1 */
hipError_t launch_agile(const dprf_enum &e, const dprf_agile_params &p, const dprf_aes_tables *T,
                        dprf_results *R, uint32_t cap, uint32_t stop, hipStream_t s, uint32_t *keys,
                        hipEvent_t mid);
/* Office 97-2003 RC4 (dprf_kernels_oldoffice.hip): one kernel per launch, no key hand-off; e.mode 0 or 1 */
hipError_t launch_oldoffice(const dprf_enum &e, const dprf_oldoffice_params &p, dprf_results *R, uint32_t cap,
                            uint32_t stop, hipStream_t s);
/* ODF 1.0 / 1.1 Blowfish (dprf_kernels_odf.hip): KDF on s_kdf, then the check on s_check (which may be s_kdf; if it is
 * not, it waits for `mid`, which must then be given), four key words per candidate in `keys`; e.mode 0 or 1 */
hipError_t launch_odf(const dprf_enum &e, const dprf_odf_params &p, dprf_results *R, uint32_t cap, uint32_t stop,
                      hipStream_t s_kdf, hipStream_t s_check, uint32_t *keys, hipEvent_t mid);
hipError_t launch_odt(const dprf_enum &e, const dprf_odt_params &p, const dprf_aes_tables *T,
                      dprf_results *R, uint32_t cap, uint32_t stop, hipStream_t s, uint32_t *keys,
                         hipEvent_t mid);
/* ODF 1.2 at the manifest's iteration count (dprf_kernels_odfaes.hip): its own KDF with kp, then launch_odt's check
 * kernel with p, eight key words per candidate in `keys`; e.mode 0, 1 or 2 */
hipError_t launch_odf_aes(const dprf_enum &e, const dprf_odf_aes_params &kp, const dprf_odt_params &p,
                          const dprf_aes_tables *T, dprf_results *R, uint32_t cap, uint32_t stop, hipStream_t s,
                          uint32_t *keys, hipEvent_t mid);
hipError_t launch_pdf_r5(const dprf_enum &e, const dprf_pdf_params &p, dprf_results *R, uint32_t cap,
                         uint32_t stop, hipStream_t s);
hipError_t launch_pdf_r24(const dprf_enum &e, const dprf_pdf_params &p, dprf_results *R, uint32_t cap,
                          uint32_t stop, hipStream_t s);
/* 40-bit key search (e.mode DPRF_ENUM_KEY40; dprf_kernels.hip and dprf_kernels_oldoffice.hip built with
 * DPRF_PART_KEY40): keys e.start .. e.start + e.count - 1 of a PDF R2 / R3-R4 Length-40 or an Office 97-2003 type
 * 0 / 1 / 3 document; any other document is hipErrorInvalidValue */
hipError_t launch_key40_pdf(const dprf_enum &e, const dprf_pdf_params &p, dprf_results *R, uint32_t cap,
                            uint32_t stop, hipStream_t s);
hipError_t launch_key40_oldoffice(const dprf_enum &e, const dprf_oldoffice_params &p, dprf_results *R, uint32_t cap,
                                  uint32_t stop, hipStream_t s);
/* password for a known 40-bit key (dprf_ctx_set_key40; the same two sources built with DPRF_PART_COLLIDE): range or
 * list candidates (e.mode 0 / 1) whose derived key is `key` -- the LE word of its bytes 0..3 and its byte 4 (dprf_doc.h
 * key40_words).  The same documents as above, PDF in user mode; anything else is hipErrorInvalidValue */
hipError_t launch_collide_pdf(const dprf_enum &e, const dprf_pdf_params &p, const uint32_t key[2], dprf_results *R,
                              uint32_t cap, uint32_t stop, hipStream_t s);
hipError_t launch_collide_oldoffice(const dprf_enum &e, const dprf_oldoffice_params &p, const uint32_t key[2],
                                    dprf_results *R, uint32_t cap, uint32_t stop, hipStream_t s);
/* long list (e.mode 2): the records' first-message hash into e.keys, or (DPRF_LONG_R5) the whole R5 check */
hipError_t launch_long_prehash(const dprf_enum &e, const dprf_long_params &lp, dprf_results *R, uint32_t cap,
                               uint32_t stop, hipStream_t s);
/* The device spellers (dprf_kernels_spell.hip), each into slots[n][DPRF_SLOT_WORDS] / lens[n]; bytes at or past
 * the trunc of the arguments stay zero. */
/* symbol windows (dprf_search_symbols): e.count candidates from the digits in e.sdig (base e.cslen), symbol table
 * symtab = [256] LE-packed bytes + [256] byte counts */
hipError_t launch_spell_symbols(const dprf_enum &e, const uint32_t *symtab, uint32_t trunc, uint32_t *slots,
                                uint8_t *lens, hipStream_t s);
/* mask windows (dprf_search_mask): a.count candidates from the digits in a.sdig, position records and symbol pool in
 * tab (DPRF_MASK_TAB_WORDS words, dprf_params.h) */
hipError_t launch_spell_mask(const dprf_mask_args &a, const uint32_t *tab, uint32_t *slots, uint8_t *lens,
                             hipStream_t s);
/* hybrid windows (dprf_search_hybrid): as launch_spell_mask with a word of the table
 * (wblob: packed bytes as u32 words, woff: a.nwords + 1 byte offsets) spelled before mask position a.word_at */
hipError_t launch_spell_hybrid(const dprf_hybrid_args &a, const uint32_t *tab, const uint32_t *wblob,
                               const uint32_t *woff, uint32_t *slots, uint8_t *lens, hipStream_t s);
/* rule windows (dprf_search_rules / dprf_spell_rules): a.count candidates, rule (a.r0 + g) %
 * a.nrules of the table (fns: a.nfns function words, roff: a.nrules + 1 offsets) applied to word a.w0 + (a.r0 + g) /
 * a.nrules */
hipError_t launch_spell_rules(const dprf_rules_args &a, const uint32_t *fns, const uint32_t *roff,
                              const uint32_t *wblob, const uint32_t *woff, uint32_t *slots, uint8_t *lens,
                              hipStream_t s);
/* combinator windows (dprf_search_combine / dprf_spell_combine): a.count candidates, left word a.l0 + (a.r0 + g) /
 * a.nright of (lblob, loff: a.nleft + 1 byte offsets) followed by right word (a.r0 + g) % a.nright of (rblob, roff:
 * a.nright + 1 byte offsets) */
hipError_t launch_spell_combine(const dprf_combine_args &a, const uint32_t *lblob, const uint32_t *loff,
                                const uint32_t *rblob, const uint32_t *roff, uint32_t *slots, uint8_t *lens,
                                hipStream_t s);
hipError_t launch_pdf_r6(const dprf_enum &e, const dprf_pdf_params &p, const dprf_aes_tables *T,
                         dprf_results *R, uint32_t cap, uint32_t stop, hipStream_t s);
#endif
