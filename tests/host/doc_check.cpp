/* doc_check.cpp -- the document layer of libdprf (dprf_amd/csrc/dprf_doc.cpp) as a stand-alone program: no HIP, no
 * Python, so the parsers of untrusted text run on any machine, and under a host sanitizer when built with one:
 *
 *     g++ -std=c++17 -I dprf_amd/csrc tests/host/doc_check.cpp dprf_amd/csrc/dprf_doc.cpp -o doc_check
 *
 * One line of output per line of input; the columns of a line are separated by tabs.
 *   ctx <field> <field> ...   the field array of dprf_ctx_create.  Prints the return code and then, on failure,
 *                             dprf_last_error's text; on success the family name, fmt, flags, the family's params
 *                             struct as hex words (a device pointer in it is null here: two zero words) and, for the
 *                             $odt$ and $odf$ streams, the context's word vector.
 *   owner <0 | 1>             dprf_ctx_set_pdf_password's check on the last parsed document: the code, the text on
 *                             failure; on success the document is in that mode for the cand lines after it.
 *   cand <hex bytes>          convert_candidate on the last parsed document: its code, the converted length and, for
 *                             a refusal, status_text's sentence.
 * tests/test_doc_layer.py drives it. */
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "dprf_doc.h"

using namespace dprf_internal;

static std::vector<std::string> split_tabs(const std::string &line) {
    std::vector<std::string> out(1);
    for (char ch : line) {
        if (ch == '\t') out.emplace_back();
        else out.back().push_back(ch);
    }
    return out;
}

static void print_words(const void *p, size_t bytes) {
    for (size_t i = 0; i + 4 <= bytes; i += 4) {
        uint32_t w;
        memcpy(&w, (const char *)p + i, 4);
        printf("%s%08x", i ? " " : "", w);
    }
}

/* the params struct the family's kernels take, as the context holds it */
static void print_params(const dprf_doc &d) {
    switch (d.kind) {
        case K_OFFICE: print_words(&d.office, sizeof d.office); break;
        case K_AGILE_SHA1:
        case K_AGILE_SHA512: print_words(&d.agile, sizeof d.agile); break;
        case K_OLDOFFICE_MD5:
        case K_OLDOFFICE_SHA1: print_words(&d.oldoffice, sizeof d.oldoffice); break;
        case K_ODT: print_words(&d.odt, sizeof d.odt); break;
        case K_ODF_BF: print_words(&d.odf, sizeof d.odf); break;
        case K_PDF_R24:
        case K_PDF_R5:
        case K_PDF_R6: print_words(&d.pdf, sizeof d.pdf); break;
        default: break;
    }
}

int main() {
    dprf_doc doc;
    bool have = false;
    std::string line;
    while (std::getline(std::cin, line)) {
        const std::vector<std::string> col = split_tabs(line);
        if (col[0] == "ctx") {
            std::vector<const char *> f;
            for (size_t i = 1; i < col.size(); i++) f.push_back(col[i].c_str());
            dprf_doc d;
            const int r = f.empty() ? fail(DPRF_E_INVALID, "no fields") : parse_document(&d, f.data(), (int)f.size());
            if (r != DPRF_OK) {
                printf("%d\t%s\n", r, dprf_last_error());
                continue;
            }
            doc = d;
            have = true;
            printf("0\t%s\t%d\t%d\t", kind_name(d.kind), d.fmt, d.flags);
            print_params(d);
            printf("\t");
            const std::vector<uint32_t> &w = d.kind == K_ODT ? d.odt_words : d.odf_words;
            print_words(w.data(), 4 * w.size());
            printf("\n");
        } else if (col[0] == "owner" && col.size() == 2 && have) {
            const int which = col[1] == "1" ? DPRF_PDF_OWNER : DPRF_PDF_USER;
            const int r = check_pdf_password(&doc, which);
            if (r == DPRF_OK) doc.pdf.owner = which == DPRF_PDF_OWNER ? 1u : 0u;
            printf("%d\t%s\t%s\n", r, r ? dprf_last_error() : "", kind_name(doc.kind, doc.pdf.owner != 0));
        } else if (col[0] == "cand" && col.size() == 2 && have && col[1].size() % 2 == 0) {
            std::vector<uint8_t> pw, tmp;
            pw.reserve(1);   /* an empty candidate still has an address, as in a caller's blob */
            for (size_t i = 0; i < col[1].size(); i += 2) pw.push_back((uint8_t)std::stoi(col[1].substr(i, 2), nullptr, 16));
            const uint8_t *cv = nullptr;
            size_t cl = 0;
            const int r = convert_candidate(&doc, pw.data(), pw.size(), &cv, &cl, tmp);
            printf("%d\t%zu\t%s\n", r, cl, r < 0 ? status_text(r, &doc, pw.size()) : "");
        } else {
            printf("?\t%s\n", col[0].c_str());
        }
    }
    return 0;
}
