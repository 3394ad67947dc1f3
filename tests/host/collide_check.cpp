/* collide_check.cpp -- what dprf_ctx_set_key40 decides without a device (dprf_amd/csrc/dprf_doc.cpp check_set_key40,
 * check_pdf_password, the family table) as a stand-alone program: no HIP, no Python, so it runs on any machine, and
 * under a host sanitizer when built with one:
 *
 *     g++ -std=c++17 -I dprf_amd/csrc tests/host/collide_check.cpp dprf_amd/csrc/dprf_doc.cpp -o collide_check
 *
 * One line of output per line of input; the columns of a line are separated by tabs.  The program keeps what a context
 * keeps: the parsed document, its user / owner mode and its key.
 *   ctx <field> <field> ...   the field array of dprf_ctx_create.  Prints the return code, then dprf_last_error's text
 *                             on failure, else the family name and its known-key name ("-" when it has none).
 *   key <10 hex digits | ->   check_set_key40 (- clears), applied on success as dprf_ctx_set_key40 applies it: the
 *                             code, then the refusal's text or the name dprf_ctx_kernel would return.
 *   owner <0 | 1>             check_pdf_password, applied on success: the code, then the text or the name likewise.
 *   words                     the compare words of the set key (dprf_doc.h key40_words), two hex numbers.
 *   plan <name> <rate> <remaining> <total> <ndev> <inflight>   dprf_plan_chunk: the chunk.
 * tests/test_collide_doc.py drives it. */
#include <cstdio>
#include <cstdlib>
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

static const char *name_now(const dprf_doc &d) { return kind_name(d.kind, d.pdf.owner != 0, d.has_key40); }

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
            printf("0\t%s\t%s\n", kind_name(d.kind), fam(d.kind).collide_name ? fam(d.kind).collide_name : "-");
        } else if (col[0] == "key" && col.size() == 2 && have) {
            const bool set = col[1] != "-";
            if (set && col[1].size() != 10) { printf("?\n"); continue; }
            const int r = check_set_key40(&doc, set);
            if (r == DPRF_OK) {
                doc.has_key40 = set;
                for (int k = 0; k < 5; k++)
                    doc.key40[k] = set ? (uint8_t)strtoul(col[1].substr(2 * k, 2).c_str(), nullptr, 16) : 0;
            }
            printf("%d\t%s\n", r, r == DPRF_OK ? name_now(doc) : dprf_last_error());
        } else if (col[0] == "owner" && col.size() == 2 && have) {
            const int which = atoi(col[1].c_str());
            const int r = check_pdf_password(&doc, which);
            if (r == DPRF_OK) doc.pdf.owner = which == DPRF_PDF_OWNER ? 1u : 0u;
            printf("%d\t%s\n", r, r == DPRF_OK ? name_now(doc) : dprf_last_error());
        } else if (col[0] == "words" && have) {
            uint32_t k[2];
            key40_words(&doc, k);
            printf("%08x\t%08x\n", k[0], k[1]);
        } else if (col[0] == "plan" && col.size() == 7) {
            printf("%llu\n", (unsigned long long)dprf_plan_chunk(col[1].c_str(), atof(col[2].c_str()),
                                                                 strtoull(col[3].c_str(), nullptr, 10),
                                                                 strtoull(col[4].c_str(), nullptr, 10), atoi(col[5].c_str()),
                                                                 atoi(col[6].c_str())));
        } else {
            printf("?\n");
        }
    }
    return 0;
}
