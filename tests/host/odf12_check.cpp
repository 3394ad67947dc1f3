/* odf12_check.cpp -- what the document layer of libdprf (dprf_amd/csrc/dprf_doc.cpp) makes of an ODF stream, as a
 * stand-alone program: no HIP, no Python, and under a host sanitizer when built with one:
 *
 *     g++ -std=c++17 -I dprf_amd/csrc tests/host/odf12_check.cpp dprf_amd/csrc/dprf_doc.cpp -o odf12_check
 *
 * tests/host/doc_check.cpp prints one params struct per family; the "$odf$*1*1*" family has two (the KDF's and the
 * check's) and plans its chunks by the document's iteration count, which that program has no command for.
 * One line of output per line of input, columns separated by tabs.
 *   ctx <field> ...     parse_document.  On failure the code and dprf_last_error's text.  On success: 0, the family
 *                       name, fmt, flags, the family row (key words, long-list algorithm, long_keys, streams, and one
 *                       character each for the owner, key-search, collider and no-long entries: '-' null, '+' set),
 *                       dprf_odt_params as hex words (the device pointer null), dprf_odf_aes_params as hex words, the
 *                       odt word vector, and plan_iterations.
 *   cand <hex bytes>    convert_candidate on the last parsed document: code, converted length, the refusal's sentence.
 *   policy              the last document's chunk policy at its iteration count: init lo hi tail gran.
 *   plan <rate per ms> <remaining> <total> <ndev> <inflight>      plan_chunk for the last document.
 * tests/test_odf12_iter_model.py drives it. */
#include <cstdio>
#include <cstdlib>
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
            const family &fm = fam(d.kind);
            printf("0\t%s\t%d\t%d\t%u %u %d %d %c%c%c%c\t", kind_name(d.kind), d.fmt, d.flags, fm.key_words, fm.long_alg,
                   fm.long_keys ? 1 : 0, fm.streams, fm.owner_name ? '+' : '-', fm.key40_name ? '+' : '-',
                   fm.collide_name ? '+' : '-', fm.no_long ? '+' : '-');
            print_words(&d.odt, sizeof d.odt);
            printf("\t");
            print_words(&d.odfaes, sizeof d.odfaes);
            printf("\t");
            print_words(d.odt_words.data(), 4 * d.odt_words.size());
            printf("\t%u\n", plan_iterations(&d));
        } else if (col[0] == "cand" && col.size() == 2 && have && col[1].size() % 2 == 0) {
            std::vector<uint8_t> pw, tmp;
            pw.reserve(1);   /* an empty candidate still has an address, as in a caller's blob */
            for (size_t i = 0; i < col[1].size(); i += 2) pw.push_back((uint8_t)std::stoi(col[1].substr(i, 2), nullptr, 16));
            const uint8_t *cv = nullptr;
            size_t cl = 0;
            const int r = convert_candidate(&doc, pw.data(), pw.size(), &cv, &cl, tmp);
            printf("%d\t%zu\t%s\n", r, cl, r < 0 ? status_text(r, &doc, pw.size()) : "");
        } else if (col[0] == "policy" && have) {
            const chunk_policy p = policy(doc.kind, false, false, plan_iterations(&doc));
            printf("%u\t%u\t%u\t%u\t%u\n", p.init, p.lo, p.hi, p.tail, p.gran);
        } else if (col[0] == "plan" && col.size() == 6 && have) {
            const uint64_t n = plan_chunk(doc.kind, false, atof(col[1].c_str()), strtoull(col[2].c_str(), nullptr, 10),
                                          strtoull(col[3].c_str(), nullptr, 10), atoi(col[4].c_str()),
                                          atoi(col[5].c_str()), false, plan_iterations(&doc));
            printf("%llu\n", (unsigned long long)n);
        } else {
            printf("?\t%s\n", col[0].c_str());
        }
    }
    return 0;
}
