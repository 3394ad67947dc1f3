/* key40_check.cpp -- what dprf_search_key40 decides without a device (dprf_amd/csrc/dprf_doc.cpp check_key40) as a
 * stand-alone program: no HIP, no Python, so it runs on any machine, and under a host sanitizer when built with one:
 *
 *     g++ -std=c++17 -I dprf_amd/csrc tests/host/key40_check.cpp dprf_amd/csrc/dprf_doc.cpp -o key40_check
 *
 * One line of output per line of input; the columns of a line are separated by tabs.
 *   ctx <field> <field> ...   the field array of dprf_ctx_create.  Prints the return code, then dprf_last_error's text
 *                             on failure, else the family name and its key-search name ("-" when it has none).
 *   owner <0 | 1>             the last parsed PDF in user / owner mode: the code of dprf_ctx_set_pdf_password's check.
 *   key40 <start> <count>     check_key40 on the last parsed document (decimal u64 values): its code and, for a
 *                             refusal, dprf_last_error's text.
 *   plan <name> <rate> <remaining> <total> <ndev> <inflight>   dprf_plan_chunk: the chunk.
 * tests/test_key40_doc.py drives it. */
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
            printf("0\t%s\t%s\n", kind_name(d.kind), key40_name(d.kind) ? key40_name(d.kind) : "-");
        } else if (col[0] == "owner" && col.size() == 2 && have) {
            const int which = atoi(col[1].c_str());
            const int r = check_pdf_password(&doc, which);
            if (r == DPRF_OK) doc.pdf.owner = which == DPRF_PDF_OWNER ? 1u : 0u;
            printf("%d\n", r);
        } else if (col[0] == "key40" && col.size() == 3 && have) {
            const uint64_t start = strtoull(col[1].c_str(), nullptr, 10), count = strtoull(col[2].c_str(), nullptr, 10);
            const int r = check_key40(&doc, start, count);
            if (r == DPRF_OK) printf("0\n");
            else printf("%d\t%s\n", r, dprf_last_error());
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
