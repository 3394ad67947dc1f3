/* combine_check.cpp -- check_combine of the document layer (dprf_amd/csrc/dprf_doc.cpp), the device-free half of
 * dprf_search_combine and dprf_spell_combine, as a stand-alone program: no HIP, no Python, and under a host sanitizer
 * when built with one:
 *
 *     g++ -std=c++17 -I dprf_amd/csrc tests/host/combine_check.cpp dprf_amd/csrc/dprf_doc.cpp -o combine_check
 *
 * One line of output per line of input; the columns of a line are separated by tabs, numbers are decimal.
 *   ctx <field> <field> ...                   the field array of dprf_ctx_create: the return code, then the family name
 *                                             or dprf_last_error's text.
 *   tables <N1> <len1> <idx1> <N2> <len2> <idx2>
 *                                             what the two setters leave in the document: the number of words, the
 *                                             longest converted word's length and its index, left then right (0 words:
 *                                             no table).  Prints "ok".
 *   check <start> <count>                     check_combine on the last parsed document: the code, then the text on
 *                                             failure or combine_longest's value on success.
 * tests/test_combine_check.py drives it. */
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

static uint64_t num(const std::string &s) { return strtoull(s.c_str(), nullptr, 10); }

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
            if (r == DPRF_OK) {
                doc = d;
                have = true;
            }
            printf("%d\t%s\n", r, r ? dprf_last_error() : kind_name(d.kind));
        } else if (col[0] == "tables" && col.size() == 7 && have) {
            doc.nwords = num(col[1]);
            doc.w_longest = num(col[2]);
            doc.w_longest_idx = num(col[3]);
            doc.nright = num(col[4]);
            doc.r_longest = num(col[5]);
            doc.r_longest_idx = num(col[6]);
            printf("ok\n");
        } else if (col[0] == "check" && col.size() == 3 && have) {
            const int r = check_combine(&doc, "dprf_search_combine", num(col[1]), num(col[2]));
            if (r) printf("%d\t%s\n", r, dprf_last_error());
            else printf("0\t%u\n", combine_longest(&doc));
        } else {
            printf("?\t%s\n", col[0].c_str());
        }
    }
    return 0;
}
