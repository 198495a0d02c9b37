// The mate-overlap report's text (rc_format.h: mate_overlap_text, add_mate_overlap) for a report filled by hand; tests/
// test_mate_overlap_host.py holds the expected text.
#include <cstdio>
#include <cstring>
#include <memory>

#include "../../rcorrector_amd/csrc/rc_dispatch.h"

int main()
{
    std::unique_ptr<rc_mate_overlap> M(new rc_mate_overlap), S(new rc_mate_overlap);
    memset(M.get(), 0, sizeof *M);
    M->min_overlap = 30, M->max_mismatch_pct = 10, M->pairs = 1000, M->overlapping = 900;
    M->compared_before = 72000, M->compared_after = 72001, M->disagree_before = 700, M->disagree_after = 90;
    M->resolved = 620, M->kept = 78, M->introduced = 12, M->pairs_improved = 500, M->pairs_worsened = 9, M->pairs_same = 391;
    M->frag[1] = 3, M->frag[220] = 890, M->frag[2046] = 7;
    M->compared5[0][0] = 5, M->compared5[0][149] = 800, M->disagree5_before[0][149] = 9, M->disagree5_after[0][149] = 2;
    M->compared5[1][1023] = 4, M->disagree5_before[1][1023] = 4, M->disagree5_after[1][1023] = 3;
    M->disagree5_before[1][7] = 1;  // (no line: nothing was compared there)
    fputs(mate_overlap_text(*M).c_str(), stdout);
    *S = *M;
    add_mate_overlap(*S, *M);
    printf("sum\tpairs\t%llu\tfrag220\t%llu\tmin_overlap\t%llu\n", (unsigned long long)S->pairs, (unsigned long long)S->frag[220], (unsigned long long)S->min_overlap);
    return 0;
}
