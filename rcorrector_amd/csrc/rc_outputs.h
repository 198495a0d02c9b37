// rc_outputs.h -- the extra outputs of the `rcorrector` CLI (none of them in the reference): what each one arms on the contexts
// before the pipeline runs and what it collects, writes (rc_format.h: write_*) and says on stderr afterwards.
//   -histo-after FILE   the k-mer count spectrum of the CORRECTED reads as `jellyfish histo` prints it (a recount session,
//                       rcorrector_amd.h: rc_recount_begin; -histo-max: its last bin) and one line on stderr: how many of their
//                       k-mers the table does not hold
//   -report FILE        the correction report (rc_change_report): the substitutions by position, letters, quality class, mate
//                       and read
//   -weak-ends          every record tagged with the reference's dormant bad_prefix= / bad_suffix= fields (Reads.h:396-412), filled
//                       from the weak-k-mer profile of the corrected reads (rc_read_weak; -weak-min: the count below which a k-mer
//                       is weak)
//   -depth-tags         kdepth=Q1:MED:Q3 on every record whose corrected read has a valid k-mer window: the quartiles of its
//   -depth FILE         k-mers' counts in the table (rc_read_depth); the reads by median (-depth-max: the last bin)
//   -dups FILE          the duplicate census (rc_dup_census): how many reads or pairs are exact copies of one another, as uploaded
//                       and as corrected, from 128-bit keys
//   -recurrent FILE     the recurrent-correction census (rc_recur_census): the sites -- 29 corrected bases around a change, and
//                       what it was corrected from -- at which the run made one fix in many reads
//   -trust-by-pos FILE  the k-mer trust profile by read position (rc_trust_profile): the reads with a solid / weak k-mer window
//                       at every position from either end, per mate, as uploaded and as corrected
//   -overlap FILE       the mate-overlap report (rc_mate_overlap): where mate 1 and the reverse complement of mate 2 cover the
//                       same bases, the bases they disagree on before and after correction, and the fragment lengths
//                       (-overlap-min / -overlap-mm: the shortest overlap and the most mismatches accepted)
// Every one of them is counted on the GPU as the batches complete, on every context, whatever the transport; -weak-ends and the
// depth are added up by the writer (Run::weak_*, Run::depth_*).  Each adds one line to stderr.
#pragma once
#include "rc_dispatch.h"
#include "rc_options.h"

// some input has two mates (-p / -i): the reports then carry a mate 2
bool two_mates(const Run &run);
// The device memory that is free right now: on the first GPU (an error ends the run), or the least over all GPUs (a GPU that
// cannot say counts as full).  RC_HBM_FREE_MB (tests): as if this much were free.
uint64_t hbm_free(const Run &run, bool first_only);
// fn(ReadFile &) for every input file, and for its mate if it has one, in command-line order
template <class F>
inline void for_each_input(Run &run, F fn)
{
    for (size_t fi = 0; fi < run.files.size(); ++fi) {
        fn(run.files[fi]);
        if (run.files[fi].paired) fn(run.mates[fi]);
    }
}

// after rc_set_run_params: -histo-after (with its test of the free HBM), -report, -dups, -recurrent, -trust-by-pos, -overlap
void outputs_begin(Run &run, const Options &opt);
// after the output files are closed: -weak-ends, depth, -report, -dups, -recurrent, -trust-by-pos, -overlap, -histo-after
void outputs_finish(Run &run, const Options &opt);
