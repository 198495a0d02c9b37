// rc_outputs.cpp -- see rc_outputs.h
#include "rc_outputs.h"

#include <sys/stat.h>

typedef unsigned long long ull;

bool two_mates(const Run &run)
{
    for (const ReadFile &f : run.files)
        if (f.paired || f.interleaved) return true;
    return false;
}

uint64_t hbm_free(const Run &run, bool first_only)
{
    uint64_t least = ~(uint64_t)0;
    for (size_t g = 0; g < (first_only ? 1 : run.ctx.size()); ++g) {
        uint64_t f = 0;
        if (rc_device_memory(run.ctx[g], &f, nullptr)) {
            if (first_only) die("rcorrector: %s\n", rc_last_error(run.ctx[g]));
            f = 0;
        }
        least = std::min(least, f);
    }
    if (const char *hf = getenv("RC_HBM_FREE_MB")) least = (uint64_t)atoll(hf) << 20;  // tests: as if this much were free
    return least;
}

static void ok(rc_ctx *c, int failed)
{
    if (failed) die("rcorrector: %s\n", rc_last_error(c));
}
static void written(bool ok, const char *path)
{
    if (!ok) die("rcorrector: could not write %s\n", path);
}

// ---- the contexts' shares of one output, three ways ----
// fn(context) on every context: every GPU counts the batches that complete on it
template <class F>
static void on_every_context(const Run &run, F fn)
{
    for (rc_ctx *c : run.ctx) ok(c, fn(c));
}
// device side: the other contexts' keys merged into the first
template <class F>
static void merge_into_first(const Run &run, F merge)
{
    for (size_t c = 1; c < run.ctx.size(); ++c) ok(run.ctx[0], merge(run.ctx[0], run.ctx[c]));
}
// host side: get(context, &part) from every context, add(total, part) into the first one's, end(context) where the session has one
template <class T, class Get, class Add, class End>
static std::unique_ptr<T[]> added_up(const Run &run, Get get, Add add, End end)
{
    std::unique_ptr<T[]> v(new T[2]());  // [0] the total, [1] the context at hand
    for (size_t c = 0; c < run.ctx.size(); ++c) {
        ok(run.ctx[c], get(run.ctx[c], &v[c ? 1 : 0]));
        if (c) add(v[0], v[1]);
        ok(run.ctx[c], end(run.ctx[c]));
    }
    return v;
}
// ... a struct of nothing but uint64_t counts
template <class T>
static void add_words(T &to, const T &from)
{
    static_assert(sizeof(T) % sizeof(uint64_t) == 0, "counts only");
    for (size_t w = 0; w < sizeof(T) / sizeof(uint64_t); ++w) reinterpret_cast<uint64_t *>(&to)[w] += reinterpret_cast<const uint64_t *>(&from)[w];
}
static int no_end(rc_ctx *) { return 0; }

// ---- -histo-after: a recount session on the first GPU's context.  One GPU: every batch that completes leaves its corrected
// arena with the session, device to device (rc_recount_follow); several: the workers hand over the corrected text's bases. ----
static void histo_after_begin(Run &run, const Options &opt)
{
    // the bases stay in HBM until the finish, next to its sort scratch: stop here rather than half-way if they will not fit
    uint64_t bases = 0;
    bool known = true;
    if (run.resident) {
        for (rc_ctx *c : run.ctx) {
            size_t na = 0;
            ok(c, rc_table_count_arenas(c, &na, nullptr, 0));
            std::vector<uint64_t> ab(na);
            if (na) ok(c, rc_table_count_arenas(c, &na, ab.data(), na));
            for (uint64_t b : ab) bases += b;
        }
    } else {
        for_each_input(run, [&](const ReadFile &f) {
            struct stat st;
            if (stat(f.path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) {
                known = false;  // (a pipe: its size is anybody's guess, the session says so if it runs out)
                return;
            }
            // bases per byte of file: half of a FASTQ file, all of a FASTA file at most; deflated FASTQ is a fifth to a quarter of its text
            const uint64_t text = f.src.is_gz ? (uint64_t)st.st_size * 5 : (uint64_t)st.st_size;
            bases += f.fastq ? text / 2 + text / 16 : text;
        });
    }
    const uint64_t free_now = hbm_free(run, true);
    const uint64_t scratch = std::min<uint64_t>(opt.count_mem, bases * 46);  // (the passes' scratch: rc_count.hip, 40 bytes per k-mer occurrence + 15 %)
    const uint64_t need = bases + scratch + ((uint64_t)256 << 20);
    if ((known || bases) && need > free_now)
        die("rcorrector: -histo-after keeps the corrected bases in GPU memory until the end of the run: about %llu MB with the counting scratch, "
            "%llu MB are free (lower RC_COUNT_MEM_MB, or run without -histo-after)\n", (ull)(need >> 20), (ull)(free_now >> 20));
    ok(run.ctx[0], rc_recount_begin(run.ctx[0], (uint32_t)opt.histo_max));
    if (run.gpus == 1)
        ok(run.ctx[0], rc_recount_follow(run.ctx[0], 1));
    else
        run.recount_host = true;
}

static void histo_after_finish(const Run &run, const Options &opt)
{
    const double t0 = now_s();
    std::vector<uint64_t> freq((size_t)opt.histo_max + 1);
    rc_recount_stats rs;
    ok(run.ctx[0], rc_recount_finish(run.ctx[0], freq.data(), &rs));
    written(write_histo(opt.histo_after, freq), opt.histo_after);
    if (g_timing) fprintf(stderr, "[rc timing] -histo-after: recount of the corrected reads %.2f s\n", now_s() - t0);
    fprintf(stderr, "Corrected reads: %llu distinct k-mers, %llu seen once, %llu not in the table (%llu occurrences)\n", (ull)rs.all.distinct,
            (ull)rs.all.unique, (ull)rs.absent_distinct, (ull)rs.absent_total);
}

// ---- -weak-ends and -depth-tags / -depth: the writer has added them up ----
static void weak_ends_finish(const Run &run)
{
    fprintf(stderr, "Weak ends (k-mers counted below %d): %llu reads with a bad prefix, %llu with a bad suffix, %llu without a solid k-mer\n", run.weak_min,
            (ull)run.weak_prefix, (ull)run.weak_suffix, (ull)run.weak_nosolid);
}

static void depth_finish(const Run &run, const Options &opt)
{
    const uint64_t with = run.depth_reads[0] + run.depth_reads[1] - run.depth_novalid[0] - run.depth_novalid[1];
    const uint64_t zero = (run.depth_hist[0].empty() ? 0 : run.depth_hist[0][0]) + (run.depth_hist[1].empty() ? 0 : run.depth_hist[1][0]);
    const size_t mm = depth_median_of_medians(run.depth_hist);
    fprintf(stderr, "K-mer depth: %llu reads with a valid k-mer window, %llu of them with a median of 0; the median of the reads' medians is %zu%s\n",
            (ull)with, (ull)zero, mm, with && mm == (size_t)run.depth_max ? " or more (the last bin, -depth-max)" : "");
    if (opt.depth) written(write_depth_report(opt.depth, run.k, run.depth_reads, run.depth_novalid, run.depth_hist, two_mates(run)), opt.depth);
}

// ---- -report: the contexts' reports, added up ----
static void report_finish(const Run &run, const Options &opt)
{
    auto sum = added_up<rc_change_report>(run, rc_change_report_get, add_words<rc_change_report>, no_end);
    written(write_change_report(opt.report, sum[0], two_mates(run)), opt.report);
}

// ---- -dups: the contexts' keys, merged into the first ----
static void dups_finish(const Run &run, const Options &opt)
{
    const double t0 = now_s();
    merge_into_first(run, rc_dup_census_merge);
    std::vector<uint64_t> before((size_t)opt.dups_max + 1), after((size_t)opt.dups_max + 1);
    rc_dup_census dc;
    dc.copies_before = before.data();
    dc.copies_after = after.data();
    ok(run.ctx[0], rc_dup_census_get(run.ctx[0], (uint32_t)opt.dups_max, &dc));
    const char *unit = two_mates(run) ? "pairs" : "reads";  // (all of one kind: parse_options has checked)
    written(write_dup_census(opt.dups, dc, (uint32_t)opt.dups_max, unit), opt.dups);
    if (g_timing) fprintf(stderr, "[rc timing] -dups: merge, sort and census %.2f s\n", now_s() - t0);
    const double u = dc.units ? (double)dc.units : 1.0;
    fprintf(stderr, "Duplicates: %llu %s, %llu distinct before correction (duplicate fraction %.4f), %llu after (%.4f)\n", (ull)dc.units, unit,
            (ull)dc.distinct_before, dc.units ? 1.0 - (double)dc.distinct_before / u : 0.0, (ull)dc.distinct_after,
            dc.units ? 1.0 - (double)dc.distinct_after / u : 0.0);
}

// ---- -recurrent: the contexts' site keys, merged into the first ----
static void recurrent_finish(const Run &run, const Options &opt)
{
    const double t0 = now_s();
    merge_into_first(run, rc_recur_census_merge);
    std::vector<uint64_t> bins((size_t)opt.recur_max + 1), tk((size_t)opt.recur_top + 1), tc((size_t)opt.recur_top + 1);
    rc_recur_census rcs;
    rcs.recur = bins.data();
    rcs.top_key = tk.data();
    rcs.top_count = tc.data();
    ok(run.ctx[0], rc_recur_census_get(run.ctx[0], (uint32_t)opt.recur_max, (uint32_t)opt.recur_min, (uint32_t)opt.recur_top, &rcs));
    written(write_recur_census(opt.recurrent, rcs, (uint32_t)opt.recur_max, (uint32_t)opt.recur_min), opt.recurrent);
    if (g_timing) fprintf(stderr, "[rc timing] -recurrent: merge, sort and census %.2f s\n", now_s() - t0);
    // (the bins below -recurrent-min are exact, -recurrent-min <= -recurrent-max: what is not in them repeats that often)
    uint64_t few_sites = 0, few_changes = 0;
    for (long c = 1; c < opt.recur_min; ++c) {
        few_sites += bins[(size_t)c];
        few_changes += bins[(size_t)c] * (uint64_t)c;
    }
    fprintf(stderr, "Recurrent corrections: %llu contexted changes at %llu sites; %llu changes at %llu sites corrected at least %ld times\n",
            (ull)rcs.contexted, (ull)rcs.sites, (ull)(rcs.contexted - few_changes), (ull)(rcs.sites - few_sites), opt.recur_min);
}

// ---- -trust-by-pos: the contexts' counts, added up ----
static void trust_finish(const Run &run, const Options &opt)
{
    auto tp = added_up<rc_trust_profile>(run, rc_trust_profile_get, add_trust_profile, rc_trust_profile_end);
    written(write_trust_profile(opt.trust, tp[0], two_mates(run)), opt.trust);
    uint64_t valid[2] = {0, 0}, weak[2] = {0, 0};
    const rc_trust_counts *ver[2] = {&tp[0].before, &tp[0].after};
    for (int v = 0; v < 2; ++v)
        for (int m = 0; m < 2; ++m)
            for (int p = 0; p < RC_TRUST_MAX_LEN; ++p) {
                weak[v] += ver[v]->weak5[m][p];
                valid[v] += ver[v]->weak5[m][p] + ver[v]->solid5[m][p];
            }
    fprintf(stderr, "Trust by position (k-mers counted below %d are weak): %llu of %llu valid k-mer windows weak before correction (%.4f), %llu of %llu after (%.4f)\n",
            run.weak_min, (ull)weak[0], (ull)valid[0], valid[0] ? (double)weak[0] / (double)valid[0] : 0.0, (ull)weak[1], (ull)valid[1],
            valid[1] ? (double)weak[1] / (double)valid[1] : 0.0);
}

// ---- -overlap: the contexts' counts of the batches of pairs, added up ----
static void overlap_finish(const Run &run, const Options &opt)
{
    auto mo = added_up<rc_mate_overlap>(run, rc_mate_overlap_get, add_mate_overlap, rc_mate_overlap_end);
    written(write_mate_overlap(opt.overlap, mo[0]), opt.overlap);
    const rc_mate_overlap &M = mo[0];
    fprintf(stderr, "Mate overlap (at least %d bases, at most %d %% mismatches): %llu of %llu pairs overlap; %llu of %llu compared bases disagree before correction (%.6f), %llu of %llu after (%.6f); %llu introduced\n",
            opt.overlap_min, opt.overlap_mm, (ull)M.overlapping, (ull)M.pairs, (ull)M.disagree_before, (ull)M.compared_before,
            M.compared_before ? (double)M.disagree_before / (double)M.compared_before : 0.0, (ull)M.disagree_after, (ull)M.compared_after,
            M.compared_after ? (double)M.disagree_after / (double)M.compared_after : 0.0, (ull)M.introduced);
}

void outputs_begin(Run &run, const Options &opt)
{
    if (opt.histo_after) histo_after_begin(run, opt);
    if (opt.report) on_every_context(run, rc_change_report_begin);
    if (opt.dups) on_every_context(run, rc_dup_census_begin);
    if (opt.recurrent) on_every_context(run, rc_recur_census_begin);
    if (opt.trust) on_every_context(run, [&](rc_ctx *c) { return rc_trust_profile_begin(c, run.weak_min); });
    if (opt.overlap) on_every_context(run, [&](rc_ctx *c) { return rc_mate_overlap_begin(c, opt.overlap_min, opt.overlap_mm); });
}

void outputs_finish(Run &run, const Options &opt)
{
    if (run.weak_ends) weak_ends_finish(run);
    if (run.depth_on) depth_finish(run, opt);
    if (opt.report) report_finish(run, opt);
    if (opt.dups) dups_finish(run, opt);
    if (opt.recurrent) recurrent_finish(run, opt);
    if (opt.trust) trust_finish(run, opt);
    if (opt.overlap) overlap_finish(run, opt);
    if (opt.histo_after) histo_after_finish(run, opt);
}
