// rc_options.cpp -- see rc_options.h
#include "rc_options.h"

#include <sys/stat.h>

static void print_help()
{
    fprintf(stderr,
            "Usage: ./rcorrector [OPTIONS]\n"
            "OPTIONS:\n"
            "Required parameters:\n"
            "\t-r seq_file: seq_file is the path to the sequence file. Can use multiple -r to specifiy multiple sequence files\n"
            "\t-p seq_file_left seq_file_right: the paths to the paired-end data set. Can use multiple -p to specifiy multiple sequence files\n"
            "\t-i seq_file: seq_file is the path to the interleaved mate-pair sequence file. Can use multiple -i\n"
            "\t-c jf_dump: the kmer counts dumped by JellyFish (without -c the k-mers of the input files are counted on the GPU)\n"
            "\t-k kmer_length\n"
            "Other parameters:\n"
            "\t-od output_file_directory (default: ./)\n"
            "\t-t number of threads to use (default: 1)\n"
            "\t-maxcor INT: the maximum number of correction every 100bp (default: 8)\n"
            "\t-maxcorK INT: the maximum number of correction within k-bp window (default: 4)\n"
            "\t-wk FLOAT: the proportion of kmers that are used to estimate weak kmer count threshold (default: 0.95)\n"
            "\t-stdout: output the corrected sequences to stdout (default: not used)\n"
            "\t-verbose: output some correction information to stdout (default: not used)\n"
            "MI355X build only:\n"
            "\t(-t: host threads that read, pack, format and write around the GPU; without it, or with -t 1: 16)\n"
            "\t-gpus INT: number of GPUs to shard the reads over, k-mer table replicated (default: 1)\n"
            "\twithout -c the k-mers are counted here (exact counts >= 2); ERROR_RATE is then estimated over this program's own\n"
            "\t\tdump order, not Jellyfish's: self-consistent, not byte-comparable with a jellyfish + reference run on large inputs\n"
            "\t-batch INT: reads per GPU batch (default: 1048576)\n"
            "\t-inflight INT: batches in flight per GPU, 1-4 (default: 2, raised to 4 while the writer waits for the GPU)\n"
            "\t-write-dump STRING: also write the k-mer table as a jellyfish-dump text file\n"
            "\t-histo STRING: also write the k-mer count spectrum (\"<count> <frequency>\" lines, as jellyfish histo prints them):\n"
            "\t\twithout -c of every k-mer counted, count 1 included; with -c of the dump's k-mers\n"
            "\t-histo-max INT: the spectrum's last bin, which holds the k-mers counted at least that often (default: 10000)\n"
            "\t-histo-after STRING: also write the k-mer count spectrum of the corrected reads (same format, -histo-max bounds it too) and\n"
            "\t\treport how many of their k-mers the table does not hold; the corrected bases stay in GPU memory until the end of the run\n"
            "\t\t(one byte per base); with -gpus above 1 they are counted on the first GPU, from the corrected text the host holds\n"
            "\t-report STRING: also write the correction report, tab-separated text: reads, changed bases by position from either end,\n"
            "\t\tby substitution, by quality class and per read, for each mate; counted on the GPU as the batches complete; with -gpus\n"
            "\t\tabove 1 every GPU keeps a report of its own and the file holds their sum\n"
            "\t-weak-ends: tag every record, behind l:m:h and cor, with bad_prefix=N / bad_suffix=N where N > 0: the bases of the corrected\n"
            "\t\tread in front of its first / behind its last k-mer that the table holds (unfixable reads keep their mark and get no tag);\n"
            "\t\tnothing is trimmed; one more line on stderr counts the reads with a bad prefix, a bad suffix, and no such k-mer at all\n"
            "\t\t(every read counts there, unfixable ones included); not with -verbose\n"
            "\t-weak-min INT: with -weak-ends and -trust-by-pos, a k-mer counted fewer times than this in the table is weak (default: 1)\n"
            "\t-depth-tags: tag every record whose corrected read has a valid k-mer window, last behind l:m:h, cor and the -weak-ends tags,\n"
            "\t\twith kdepth=Q1:MED:Q3: the lower quartile, median and upper quartile of the counts its k-mers have in the table (exact lower\n"
            "\t\tquantiles; a k-mer the table does not hold counts 0 -- with -c, whatever the dump left out); nothing is dropped, trimmed or\n"
            "\t\treordered; one more line on stderr; not with -verbose\n"
            "\t-depth STRING: also write the k-mer depth report, tab-separated text: k, per mate the reads and those without a valid k-mer\n"
            "\t\twindow, and for every median that occurs the reads of mate 1 (and of mate 2 for -p / -i input) that have it; with -gpus\n"
            "\t\tabove 1 the GPUs' batches are added up; the same line on stderr; not with -verbose\n"
            "\t-depth-max INT: with -depth, reads with a median of this or more are counted in the last line (default: 10000)\n"
            "\t-dups STRING: also write the duplicate census, tab-separated text: the units (reads, or pairs for -1/-2 and -i input), the\n"
            "\t\tdistinct units before and after correction, and for every number of copies c the distinct units that occur c times,\n"
            "\t\tbefore and after; two units are copies when their bases are byte for byte equal (mate 1 with mate 1, mate 2 with\n"
            "\t\tmate 2, no reverse complement); one more line on stderr gives the duplicate fraction; the keys (32 bytes per unit) stay\n"
            "\t\tin GPU memory until the end of the run, at most 2^32 - 1 units; with -gpus above 1 the GPUs' keys are merged on the\n"
            "\t\tfirst; the input is all single-end or all paired (-p / -i), not a mix; not with -verbose\n"
            "\t-dups-max INT: with -dups, units with this many copies or more are counted in the last line (default: 10000)\n"
            "\t-recurrent STRING: also write the recurrent-correction census, tab-separated text: the changed bases, those with 14\n"
            "\t\tupper-case ACGT bases of the corrected read on either side (contexted) and the others (clipped), the distinct sites -- the\n"
            "\t\t29 corrected bases around a change and the letter it was corrected from, either strand read as one -- for every number\n"
            "\t\tof changes c the sites corrected c times, and the sites corrected most often: count, from, to, 29-mer; a site fixed in\n"
            "\t\tmany reads is a candidate for a real variant that was corrected away; one more line on stderr; the keys (8 bytes per\n"
            "\t\tcontexted change) stay in GPU memory until the end of the run, at most 2^32 - 1; with -gpus above 1 the GPUs' keys\n"
            "\t\tare merged on the first; not with -verbose\n"
            "\t-recurrent-min INT: with -recurrent, the fewest changes of a listed site (default: 5)\n"
            "\t-recurrent-top INT: with -recurrent, the most sites listed (default: 1000)\n"
            "\t-recurrent-max INT: with -recurrent, sites with this many changes or more are counted in the last recur line (default: 10000)\n"
            "\t-trust-by-pos STRING: also write the k-mer trust profile by read position, tab-separated text: for every k-mer window\n"
            "\t\tposition counted from the 5' end (pos5) and from the 3' end (pos3, 0 = the last window), per mate, before and after\n"
            "\t\tcorrection: the reads that have a window there and those whose window is solid (in the table at least -weak-min\n"
            "\t\ttimes), weak, or invalid (holds a letter outside ACGT); one more line on stderr gives the weak share of the valid\n"
            "\t\twindows before and after; with -gpus above 1 the GPUs' counts are added up; not with -verbose\n"
            "\t-overlap STRING: also write the mate-overlap report, tab-separated text (paired input only, -p / -i): where mate 1 and the\n"
            "\t\treverse complement of mate 2 overlap, the bases the two disagree on before and after correction -- resolved, kept and\n"
            "\t\tintroduced (probable miscorrections) -- by position from each mate's 5' end, and the fragment lengths; the offset of a\n"
            "\t\tpair is chosen on the bases as read; one more line on stderr gives the disagreement rate before and after; with -gpus\n"
            "\t\tabove 1 the GPUs' counts are added up; not with -r files, not with -verbose\n"
            "\t-overlap-min INT: with -overlap, the fewest positions with two valid bases an overlap must have, 1-1023 (default: 30)\n"
            "\t-overlap-mm INT: with -overlap, the most mismatches accepted, in percent of those positions, 0-50 (default: 10)\n"
            "\t-verbose-iter INT: threshold iterations recorded per read for -verbose (default: 64)\n");
}

enum Kind { SWITCH, INT, LONG, DOUBLE, STRING, SIZE, IGNORED };  // IGNORED: takes a value and drops it
struct Flag {
    const char *name;
    Kind kind;
    void *to;
};

// the usage checks, in the order in which a command line with several mistakes reports them
static void check_usage(const Options &o)
{
    const long top = 1l << 28;
    if (o.weak_ends && o.verbose) die("rcorrector: usage: -weak-ends cannot be combined with -verbose (the transcript's entry point takes no weak-k-mer profile)\n");
    if ((o.depth_tags || o.depth) && o.verbose) die("rcorrector: usage: %s cannot be combined with -verbose (the transcript's entry point takes no k-mer depth)\n", o.depth_tags ? "-depth-tags" : "-depth");
    if (o.depth_max < 1 || o.depth_max > top) die("rcorrector: usage: -depth-max must be 1..%ld\n", top);
    if (o.dups && o.verbose) die("rcorrector: usage: -dups cannot be combined with -verbose (small batches through the transcript's entry point: run the census without it)\n");
    if (o.recurrent && o.verbose) die("rcorrector: usage: -recurrent cannot be combined with -verbose (small batches through the transcript's entry point: run the census without it)\n");
    if (o.recurrent && (o.recur_max < 1 || o.recur_max > top)) die("rcorrector: usage: -recurrent-max must be 1..%ld\n", top);
    if (o.recurrent && (o.recur_min < 1 || o.recur_min > o.recur_max)) die("rcorrector: usage: -recurrent-min must be 1..-recurrent-max\n");
    if (o.recurrent && (o.recur_top < 0 || o.recur_top > top)) die("rcorrector: usage: -recurrent-top must be 0..%ld\n", top);
    if (o.trust && o.verbose) die("rcorrector: usage: -trust-by-pos cannot be combined with -verbose (small batches through the transcript's entry point: run the profile without it)\n");
    if (o.overlap && o.verbose) die("rcorrector: usage: -overlap cannot be combined with -verbose (small batches through the transcript's entry point: run the report without it)\n");
    if (o.overlap && (o.overlap_min < 1 || o.overlap_min > 1023)) die("rcorrector: usage: -overlap-min must be 1..1023\n");
    if (o.overlap && (o.overlap_mm < 0 || o.overlap_mm > 50)) die("rcorrector: usage: -overlap-mm must be 0..50\n");
    if (o.dups && (o.dups_max < 1 || o.dups_max > top)) die("rcorrector: usage: -dups-max must be 1..%ld\n", top);
    if (o.weak_min < 1) die("rcorrector: usage: -weak-min must be at least 1\n");
    if ((o.histo || o.histo_after) && (o.histo_max < 1 || o.histo_max > top)) die("rcorrector: -histo-max must be 1..%ld\n", top);
    // what depends on the kinds of the inputs alone
    size_t single = 0;
    for (const Input &in : o.inputs) single += in.kind == 'r';
    if (o.dups && single && single != o.inputs.size())
        die("rcorrector: usage: -dups counts reads or pairs, not both in one census: give single-end files (-r) or paired ones (-p / -i), not a mix\n");
    if (o.overlap && single) die("rcorrector: usage: -overlap compares the two mates of a pair: give paired files (-p / -i), no single-end ones (-r)\n");
}

bool parse_options(int argc, char **argv, Options &o)
{
    const Flag flags[] = {
        {"-od", STRING, &o.od}, {"-c", STRING, &o.dump}, {"-k", INT, &o.k}, {"-t", INT, &o.t}, {"-maxcor", IGNORED, nullptr},
        {"-maxcorK", INT, &o.max_fix_per_k}, {"-wk", DOUBLE, &o.wk}, {"-stdout", SWITCH, &o.to_stdout}, {"-verbose", SWITCH, &o.verbose},
        {"-verbose-iter", INT, &o.trace_iter}, {"-gpus", INT, &o.gpus}, {"-batch", SIZE, &o.batch_reads}, {"-inflight", INT, &o.inflight},
        {"-write-dump", STRING, &o.write_dump}, {"-histo", STRING, &o.histo}, {"-histo-max", LONG, &o.histo_max},
        {"-histo-after", STRING, &o.histo_after}, {"-report", STRING, &o.report}, {"-dups", STRING, &o.dups}, {"-dups-max", LONG, &o.dups_max},
        {"-recurrent", STRING, &o.recurrent}, {"-recurrent-min", LONG, &o.recur_min}, {"-recurrent-top", LONG, &o.recur_top},
        {"-recurrent-max", LONG, &o.recur_max}, {"-trust-by-pos", STRING, &o.trust}, {"-overlap", STRING, &o.overlap},
        {"-overlap-min", INT, &o.overlap_min}, {"-overlap-mm", INT, &o.overlap_mm}, {"-weak-ends", SWITCH, &o.weak_ends},
        {"-weak-min", INT, &o.weak_min}, {"-depth-tags", SWITCH, &o.depth_tags}, {"-depth", STRING, &o.depth}, {"-depth-max", LONG, &o.depth_max},
        {"-packed", SWITCH, &o.packed},
    };
    if (argc == 1) {
        print_help();
        return false;
    }
    for (int i = 1; i < argc; ++i) {  // main.cpp:165-268
        const char *a = argv[i];
        auto value = [&]() -> const char * {
            if (i + 1 >= argc) die("rcorrector: usage: %s needs a value\n", a);
            return argv[++i];
        };
        if (!strcmp(a, "-h")) {
            print_help();
            return false;
        }
        if (!strcmp(a, "-r") || !strcmp(a, "-i") || !strcmp(a, "-p")) {
            Input in = {a[1], value(), nullptr};
            if (in.kind == 'p') in.mate = value();
            o.inputs.push_back(in);
            continue;
        }
        const Flag *f = std::find_if(std::begin(flags), std::end(flags), [&](const Flag &x) { return !strcmp(x.name, a); });
        if (f == std::end(flags)) {
            fprintf(stderr, "Unknown argument: %s\n", a);
            return false;
        }
        const char *v = f->kind == SWITCH ? nullptr : value();
        switch (f->kind) {
        case SWITCH: *(bool *)f->to = true; break;
        case INT: *(int *)f->to = atoi(v); break;
        case LONG: *(long *)f->to = atol(v); break;
        case DOUBLE: *(double *)f->to = atof(v); break;
        case STRING: *(const char **)f->to = v; break;
        case SIZE: *(size_t *)f->to = (size_t)atol(v); break;
        case IGNORED: break;
        }
        if (f->to == &o.od) mkdir(o.od, 0700);
        if (f->to == &o.inflight) o.inflight_given = true;
        if (f->to == &o.dump) {
            FILE *fp = fopen(o.dump, "r");
            if (!fp) die("Could not open file %s\n", o.dump);
            fclose(fp);
        }
    }
    check_usage(o);
    if (o.trace_iter < 1) o.trace_iter = 1;
    // -verbose carries RC_TRACE_ITER_WORDS x trace-iter words per read through host and device
    // (9 KB per read at the default 64 iterations): small batches, or a real data set needs tens of GB
    if (o.verbose && o.batch_reads > (1u << 16)) o.batch_reads = 1u << 16;
    if (o.gpus < 1) o.gpus = 1;
    o.inflight = std::min(std::max(o.inflight, 1), std::min(8, RC_MAX_SLOTS));
    if (o.batch_reads < 2) o.batch_reads = 2;
    o.batch_reads &= ~(size_t)1;
    const unsigned hc = std::thread::hardware_concurrency();
    // (default: 16 -- the loops these threads share are memory copies and page-cache calls, and beyond that
    // they get in each other's way: 16 M x 150 bp pairs, files to files, 0.53 / 0.50 / 0.49 / 0.51 / 0.52 / 0.62 s
    // at 8 / 12 / 16 / 20 / 24 / 32 threads on a 2 x 64-core host)
    o.threads = o.t > 1 ? o.t : (int)std::min<unsigned>(hc ? hc : 8, 16);
    if (const char *e = getenv("RC_TRANSPORT")) o.packed = o.packed || !strcmp(e, "packed");
    if (o.verbose) o.packed = false;  // (the transcript needs the traced entry point)
    if (const char *cm = getenv("RC_COUNT_MEM_MB")) o.count_mem = (uint64_t)atoll(cm) << 20;
    return true;
}
