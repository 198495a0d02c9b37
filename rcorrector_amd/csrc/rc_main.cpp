// rc_main.cpp -- `rcorrector`: stage 3 of run_rcorrector.pl on MI355X.  Same command line, stderr
// lines, output file names and *.cor.fq bytes as the reference's main.cpp (paths below are relative
// to /root/reference), with the per-read work done by librcorrector_amd.so (HIP) through its C ABI.
//
//   flags        main.cpp:50-71,165-268     -r/-p/-i/-c/-k/-od/-t/-maxcor/-maxcorK/-wk/-stdout/-verbose
//   file typing  Reads.h:108-162            first byte '>' FASTA, '@' FASTQ; ".gz" by the last two chars
//   output name  Reads.h:39-75,140-157      <od>/<name minus last extension>.cor.f[aq][.gz]
//   record       Reads.h:224-266,360-421    4 lines in; "<id> l:%d m:%d h:%d[ cor| unfixable_error]" out
//   batching     main.cpp:439-523           batches never span files; mates travel together
//
// Host pipeline: one reader thread cuts the input into batches of whole records
// (block reads, memchr line index, parallel packing into the SoA arenas of the C ABI), one worker
// threads per GPU run rc_submit / rc_wait on page-locked arenas, one writer thread formats in parallel and writes in input order.
//
// Extra flags (not in the reference): -gpus N shards batches over N GPUs (table replicated),
// -batch N sets the reads per batch, -inflight N the batches in flight per GPU (worker threads sharing
// the GPU's context through rc_submit / rc_wait slots: upload, kernels and download of consecutive
// batches overlap, and the GPU stays busy while a batch's slowest reads finish).  -t sets the host threads used
// for packing / formatting.
// -verbose prints the reference's per-read transcript (the -t 1 order) from rc_correct_batch_traced;
// -write-dump FILE keeps the k-mer table as jellyfish-dump text; without -c the k-mers are counted here.
// -histo FILE writes the k-mer count spectrum as `jellyfish histo` prints it (-histo-max: its last bin): without -c the
// spectrum of every k-mer counted, singletons included; with -c that of the dump's entries.
// -histo-after FILE writes the spectrum of the CORRECTED reads in the same format (a recount session, rcorrector_amd.h:
// rc_recount_begin) and adds one line to stderr: how many of their k-mers the table does not hold.
// -report FILE writes the correction report (rcorrector_amd.h: rc_change_report; rc_format.h: write_change_report): the
// substitutions by position, letters, quality class, mate and read, counted on the GPU as the batches complete.
// -weak-ends tags every record with the reference's dormant bad_prefix= / bad_suffix= fields (Reads.h:396-412), filled from the
// weak-k-mer profile of the corrected reads (rcorrector_amd.h: rc_read_weak; -weak-min: the count below which a k-mer is weak).
// -recurrent FILE writes the recurrent-correction census (rcorrector_amd.h: rc_recur_census; rc_format.h: write_recur_census): the
// sites -- 29 corrected bases around a change, and what it was corrected from -- at which the run made one fix in many reads.
// -dups FILE writes the duplicate census (rcorrector_amd.h: rc_dup_census; rc_format.h: write_dup_census): how many reads or
// pairs are exact copies of one another, as uploaded and as corrected, from 128-bit keys taken on the GPU as the batches complete.
// -trust-by-pos FILE writes the k-mer trust profile by read position (rcorrector_amd.h: rc_trust_profile; rc_format.h:
// write_trust_profile): the reads with a solid / weak k-mer window at every position from either end, per mate, as uploaded and
// as corrected, counted on the GPU as the batches complete (-weak-min: the count below which a k-mer is weak).
// -overlap FILE writes the mate-overlap report (rcorrector_amd.h: rc_mate_overlap; rc_format.h: write_mate_overlap): where mate 1
// and the reverse complement of mate 2 cover the same bases, the bases they disagree on before and after correction -- resolved,
// kept, introduced -- and the fragment lengths (-overlap-min / -overlap-mm: the shortest overlap and the most mismatches accepted).
// -depth-tags tags every record whose corrected read has a valid k-mer window with kdepth=Q1:MED:Q3, the quartiles of its k-mers'
// counts in the table (rcorrector_amd.h: rc_read_depth); -depth FILE writes the reads by median (rc_format.h: write_depth_report;
// -depth-max: its last bin).  Either adds one line to stderr.
#include <fcntl.h>
#include <malloc.h>
#include <sys/stat.h>
#include <unistd.h>

#include "rc_dispatch.h"

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

int main(int argc, char **argv)
{
    Run run;
    int &k = run.k, &gpus = run.gpus, &inflight = run.inflight;
    bool inflight_given = false;
    size_t &batch_reads = run.batch_reads;
    std::vector<ReadFile> &files = run.files, &mates = run.mates;
    int max_fix_per_k = 4, i;
    double wk = 0.95;
    const char *dump = nullptr, *write_dump = nullptr, *histo = nullptr, *histo_after = nullptr, *report = nullptr, *dups = nullptr, *trust = nullptr;
    const char *overlap = nullptr, *depth = nullptr, *recurrent = nullptr;
    long recur_min = 5, recur_top = 1000, recur_max = 10000;
    long depth_max = 10000;
    int overlap_min = 30, overlap_mm = 10;
    long dups_max = 10000;
    long histo_max = 10000;
    std::string od = "./";
    bool verbose = false;
    int t_flag = 0;
    if (argc == 1) {
        print_help();
        return 0;
    }
    g_timing = getenv("RC_TIMING") != nullptr;
    stamp("main() entered");
    for (i = 1; i < argc; ++i) {  // main.cpp:165-247
        if (!strcmp("-r", argv[i]) || !strcmp("-i", argv[i]))
            ++i;
        else if (!strcmp("-p", argv[i]))
            i += 2;
        else if (!strcmp("-od", argv[i])) {
            mkdir(argv[i + 1], 0700);
            od = argv[++i];
        } else if (!strcmp("-c", argv[i])) {
            dump = argv[++i];
            FILE *fp = fopen(dump, "r");
            if (!fp) die("Could not open file %s\n", dump);
            fclose(fp);
        } else if (!strcmp("-k", argv[i]))
            k = atoi(argv[++i]);
        else if (!strcmp("-t", argv[i]))
            t_flag = atoi(argv[++i]);
        else if (!strcmp("-maxcor", argv[i]))
            ++i;
        else if (!strcmp("-maxcorK", argv[i]))
            max_fix_per_k = atoi(argv[++i]);
        else if (!strcmp("-wk", argv[i]))
            wk = atof(argv[++i]);
        else if (!strcmp("-stdout", argv[i]))
            g_stdout = true;
        else if (!strcmp("-verbose", argv[i]))
            verbose = true;
        else if (!strcmp("-verbose-iter", argv[i]))
            g_trace_iter = atoi(argv[++i]);
        else if (!strcmp("-gpus", argv[i]))
            gpus = atoi(argv[++i]);
        else if (!strcmp("-batch", argv[i]))
            batch_reads = (size_t)atol(argv[++i]);
        else if (!strcmp("-inflight", argv[i])) {
            inflight = atoi(argv[++i]);
            inflight_given = true;
        }
        else if (!strcmp("-write-dump", argv[i]))
            write_dump = argv[++i];
        else if (!strcmp("-histo", argv[i]))
            histo = argv[++i];
        else if (!strcmp("-histo-max", argv[i]))
            histo_max = atol(argv[++i]);
        else if (!strcmp("-histo-after", argv[i]))
            histo_after = argv[++i];
        else if (!strcmp("-report", argv[i]))
            report = argv[++i];
        else if (!strcmp("-dups", argv[i]))
            dups = argv[++i];
        else if (!strcmp("-dups-max", argv[i]))
            dups_max = atol(argv[++i]);
        else if (!strcmp("-recurrent", argv[i]))
            recurrent = argv[++i];
        else if (!strcmp("-recurrent-min", argv[i]))
            recur_min = atol(argv[++i]);
        else if (!strcmp("-recurrent-top", argv[i]))
            recur_top = atol(argv[++i]);
        else if (!strcmp("-recurrent-max", argv[i]))
            recur_max = atol(argv[++i]);
        else if (!strcmp("-trust-by-pos", argv[i]))
            trust = argv[++i];
        else if (!strcmp("-overlap", argv[i]))
            overlap = argv[++i];
        else if (!strcmp("-overlap-min", argv[i]))
            overlap_min = atoi(argv[++i]);
        else if (!strcmp("-overlap-mm", argv[i]))
            overlap_mm = atoi(argv[++i]);
        else if (!strcmp("-weak-ends", argv[i]))
            run.weak_ends = true;
        else if (!strcmp("-weak-min", argv[i]))
            run.weak_min = atoi(argv[++i]);
        else if (!strcmp("-depth-tags", argv[i]))
            run.depth_tags = true;
        else if (!strcmp("-depth", argv[i]))
            depth = argv[++i];
        else if (!strcmp("-depth-max", argv[i]))
            depth_max = atol(argv[++i]);
        else if (!strcmp("-packed", argv[i]))
            g_packed = true;
        else if (!strcmp("-h", argv[i])) {
            print_help();
            return 0;
        } else {
            fprintf(stderr, "Unknown argument: %s\n", argv[i]);
            return 0;
        }
    }
    g_verbose = verbose;
    if (run.weak_ends && verbose) die("rcorrector: usage: -weak-ends cannot be combined with -verbose (the transcript's entry point takes no weak-k-mer profile)\n");
    if ((run.depth_tags || depth) && verbose) die("rcorrector: usage: %s cannot be combined with -verbose (the transcript's entry point takes no k-mer depth)\n", run.depth_tags ? "-depth-tags" : "-depth");
    if (depth_max < 1 || depth_max > (1l << 28)) die("rcorrector: usage: -depth-max must be 1..%ld\n", 1l << 28);
    run.depth_on = run.depth_tags || depth;
    run.depth_max = (uint32_t)depth_max;
    if (dups && verbose) die("rcorrector: usage: -dups cannot be combined with -verbose (small batches through the transcript's entry point: run the census without it)\n");
    if (recurrent && verbose) die("rcorrector: usage: -recurrent cannot be combined with -verbose (small batches through the transcript's entry point: run the census without it)\n");
    if (recurrent && (recur_max < 1 || recur_max > (1l << 28))) die("rcorrector: usage: -recurrent-max must be 1..%ld\n", 1l << 28);
    if (recurrent && (recur_min < 1 || recur_min > recur_max)) die("rcorrector: usage: -recurrent-min must be 1..-recurrent-max\n");
    if (recurrent && (recur_top < 0 || recur_top > (1l << 28))) die("rcorrector: usage: -recurrent-top must be 0..%ld\n", 1l << 28);
    if (trust && verbose) die("rcorrector: usage: -trust-by-pos cannot be combined with -verbose (small batches through the transcript's entry point: run the profile without it)\n");
    if (overlap && verbose) die("rcorrector: usage: -overlap cannot be combined with -verbose (small batches through the transcript's entry point: run the report without it)\n");
    if (overlap && (overlap_min < 1 || overlap_min > 1023)) die("rcorrector: usage: -overlap-min must be 1..1023\n");
    if (overlap && (overlap_mm < 0 || overlap_mm > 50)) die("rcorrector: usage: -overlap-mm must be 0..50\n");
    if (dups && (dups_max < 1 || dups_max > (1l << 28))) die("rcorrector: usage: -dups-max must be 1..%ld\n", 1l << 28);
    if (run.weak_min < 1) die("rcorrector: usage: -weak-min must be at least 1\n");
    if (g_trace_iter < 1) g_trace_iter = 1;
    // -verbose carries RC_TRACE_ITER_WORDS x trace-iter words per read through host and device
    // (9 KB per read at the default 64 iterations): small batches, or a real data set needs tens of GB
    if (verbose && batch_reads > (1u << 16)) batch_reads = 1u << 16;
    if ((histo || histo_after) && (histo_max < 1 || histo_max > (1l << 28))) die("rcorrector: -histo-max must be 1..%ld\n", 1l << 28);
    if (gpus < 1) gpus = 1;
    if (inflight < 1) inflight = 1;
    if (inflight > 8) inflight = 8;
    if (batch_reads < 2) batch_reads = 2;
    batch_reads &= ~(size_t)1;
    {
        unsigned hc = std::thread::hardware_concurrency();
        // (default: 16 -- the loops these threads share are memory copies and page-cache calls, and beyond that
        // they get in each other's way: 16 M x 150 bp pairs, files to files, 0.53 / 0.50 / 0.49 / 0.51 / 0.52 / 0.62 s
        // at 8 / 12 / 16 / 20 / 24 / 32 threads on a 2 x 64-core host)
        g_threads = t_flag > 1 ? t_flag : (int)std::min<unsigned>(hc ? hc : 8, 16);
        if (g_threads < 1) g_threads = 1;
    }
    g_timing = getenv("RC_TIMING") != nullptr;
    if (const char *e = getenv("RC_TRANSPORT")) g_packed = g_packed || !strcmp(e, "packed");
    if (verbose) g_packed = false;  // (the transcript needs the traced entry point)
    // batches recycle buffers of hundreds of MB: keep freed memory in the heap instead of handing it
    // back to the kernel and faulting it in again page by page (with dozens of threads every
    // mmap/munmap/page fault also serialises on the process's memory-map lock)
    mallopt(M_MMAP_THRESHOLD, 1 << 30);
    mallopt(M_TRIM_THRESHOLD, -1);

    files.reserve(MAX_READ_FILE);
    mates.reserve(MAX_READ_FILE);
    for (i = 1; i < argc; ++i) {  // main.cpp:250-268
        const bool is_in = !strcmp("-r", argv[i]) || !strcmp("-p", argv[i]) || !strcmp("-i", argv[i]);
        if (!is_in) continue;
        if (files.size() >= MAX_READ_FILE) die("The number of read files exceeds the limit %d.\n", MAX_READ_FILE);
        files.emplace_back();
        mates.emplace_back();
        if (!strcmp("-r", argv[i])) {
            open_file(files.back(), argv[i + 1], false, false, od);
            ++i;
        } else if (!strcmp("-p", argv[i])) {
            open_file(files.back(), argv[i + 1], true, false, od);
            open_file(mates.back(), argv[i + 2], true, false, od);
            if (files.back().fastq != mates.back().fastq)
                die("rcorrector: %s and %s are a FASTQ and a FASTA file: the mates of a pair must have the same format\n", argv[i + 1], argv[i + 2]);
            i += 2;
        } else {
            open_file(files.back(), argv[i + 1], false, true, od);
            ++i;
        }
    }

    // one context per GPU (the table is replicated across GPUs); `inflight` worker threads per GPU keep
    // that many batches in flight in it through rc_submit / rc_wait, one slot each
    if (inflight > RC_MAX_SLOTS) inflight = RC_MAX_SLOTS;
    run.lane_limit = inflight;
    if (!inflight_given && !verbose) {  // (Run::lane_limit) two at work, up to four where the GPU is what the writer waits for
        run.adaptive = true;
        inflight = RC_MAX_SLOTS;
    }
    const int nctx = gpus, nworkers = run.nworkers = gpus * inflight;
    run.submit_mu.reset(new std::mutex[(size_t)gpus]);
    std::vector<rc_ctx *> &ctx = run.ctx;
    ctx.assign((size_t)nctx, nullptr);
    // RC_SHARED_GPU=1 (tests): every "GPU" is device 0, so that the -gpus N path -- one table replica
    // per GPU, batches dealt to whichever context is free -- runs on a one-GPU box
    const bool shared_gpu = run.shared_gpu = getenv("RC_SHARED_GPU") != nullptr;
    const bool numa_on = run.numa_on = !(getenv("RC_NUMA") && !strcmp(getenv("RC_NUMA"), "0"));
    const bool lanes_env = getenv("RC_SLOT_LANES") != nullptr;
    rc_runtime_prepare(16);  // hardware queues for the slot lanes' streams: no thread exists yet, HIP has not started
    // The GPU runtime takes 0.08-0.25 s to come up (tools/mb/hipinit.hip): the contexts are created on a thread of their own,
    // and what needs no GPU goes ahead -- the test whether this is a one-pass run, as far as the host can say, and its reader.
    std::string ctx_err;
    std::thread ctx_thread([&]() {
        char err[512];
        for (int c = 0; c < nctx; ++c) {
            rc_config cfg = {shared_gpu ? 0 : c, k, max_fix_per_k};
            ctx[c] = rc_create(&cfg, err, sizeof err);
            if (!ctx[c]) {
                ctx_err = err;
                return;
            }
            // slot lanes (rcorrector_amd.h: rc_submit): off while the run is bound by its writer, which wants its batches back one
            // after the other (two batches side by side on the GPU each take twice as long: 25 M x 150 bp pairs, loop 0.60 against
            // 0.52 s); on from the moment the writer waits for the GPU (rc_dispatch: Run::lane_limit).  RC_SLOT_LANES decides if set.
            if (!lanes_env) rc_set_slot_lanes(ctx[c], run.adaptive ? 0 : 1);
        }
    });
    for (size_t fi = 0; fi < files.size(); ++fi)
        if ((files[fi].out_gz || (files[fi].paired && mates[fi].out_gz)) && !g_stdout) {
            const unsigned hc = std::thread::hardware_concurrency();
            g_deflate_threads = t_flag > 1 ? (size_t)t_flag : std::min<size_t>(hc ? hc / 2 : 8, 96);
        }
    // One pass (see ingest_resident): no dump, any number of GPUs (the batches are dealt to them as they are read), regular files (plain or .gz: one inflate pass instead of two) whose text
    // fits a third of the host memory that is available and whose bases, count scratch and table fit the HBM that is free.  RC_RESIDENT=0 keeps the two passes, =1 skips the size test.
    bool &resident = run.resident;
    std::vector<std::unique_ptr<Retained>> &kept = run.kept;
    const bool one_pass_shape = !dump && !verbose && !files.empty();
    uint64_t text_bytes = 0;
    bool plain = true, any_gz = false, host_fits = false;
    const char *res_env = getenv("RC_RESIDENT");
    if (one_pass_shape) {
        for (size_t fi = 0; fi < files.size(); ++fi)
            for (const ReadFile *f : {(const ReadFile *)&files[fi], files[fi].paired ? (const ReadFile *)&mates[fi] : (const ReadFile *)nullptr}) {
                if (!f) continue;
                struct stat st;
                if (f->src.is_gz) {  // (its text is taken as eight times the file: FASTQ deflates to a fifth or a quarter)
                    any_gz = true;
                    if (stat(f->path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) {
                        plain = false;
                        continue;
                    }
                    text_bytes += (uint64_t)st.st_size * 8;
                    continue;
                }
                if (!f->src.seekable || fstat(f->src.fd, &st) != 0) {
                    plain = false;
                    continue;
                }
                text_bytes += (uint64_t)st.st_size;
            }
        uint64_t avail = 0;
        if (FILE *mi = fopen("/proc/meminfo", "r")) {
            char ln[256];
            while (fgets(ln, sizeof ln, mi))
                if (!strncmp(ln, "MemAvailable:", 13)) avail = (uint64_t)atoll(ln + 13) << 10;
            fclose(mi);
        }
        for (const char *lim : {"/sys/fs/cgroup/memory.max", "/sys/fs/cgroup/memory/memory.limit_in_bytes"})  // a container's own limit
            if (FILE *cg = fopen(lim, "r")) {
                char ln[64];
                if (fgets(ln, sizeof ln, cg) && ln[0] >= '0' && ln[0] <= '9') avail = std::min<uint64_t>(avail, strtoull(ln, nullptr, 10));
                fclose(cg);
            }
        host_fits = plain && (res_env ? atoi(res_env) != 0 : text_bytes <= avail / 3);
        if (res_env && atoi(res_env) > 1) batch_reads = std::max<size_t>(2, (size_t)atoi(res_env)) & ~(size_t)1;  // (tests: RC_RESIDENT=<batch size>)
    }
    uint64_t count_mem = (uint64_t)24 << 30;
    if (const char *cm = getenv("RC_COUNT_MEM_MB")) count_mem = (uint64_t)atoll(cm) << 20;
    // The reader goes ahead where the answer is all but certain -- plain files (a .gz source cannot be rewound, and how it is
    // inflated depends on the answer), a text that leaves most of an MI355X's HBM free -- and where its buffers land on the right
    // NUMA node: one GPU means the host side is bound to that GPU's node, which sysfs can tell before HIP can.
    int node_guess = -2;
    bool ahead = host_fits && !any_gz && text_bytes + count_mem + ((uint64_t)1 << 30) <= ((uint64_t)160 << 30) && !getenv("RC_NO_READ_AHEAD");
    if (ahead && numa_on && gpus == 1) {
        node_guess = first_gpu_numa_node();
        if (node_guess == -2) ahead = false;
    }
    bool pool_started = false;
    HeadStats head;
    std::unique_ptr<Ingest> ingest;
    if (ahead) {
        if (numa_on && gpus == 1 && node_guess >= 0 && bind_to_numa_node(node_guess) && g_timing)
            fprintf(stderr, "[rc timing] host threads bound to NUMA node %d (the first GPU's, by sysfs)\n", node_guess);
        g_pool.start(std::max<size_t>((size_t)g_threads * 2, g_deflate_threads));
        pool_started = true;
        if (g_timing) fprintf(stderr, "[rc timing] the reader starts before the GPU runtime is up\n");
        head = head_stats(run);  // (before the reader takes the head of the first file out of its source)
        ingest.reset(new Ingest(run, batch_reads, true));
        ingest->depth = 8;
        ingest->start();
    }
    ctx_thread.join();
    if (!ctx_err.empty()) die("rcorrector: %s\n", ctx_err.c_str());
    // One GPU: the whole host pipeline -- reader, packers, formatters, writers and their buffers -- lives on the NUMA
    // node that GPU hangs off (every byte of a read crosses host memory a dozen times on its way through; across the
    // socket link each crossing costs more).  Several GPUs: each GPU's worker threads bind themselves (below).
    if (numa_on && gpus == 1) {
        const int node = rc_device_numa_node(ctx[0]);
        if (node >= 0 && node != node_guess && bind_to_numa_node(node) && g_timing)
            fprintf(stderr, "[rc timing] host threads bound to NUMA node %d%s\n", node, ahead ? " (sysfs had said another: the helper threads and the first blocks stay where they are)" : "");
    }
    // (the reader, the mate's reader and the workers call the pool side by side)
    if (!pool_started) g_pool.start(std::max<size_t>((size_t)g_threads * 2, g_deflate_threads));
    stamp("contexts created (HIP initialised, scratch allocated)");
    const double t_start = now_s();
    // While the table loads: the batch buffers of the pipeline -- text blocks, page-locked arenas, output slices --
    // are allocated, sized from the head of the first input, touched and registered with the GPU runtime here, so
    // that the first batches do not pay for a few GB of page faults and hipHostRegister calls one after the other
    run.max_in_flight = (size_t)(gpus * run.lane_limit + 2);
    if (one_pass_shape) {
        // HBM: the bases stay with the counter through the table build (about half of a FASTQ file's bytes), next to its
        // sort scratch (RC_COUNT_MEM_MB, 24 GiB by default) and the table itself, which the bases bound from above for
        // anything but a tiny input -- against what the device has free right now (another process may share it)
        // Several GPUs: every one of them holds its share of the bases, a sort scratch of its own and the staging of the
        // sharded count (rc_table_count_finish_sharded) -- priced as if each held everything, against the GPU with the
        // least free memory (a GPU another process shares must not run out in the middle of the count)
        uint64_t hbm_free = ~(uint64_t)0;
        for (int g = 0; g < gpus; ++g) {
            uint64_t f = 0;
            if (rc_device_memory(ctx[g], &f, nullptr)) f = 0;
            hbm_free = std::min(hbm_free, f);
        }
        if (const char *hf = getenv("RC_HBM_FREE_MB")) hbm_free = (uint64_t)atoll(hf) << 20;  // tests: as if this much were free
        const bool fits_hbm = text_bytes + count_mem + ((uint64_t)1 << 30) <= hbm_free;
        resident = plain && (res_env ? atoi(res_env) != 0 : (host_fits && fits_hbm));
        g_gz_whole = resident;
    }
    if (ahead && !resident) {  // the HBM is not free after all: two passes, from the start of the files
        ingest->abort();
        ingest.reset();
        for (size_t fi = 0; fi < files.size(); ++fi)
            for (ReadFile *f : {&files[fi], files[fi].paired ? &mates[fi] : (ReadFile *)nullptr}) {
                if (!f) continue;
                f->src.rewind();
                f->src.left.need(4096);
                f->src.left_len = f->src.fill(f->src.left.p, 4096);
            }
        if (g_timing) fprintf(stderr, "[rc timing] the reader had gone ahead for one pass; the device memory says two: started over\n");
        ahead = false;
    }
    // (the head of the first file is looked at here, not in the thread: the one-pass reader takes it out of the source)
    if (!ahead) head = head_stats(run);
    std::thread warm([&]() { warm_buffers(run, head); });
    int64_t stored = 0;
    // -histo without -c: the counter bins every k-mer it sees (on the first GPU's context, which holds a sharded count's result)
    if (histo && !dump && rc_table_count_spectrum(ctx[0], (uint32_t)histo_max)) die("rcorrector: %s\n", rc_last_error(ctx[0]));
    if (dump) {  // main.cpp:294-308: ONE Store, loaded once
        if (rc_table_load_jfdump(ctx[0], dump, &stored)) die("rcorrector: %s\n", rc_last_error(ctx[0]));
    } else {
        // no -c: stages 0-2 of run_rcorrector.pl:262-281 on the GPU -- count the canonical k-mers of
        // every input file (mates included), keep count >= 2, build the table
        std::vector<std::pair<std::string, bool>> inputs;  // path, fastq
        for (size_t fi = 0; fi < files.size(); ++fi) {
            inputs.emplace_back(files[fi].path, files[fi].fastq);
            if (files[fi].paired) inputs.emplace_back(mates[fi].path, mates[fi].fastq);
        }
        if (ahead)
            ingest->consume(&stored);
        else
            ingest_resident(run, resident ? batch_reads : std::max<size_t>(batch_reads, (size_t)1 << 20), &stored, resident);
        if (g_timing)
            fprintf(stderr, "[rc timing] k-mer counting pass over %zu file(s): %.2f s%s\n", inputs.size(), now_s() - t_start,
                    resident ? " (one pass: the text stays in host memory, the bases in HBM)" : "");
    }
    if (gpus > 1) {  // replicate the bucket array device to device (xGMI) and make sure the replicas agree
        uint64_t d0 = 0;
        if (rc_table_digest(ctx[0], &d0)) die("rcorrector: %s\n", rc_last_error(ctx[0]));
        for (int g = 1; g < gpus; ++g)  // every copy is queued before the first one is waited for: one per xGMI link
            if (rc_table_replicate_async(ctx[g], ctx[0])) die("rcorrector: %s\n", rc_last_error(ctx[g]));
        for (int g = 1; g < gpus; ++g) {
            uint64_t dg = 0;
            if (rc_sync(ctx[g]) || rc_table_digest(ctx[g], &dg)) die("rcorrector: %s\n", rc_last_error(ctx[g]));
            if (dg != d0) die("rcorrector: the k-mer table replica on GPU %d differs from the original\n", g);
        }
    }
    if (write_dump && rc_table_write_jfdump(ctx[0], write_dump, nullptr)) die("rcorrector: %s\n", rc_last_error(ctx[0]));
    if (histo) {
        std::vector<uint64_t> freq((size_t)histo_max + 1);
        if (rc_table_spectrum(ctx[0], dump ? 0 : 1, freq.data(), (uint32_t)histo_max, nullptr)) die("rcorrector: %s\n", rc_last_error(ctx[0]));
        if (!write_histo(histo, freq)) die("rcorrector: could not write %s\n", histo);
    }
    fprintf(stderr, "Stored %d kmers\n", (int)stored);
    double rate = 0.01;
    if (rc_estimate_error_rate(ctx[0], wk, &rate)) die("rcorrector: %s\n", rc_last_error(ctx[0]));
    fprintf(stderr, "Weak kmer threshold rate: %lf (estimated from %.3lf/1 of the chosen kmers)\n", rate, wk);
    stamp("ERROR_RATE known");

    // GetBadQuality, main.cpp:88-128: first <= 1M records of the primary files, in order
    char &bad_q = run.bad_q;
    if (!files.empty() && files[0].fastq) {
        std::vector<int32_t> fh(300, 0), lh(300, 0);
        int total = 0;
        if (resident) {  // the same records, from the blocks the counting pass kept (primary files, in order)
            for (const auto &R : kept) {
                if (total >= 1000000) break;
                quality_histograms(R->a, R->lpr_a, (size_t)(1000000 - total), fh, lh, &total);
            }
        } else {
            for (size_t fi = 0; fi < files.size() && total < 1000000; ++fi) {
                Source s;
                s.open(files[fi].path);
                Block b;
                const int lpr = files[fi].fastq ? 4 : 2;
                while (total < 1000000) {
                    take_records(s, std::min<size_t>((size_t)(1000000 - total), (size_t)1 << 18), lpr, b);
                    if (b.records == 0) break;
                    quality_histograms(b, lpr, b.records, fh, lh, &total);
                }
                s.close();
            }
        }
        bad_q = rc_bad_quality_from_hist(fh.data(), lh.data(), total);
    }
    fprintf(stderr, "Bad quality threshold is '%c'\n", bad_q);
    stamp("ERROR_RATE and bad quality known");
    for (int c = 0; c < nctx; ++c)
        if (rc_set_run_params(ctx[c], rate, bad_q)) die("rcorrector: %s\n", rc_last_error(ctx[c]));
    const double t_setup = now_s();
    stamp("start-up done");

    // -histo-after: a recount session on the first GPU's context.  One GPU: every batch that completes leaves its corrected
    // arena with the session, device to device (rc_recount_follow); several: the workers hand over the corrected text's bases.
    if (histo_after) {
        // the bases stay in HBM until the finish, next to its sort scratch: stop here rather than half-way if they will not fit
        uint64_t bases = 0;
        bool known = true;
        if (resident) {
            for (int c = 0; c < nctx; ++c) {
                size_t na = 0;
                if (rc_table_count_arenas(ctx[c], &na, nullptr, 0)) die("rcorrector: %s\n", rc_last_error(ctx[c]));
                std::vector<uint64_t> ab(na);
                if (na && rc_table_count_arenas(ctx[c], &na, ab.data(), na)) die("rcorrector: %s\n", rc_last_error(ctx[c]));
                for (uint64_t b : ab) bases += b;
            }
        } else {
            for (size_t fi = 0; fi < files.size(); ++fi)
                for (const ReadFile *f : {(const ReadFile *)&files[fi], files[fi].paired ? (const ReadFile *)&mates[fi] : (const ReadFile *)nullptr}) {
                    if (!f) continue;
                    struct stat st;
                    if (stat(f->path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) {
                        known = false;  // (a pipe: its size is anybody's guess, the session says so if it runs out)
                        continue;
                    }
                    // bases per byte of file: half of a FASTQ file, all of a FASTA file at most; deflated FASTQ is a fifth to a quarter of its text
                    const uint64_t text = f->src.is_gz ? (uint64_t)st.st_size * 5 : (uint64_t)st.st_size;
                    bases += f->fastq ? text / 2 + text / 16 : text;
                }
        }
        uint64_t hbm_free = 0;
        if (rc_device_memory(ctx[0], &hbm_free, nullptr)) die("rcorrector: %s\n", rc_last_error(ctx[0]));
        if (const char *hf = getenv("RC_HBM_FREE_MB")) hbm_free = (uint64_t)atoll(hf) << 20;  // tests: as if this much were free
        const uint64_t scratch = std::min<uint64_t>(count_mem, bases * 46);  // (the passes' scratch: rc_count.hip, 40 bytes per k-mer occurrence + 15 %)
        const uint64_t need = bases + scratch + ((uint64_t)256 << 20);
        if ((known || bases) && need > hbm_free)
            die("rcorrector: -histo-after keeps the corrected bases in GPU memory until the end of the run: about %llu MB with the counting scratch, "
                "%llu MB are free (lower RC_COUNT_MEM_MB, or run without -histo-after)\n", (unsigned long long)(need >> 20), (unsigned long long)(hbm_free >> 20));
        if (rc_recount_begin(ctx[0], (uint32_t)histo_max)) die("rcorrector: %s\n", rc_last_error(ctx[0]));
        if (gpus == 1) {
            if (rc_recount_follow(ctx[0], 1)) die("rcorrector: %s\n", rc_last_error(ctx[0]));
        } else {
            run.recount_host = true;
        }
    }

    // -report: every context counts the batches that complete on it, whatever the transport
    if (report)
        for (int c = 0; c < nctx; ++c)
            if (rc_change_report_begin(ctx[c])) die("rcorrector: %s\n", rc_last_error(ctx[c]));

    // -dups: every context keeps the keys of the batches that complete on it, whatever the transport
    if (dups) {
        size_t two = 0;
        for (const ReadFile &f : files) two += f.paired || f.interleaved;
        if (two && two != files.size())
            die("rcorrector: usage: -dups counts reads or pairs, not both in one census: give single-end files (-r) or paired ones (-p / -i), not a mix\n");
    }
    if (dups)
        for (int c = 0; c < nctx; ++c)
            if (rc_dup_census_begin(ctx[c])) die("rcorrector: %s\n", rc_last_error(ctx[c]));

    // -recurrent: every context keeps the site keys of the batches that complete on it, whatever the transport
    if (recurrent)
        for (int c = 0; c < nctx; ++c)
            if (rc_recur_census_begin(ctx[c])) die("rcorrector: %s\n", rc_last_error(ctx[c]));

    // -trust-by-pos: every context counts the batches that complete on it, whatever the transport
    if (trust)
        for (int c = 0; c < nctx; ++c)
            if (rc_trust_profile_begin(ctx[c], run.weak_min)) die("rcorrector: %s\n", rc_last_error(ctx[c]));

    // -overlap: every context counts the batches of pairs that complete on it, whatever the transport
    if (overlap) {
        for (const ReadFile &f : files)
            if (!f.paired && !f.interleaved)
                die("rcorrector: usage: -overlap compares the two mates of a pair: give paired files (-p / -i), no single-end ones (-r)\n");
        for (int c = 0; c < nctx; ++c)
            if (rc_mate_overlap_begin(ctx[c], overlap_min, overlap_mm)) die("rcorrector: %s\n", rc_last_error(ctx[c]));
    }

    // pipeline: reader (this thread) -> `inflight` workers per GPU -> writer thread (input order)
    warm.join();
    stamp("batch buffers ready");
    run_pipeline(run);
    const double t_loop_end = now_s();

    for (size_t fi = 0; fi < files.size(); ++fi) {
        for (ReadFile *f : {&files[fi], &mates[fi]}) {
            if (f->out && f->out_gz && !f->wrote) {  // an empty .gz is still one (empty) gzip member
                OutBuf none, z;
                gzip_member(none, z);
                std::vector<OutBuf> one(1);
                one[0].swap(z);
                emit_slices(*f, one);
            }
            if (f->out && f->out != stdout && f->preallocated && ftruncate(fileno(f->out), f->out_off) != 0)
                die("ERROR: could not set the length of the output of %s\n", f->path.c_str());
            if (f->out && f->out != stdout) fclose(f->out);
            f->src.close();
        }
    }
    // (the contexts are not torn down: the process ends here, and releasing gigabytes of device and
    // host memory piece by piece costs more than everything else after the last write)
    if (g_timing)
        fprintf(stderr, "[rc timing] start-up (dump load, table build, ERROR_RATE, bad quality) %.2f s; correction loop (read, correct, write) %.2f s; %d host threads\n",
                t_setup - t_start, t_loop_end - t_setup, g_threads);
    if (g_timing)
        fprintf(stderr, "[rc timing] stage totals: read+index %.2f s (reader thread); pack %.2f s + correct_batch %.2f s + format %.2f s (sum over %d worker threads); write %.2f s (writer thread)\n",
                g_t_read, g_t_pack, g_t_gpu, g_t_format, nworkers, g_t_write);
    if (g_timing) fprintf(stderr, "[rc timing] inside read+index (all files, thread-seconds): pread %.2f s, newline scan %.2f s, line index %.2f s\n", g_t_fill, g_t_nl, g_t_idx);
    if (g_timing)
        fprintf(stderr, "[rc timing] blocked: reader %.2f s (no free slot), workers %.2f s (no batch), writer %.2f s (next batch not done)\n", g_w_reader, g_w_worker, g_w_writer);
    fprintf(stderr, "Processed %llu reads\n\tCorrected %llu bases.\n", (unsigned long long)run.total_reads, (unsigned long long)run.total_cor);
    if (run.weak_ends)
        fprintf(stderr, "Weak ends (k-mers counted below %d): %llu reads with a bad prefix, %llu with a bad suffix, %llu without a solid k-mer\n", run.weak_min,
                (unsigned long long)run.weak_prefix, (unsigned long long)run.weak_suffix, (unsigned long long)run.weak_nosolid);
    if (run.depth_on) {
        const uint64_t with = run.depth_reads[0] + run.depth_reads[1] - run.depth_novalid[0] - run.depth_novalid[1];
        const uint64_t zero = (run.depth_hist[0].empty() ? 0 : run.depth_hist[0][0]) + (run.depth_hist[1].empty() ? 0 : run.depth_hist[1][0]);
        const size_t mm = depth_median_of_medians(run.depth_hist);
        fprintf(stderr, "K-mer depth: %llu reads with a valid k-mer window, %llu of them with a median of 0; the median of the reads' medians is %zu%s\n",
                (unsigned long long)with, (unsigned long long)zero, mm, with && mm == (size_t)run.depth_max ? " or more (the last bin, -depth-max)" : "");
        if (depth) {
            bool two_mates = false;
            for (const ReadFile &f : files) two_mates = two_mates || f.paired || f.interleaved;
            if (!write_depth_report(depth, k, run.depth_reads, run.depth_novalid, run.depth_hist, two_mates)) die("rcorrector: could not write %s\n", depth);
        }
    }
    if (report) {  // the contexts' reports, added up
        std::vector<rc_change_report> part(1), sum(1);
        memset(&sum[0], 0, sizeof sum[0]);
        for (int c = 0; c < nctx; ++c) {
            if (rc_change_report_get(ctx[c], &part[0])) die("rcorrector: %s\n", rc_last_error(ctx[c]));
            const uint64_t *src = reinterpret_cast<const uint64_t *>(&part[0]);
            uint64_t *dst = reinterpret_cast<uint64_t *>(&sum[0]);
            for (size_t w = 0; w < sizeof(rc_change_report) / sizeof(uint64_t); ++w) dst[w] += src[w];
        }
        bool two_mates = false;
        for (const ReadFile &f : files) two_mates = two_mates || f.paired || f.interleaved;
        if (!write_change_report(report, sum[0], two_mates)) die("rcorrector: could not write %s\n", report);
    }
    if (dups) {  // the contexts' keys, merged into the first
        const double td0 = now_s();
        for (int c = 1; c < nctx; ++c)
            if (rc_dup_census_merge(ctx[0], ctx[c])) die("rcorrector: %s\n", rc_last_error(ctx[0]));
        std::vector<uint64_t> before((size_t)dups_max + 1), after((size_t)dups_max + 1);
        rc_dup_census dc;
        dc.copies_before = before.data();
        dc.copies_after = after.data();
        if (rc_dup_census_get(ctx[0], (uint32_t)dups_max, &dc)) die("rcorrector: %s\n", rc_last_error(ctx[0]));
        size_t two = 0;
        for (const ReadFile &f : files) two += f.paired || f.interleaved;
        const char *unit = two ? "pairs" : "reads";  // (all of one kind: checked before the run)
        if (!write_dup_census(dups, dc, (uint32_t)dups_max, unit)) die("rcorrector: could not write %s\n", dups);
        if (g_timing) fprintf(stderr, "[rc timing] -dups: merge, sort and census %.2f s\n", now_s() - td0);
        const double u = dc.units ? (double)dc.units : 1.0;
        fprintf(stderr, "Duplicates: %llu %s, %llu distinct before correction (duplicate fraction %.4f), %llu after (%.4f)\n", (unsigned long long)dc.units, unit,
                (unsigned long long)dc.distinct_before, dc.units ? 1.0 - (double)dc.distinct_before / u : 0.0, (unsigned long long)dc.distinct_after,
                dc.units ? 1.0 - (double)dc.distinct_after / u : 0.0);
    }
    if (recurrent) {  // the contexts' keys, merged into the first
        const double tr0 = now_s();
        for (int c = 1; c < nctx; ++c)
            if (rc_recur_census_merge(ctx[0], ctx[c])) die("rcorrector: %s\n", rc_last_error(ctx[0]));
        std::vector<uint64_t> bins((size_t)recur_max + 1), tk((size_t)recur_top + 1), tc((size_t)recur_top + 1);
        rc_recur_census rcs;
        rcs.recur = bins.data();
        rcs.top_key = tk.data();
        rcs.top_count = tc.data();
        if (rc_recur_census_get(ctx[0], (uint32_t)recur_max, (uint32_t)recur_min, (uint32_t)recur_top, &rcs)) die("rcorrector: %s\n", rc_last_error(ctx[0]));
        if (!write_recur_census(recurrent, rcs, (uint32_t)recur_max, (uint32_t)recur_min)) die("rcorrector: could not write %s\n", recurrent);
        if (g_timing) fprintf(stderr, "[rc timing] -recurrent: merge, sort and census %.2f s\n", now_s() - tr0);
        // (the bins below -recurrent-min are exact, -recurrent-min <= -recurrent-max: what is not in them repeats that often)
        uint64_t few_sites = 0, few_changes = 0;
        for (long c = 1; c < recur_min; ++c) {
            few_sites += bins[(size_t)c];
            few_changes += bins[(size_t)c] * (uint64_t)c;
        }
        fprintf(stderr, "Recurrent corrections: %llu contexted changes at %llu sites; %llu changes at %llu sites corrected at least %ld times\n",
                (unsigned long long)rcs.contexted, (unsigned long long)rcs.sites, (unsigned long long)(rcs.contexted - few_changes),
                (unsigned long long)(rcs.sites - few_sites), recur_min);
    }
    if (trust) {  // the contexts' counts, added up
        std::vector<rc_trust_profile> tp(2);
        for (int c = 0; c < nctx; ++c) {
            if (rc_trust_profile_get(ctx[c], &tp[c ? 1 : 0])) die("rcorrector: %s\n", rc_last_error(ctx[c]));
            if (c) add_trust_profile(tp[0], tp[1]);
            if (rc_trust_profile_end(ctx[c])) die("rcorrector: %s\n", rc_last_error(ctx[c]));
        }
        bool two_mates = false;
        for (const ReadFile &f : files) two_mates = two_mates || f.paired || f.interleaved;
        if (!write_trust_profile(trust, tp[0], two_mates)) die("rcorrector: could not write %s\n", trust);
        uint64_t valid[2] = {0, 0}, weak[2] = {0, 0};
        const rc_trust_counts *ver[2] = {&tp[0].before, &tp[0].after};
        for (int v = 0; v < 2; ++v)
            for (int m = 0; m < 2; ++m)
                for (int p = 0; p < RC_TRUST_MAX_LEN; ++p) {
                    weak[v] += ver[v]->weak5[m][p];
                    valid[v] += ver[v]->weak5[m][p] + ver[v]->solid5[m][p];
                }
        fprintf(stderr, "Trust by position (k-mers counted below %d are weak): %llu of %llu valid k-mer windows weak before correction (%.4f), %llu of %llu after (%.4f)\n",
                run.weak_min, (unsigned long long)weak[0], (unsigned long long)valid[0], valid[0] ? (double)weak[0] / (double)valid[0] : 0.0,
                (unsigned long long)weak[1], (unsigned long long)valid[1], valid[1] ? (double)weak[1] / (double)valid[1] : 0.0);
    }
    if (overlap) {  // the contexts' counts, added up
        std::vector<rc_mate_overlap> mo(2);
        for (int c = 0; c < nctx; ++c) {
            if (rc_mate_overlap_get(ctx[c], &mo[c ? 1 : 0])) die("rcorrector: %s\n", rc_last_error(ctx[c]));
            if (c) add_mate_overlap(mo[0], mo[1]);
            if (rc_mate_overlap_end(ctx[c])) die("rcorrector: %s\n", rc_last_error(ctx[c]));
        }
        if (!write_mate_overlap(overlap, mo[0])) die("rcorrector: could not write %s\n", overlap);
        const rc_mate_overlap &M = mo[0];
        fprintf(stderr, "Mate overlap (at least %d bases, at most %d %% mismatches): %llu of %llu pairs overlap; %llu of %llu compared bases disagree before correction (%.6f), %llu of %llu after (%.6f); %llu introduced\n",
                overlap_min, overlap_mm, (unsigned long long)M.overlapping, (unsigned long long)M.pairs, (unsigned long long)M.disagree_before,
                (unsigned long long)M.compared_before, M.compared_before ? (double)M.disagree_before / (double)M.compared_before : 0.0,
                (unsigned long long)M.disagree_after, (unsigned long long)M.compared_after,
                M.compared_after ? (double)M.disagree_after / (double)M.compared_after : 0.0, (unsigned long long)M.introduced);
    }
    if (histo_after) {
        const double th0 = now_s();
        std::vector<uint64_t> freq((size_t)histo_max + 1);
        rc_recount_stats rs;
        if (rc_recount_finish(ctx[0], freq.data(), &rs)) die("rcorrector: %s\n", rc_last_error(ctx[0]));
        if (!write_histo(histo_after, freq)) die("rcorrector: could not write %s\n", histo_after);
        if (g_timing) fprintf(stderr, "[rc timing] -histo-after: recount of the corrected reads %.2f s\n", now_s() - th0);
        fprintf(stderr, "Corrected reads: %llu distinct k-mers, %llu seen once, %llu not in the table (%llu occurrences)\n", (unsigned long long)rs.all.distinct,
                (unsigned long long)rs.all.unique, (unsigned long long)rs.absent_distinct, (unsigned long long)rs.absent_total);
    }
    stamp("outputs closed, leaving");
    if (getenv("RC_TEARDOWN")) {  // dev: where the time between _exit and the parent's wait goes
        run.pool.clear();
        run.warm_jobs.clear();
        run.order.clear();
        run.q.clear();
        stamp("teardown: job buffers unregistered and freed");
        for (rc_ctx *c : ctx) rc_destroy(c);
        stamp("teardown: contexts destroyed");
        if (atoi(getenv("RC_TEARDOWN")) >= 2) {  // ... and what is left once the helper threads, the heap and the HIP runtime are gone too
            g_pool.stop_and_join();
            stamp("teardown: helper threads joined");
            malloc_trim(0);
            stamp("teardown: heap trimmed");
            if (void *h = dlopen("libamdhip64.so", RTLD_NOW | RTLD_NOLOAD)) {
                typedef int (*reset_fn)();
                if (reset_fn f = (reset_fn)dlsym(h, "hipDeviceReset")) f();
                stamp("teardown: hipDeviceReset");
            }
            if (FILE *sm = fopen("/proc/self/smaps", "r")) {  // the largest resident mappings that are left
                std::vector<std::pair<long, std::string>> maps;
                char ln[512];
                std::string head;
                while (fgets(ln, sizeof ln, sm)) {
                    if (strchr(ln, '-') && strchr(ln, '-') < ln + 20 && !strstr(ln, "kB")) head = ln;
                    if (!strncmp(ln, "Rss:", 4)) maps.emplace_back(atol(ln + 4), head);
                }
                fclose(sm);
                std::sort(maps.begin(), maps.end(), [](const std::pair<long, std::string> &a, const std::pair<long, std::string> &b) { return a.first > b.first; });
                for (size_t i2 = 0; i2 < maps.size() && i2 < 8; ++i2) fprintf(stderr, "[rc timing] at exit %8ld kB resident: %s", maps[i2].first, maps[i2].second.c_str());
            }
            if (FILE *st = fopen("/proc/self/status", "r")) {
                char ln[256];
                while (fgets(ln, sizeof ln, st))
                    if (!strncmp(ln, "VmRSS:", 6) || !strncmp(ln, "RssAnon:", 8) || !strncmp(ln, "RssFile:", 8) || !strncmp(ln, "RssShmem:", 9) || !strncmp(ln, "Threads:", 8) || !strncmp(ln, "VmPTE:", 6))
                        fprintf(stderr, "[rc timing] at exit %s", ln);
                fclose(st);
            }
        }
    }
    fflush(NULL);
    _exit(0);  // every output is closed: skip unmapping gigabytes of buffers one by one
}
