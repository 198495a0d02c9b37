// rc_main.cpp -- `rcorrector`: stage 3 of run_rcorrector.pl on MI355X.  Same command line, stderr
// lines, output file names and *.cor.fq bytes as the reference's main.cpp (paths below are relative
// to /root/reference), with the per-read work done by librcorrector_amd.so (HIP) through its C ABI.
//
//   flags        main.cpp:50-71,165-268     rc_options.h: one table, one parse, every usage check
//   file typing  Reads.h:108-162            first byte '>' FASTA, '@' FASTQ; ".gz" by the last two chars
//   output name  Reads.h:39-75,140-157      <od>/<name minus last extension>.cor.f[aq][.gz]
//   record       Reads.h:224-266,360-421    4 lines in; "<id> l:%d m:%d h:%d[ cor| unfixable_error]" out
//   batching     main.cpp:439-523           batches never span files; mates travel together
//   extra outputs (not in the reference)    rc_outputs.h: -histo-after, -report, -weak-ends, -depth, -dups, -recurrent, ...
//
// Host pipeline: one reader thread cuts the input into batches of whole records
// (block reads, memchr line index, parallel packing into the SoA arenas of the C ABI), one worker
// threads per GPU run rc_submit / rc_wait on page-locked arenas, one writer thread formats in parallel and writes in input order.
//
// This file is the start-up and the exit around that pipeline, one function per stage, in main()'s order: parse -> mallopt ->
// open files -> context thread (after rc_runtime_prepare) -> size the inputs -> reader ahead? -> join contexts, bind NUMA,
// start the pool -> one pass? (rewind if the reader was wrong) -> head stats, warm thread -> load the dump or count ->
// replicate -> -write-dump, -histo -> error rate -> bad quality -> run params -> outputs_begin -> run_pipeline -> close ->
// timing lines -> outputs_finish -> RC_TEARDOWN report -> _exit.  parse_options and the checks on the kinds of the inputs come
// before rc_runtime_prepare and before any other rc_* call: a usage error is answered without a GPU.
#include <fcntl.h>
#include <malloc.h>
#include <sys/stat.h>
#include <unistd.h>

#include "rc_outputs.h"

// what the stages between the first file opened and the first batch share
struct Startup {
    std::thread ctx_thread;
    std::string ctx_err;
    bool one_pass_shape = false, plain = true, any_gz = false, host_fits = false;
    uint64_t text_bytes = 0;  // the inputs' text, as far as the file sizes tell
    const char *res_env = nullptr;  // RC_RESIDENT
    bool ahead = false, pool_started = false;  // the reader has gone ahead of the GPU runtime
    int node_guess = -2;
    HeadStats head;
    std::unique_ptr<Ingest> ingest;
    double t_start = 0, t_setup = 0, t_loop_end = 0;
};

static void ok(rc_ctx *c, int failed)
{
    if (failed) die("rcorrector: %s\n", rc_last_error(c));
}

// the options, where the units of the pipeline read them
static void apply_options(const Options &o, Run &run)
{
    g_stdout = o.to_stdout;
    g_verbose = o.verbose;
    g_trace_iter = o.trace_iter;
    g_threads = o.threads;
    g_packed = o.packed;
    run.k = o.k;
    run.gpus = o.gpus;
    run.batch_reads = o.batch_reads;
    run.weak_ends = o.weak_ends;
    run.weak_min = o.weak_min;
    run.depth_tags = o.depth_tags;
    run.depth_on = o.depth_tags || o.depth;
    run.depth_max = (uint32_t)o.depth_max;
    // one context per GPU (the table is replicated across GPUs); `inflight` worker threads per GPU keep
    // that many batches in flight in it through rc_submit / rc_wait, one slot each
    run.inflight = run.lane_limit = o.inflight;
    if (!o.inflight_given && !o.verbose) {  // (Run::lane_limit) two at work, up to four where the GPU is what the writer waits for
        run.adaptive = true;
        run.inflight = RC_MAX_SLOTS;
    }
    run.nworkers = run.gpus * run.inflight;
    run.max_in_flight = (size_t)(run.gpus * run.lane_limit + 2);
    run.submit_mu.reset(new std::mutex[(size_t)run.gpus]);
    run.ctx.assign((size_t)run.gpus, nullptr);
    // RC_SHARED_GPU=1 (tests): every "GPU" is device 0, so that the -gpus N path -- one table replica
    // per GPU, batches dealt to whichever context is free -- runs on a one-GPU box
    run.shared_gpu = getenv("RC_SHARED_GPU") != nullptr;
    run.numa_on = !(getenv("RC_NUMA") && !strcmp(getenv("RC_NUMA"), "0"));
}

static void open_inputs(const Options &o, Run &run)  // main.cpp:250-268
{
    run.files.reserve(MAX_READ_FILE);
    run.mates.reserve(MAX_READ_FILE);
    for (const Input &in : o.inputs) {
        if (run.files.size() >= MAX_READ_FILE) die("The number of read files exceeds the limit %d.\n", MAX_READ_FILE);
        run.files.emplace_back();
        run.mates.emplace_back();
        open_file(run.files.back(), in.path, in.kind == 'p', in.kind == 'i', o.od);
        if (in.kind != 'p') continue;
        open_file(run.mates.back(), in.mate, true, false, o.od);
        if (run.files.back().fastq != run.mates.back().fastq)
            die("rcorrector: %s and %s are a FASTQ and a FASTA file: the mates of a pair must have the same format\n", in.path, in.mate);
    }
    for_each_input(run, [&](const ReadFile &f) {
        if (!f.out_gz || g_stdout) return;
        const unsigned hc = std::thread::hardware_concurrency();
        g_deflate_threads = o.t > 1 ? (size_t)o.t : std::min<size_t>(hc ? hc / 2 : 8, 96);
    });
}

// The GPU runtime takes 0.08-0.25 s to come up (tools/mb/hipinit.hip): the contexts are created on a thread of their own,
// and what needs no GPU goes ahead -- the test whether this is a one-pass run, as far as the host can say, and its reader.
static void start_contexts(Startup &s, Run &run, const Options &o)
{
    const bool lanes_env = getenv("RC_SLOT_LANES") != nullptr;
    rc_runtime_prepare(16);  // hardware queues for the slot lanes' streams: no thread exists yet, HIP has not started
    s.ctx_thread = std::thread([&s, &run, &o, lanes_env]() {
        char err[512];
        for (int c = 0; c < run.gpus; ++c) {
            rc_config cfg = {run.shared_gpu ? 0 : c, run.k, o.max_fix_per_k};
            run.ctx[c] = rc_create(&cfg, err, sizeof err);
            if (!run.ctx[c]) {
                s.ctx_err = err;
                return;
            }
            // slot lanes (rcorrector_amd.h: rc_submit): off while the run is bound by its writer, which wants its batches back one
            // after the other (two batches side by side on the GPU each take twice as long: 25 M x 150 bp pairs, loop 0.60 against
            // 0.52 s); on from the moment the writer waits for the GPU (rc_dispatch: Run::lane_limit).  RC_SLOT_LANES decides if set.
            if (!lanes_env) rc_set_slot_lanes(run.ctx[c], run.adaptive ? 0 : 1);
        }
    });
}

// One pass (see ingest_resident): no dump, any number of GPUs (the batches are dealt to them as they are read), regular files (plain or .gz: one inflate pass instead of two) whose text
// fits a third of the host memory that is available and whose bases, count scratch and table fit the HBM that is free.  RC_RESIDENT=0 keeps the two passes, =1 skips the size test.
static void size_inputs(Startup &s, Run &run, const Options &o)
{
    s.one_pass_shape = !o.dump && !o.verbose && !run.files.empty();
    s.res_env = getenv("RC_RESIDENT");
    if (!s.one_pass_shape) return;
    for_each_input(run, [&](const ReadFile &f) {
        struct stat st;
        if (f.src.is_gz) {  // (its text is taken as eight times the file: FASTQ deflates to a fifth or a quarter)
            s.any_gz = true;
            if (stat(f.path.c_str(), &st) != 0 || !S_ISREG(st.st_mode))
                s.plain = false;
            else
                s.text_bytes += (uint64_t)st.st_size * 8;
        } else if (!f.src.seekable || fstat(f.src.fd, &st) != 0)
            s.plain = false;
        else
            s.text_bytes += (uint64_t)st.st_size;
    });
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
    s.host_fits = s.plain && (s.res_env ? atoi(s.res_env) != 0 : s.text_bytes <= avail / 3);
    if (s.res_env && atoi(s.res_env) > 1) run.batch_reads = std::max<size_t>(2, (size_t)atoi(s.res_env)) & ~(size_t)1;  // (tests: RC_RESIDENT=<batch size>)
}

// (the reader, the mate's reader and the workers call the pool side by side)
static void start_pool(Startup &s)
{
    if (!s.pool_started) g_pool.start(std::max<size_t>((size_t)g_threads * 2, g_deflate_threads));
    s.pool_started = true;
}

// The reader goes ahead where the answer is all but certain -- plain files (a .gz source cannot be rewound, and how it is
// inflated depends on the answer), a text that leaves most of an MI355X's HBM free -- and where its buffers land on the right
// NUMA node: one GPU means the host side is bound to that GPU's node, which sysfs can tell before HIP can.
static void start_reader_ahead(Startup &s, Run &run, const Options &o)
{
    s.ahead = s.host_fits && !s.any_gz && s.text_bytes + o.count_mem + ((uint64_t)1 << 30) <= ((uint64_t)160 << 30) && !getenv("RC_NO_READ_AHEAD");
    if (s.ahead && run.numa_on && run.gpus == 1) {
        s.node_guess = first_gpu_numa_node();
        if (s.node_guess == -2) s.ahead = false;
    }
    if (!s.ahead) return;
    if (run.numa_on && run.gpus == 1 && s.node_guess >= 0 && bind_to_numa_node(s.node_guess) && g_timing)
        fprintf(stderr, "[rc timing] host threads bound to NUMA node %d (the first GPU's, by sysfs)\n", s.node_guess);
    start_pool(s);
    if (g_timing) fprintf(stderr, "[rc timing] the reader starts before the GPU runtime is up\n");
    s.head = head_stats(run);  // (before the reader takes the head of the first file out of its source)
    s.ingest.reset(new Ingest(run, run.batch_reads, true));
    s.ingest->depth = 8;
    s.ingest->start();
}

static void join_contexts(Startup &s, Run &run)
{
    s.ctx_thread.join();
    if (!s.ctx_err.empty()) die("rcorrector: %s\n", s.ctx_err.c_str());
    // One GPU: the whole host pipeline -- reader, packers, formatters, writers and their buffers -- lives on the NUMA
    // node that GPU hangs off (every byte of a read crosses host memory a dozen times on its way through; across the
    // socket link each crossing costs more).  Several GPUs: each GPU's worker threads bind themselves (rc_dispatch).
    if (run.numa_on && run.gpus == 1) {
        const int node = rc_device_numa_node(run.ctx[0]);
        if (node >= 0 && node != s.node_guess && bind_to_numa_node(node) && g_timing)
            fprintf(stderr, "[rc timing] host threads bound to NUMA node %d%s\n", node, s.ahead ? " (sysfs had said another: the helper threads and the first blocks stay where they are)" : "");
    }
    start_pool(s);
    stamp("contexts created (HIP initialised, scratch allocated)");
    s.t_start = now_s();
}

static void decide_one_pass(Startup &s, Run &run, const Options &o)
{
    if (s.one_pass_shape) {
        // HBM: the bases stay with the counter through the table build (about half of a FASTQ file's bytes), next to its
        // sort scratch (RC_COUNT_MEM_MB, 24 GiB by default) and the table itself, which the bases bound from above for
        // anything but a tiny input -- against what the device has free right now (another process may share it)
        // Several GPUs: every one of them holds its share of the bases, a sort scratch of its own and the staging of the
        // sharded count (rc_table_count_finish_sharded) -- priced as if each held everything, against the GPU with the
        // least free memory (a GPU another process shares must not run out in the middle of the count)
        const bool fits_hbm = s.text_bytes + o.count_mem + ((uint64_t)1 << 30) <= hbm_free(run, false);
        run.resident = s.plain && (s.res_env ? atoi(s.res_env) != 0 : (s.host_fits && fits_hbm));
        g_gz_whole = run.resident;
    }
    if (s.ahead && !run.resident) {  // the HBM is not free after all: two passes, from the start of the files
        s.ingest->abort();
        s.ingest.reset();
        for_each_input(run, [](ReadFile &f) {
            f.src.rewind();
            f.src.left.need(4096);
            f.src.left_len = f.src.fill(f.src.left.p, 4096);
        });
        if (g_timing) fprintf(stderr, "[rc timing] the reader had gone ahead for one pass; the device memory says two: started over\n");
        s.ahead = false;
    }
    // (the head of the first file is looked at here, not in the warm thread: the one-pass reader takes it out of the source)
    if (!s.ahead) s.head = head_stats(run);
}

// the k-mer table on the first GPU: the dump (main.cpp:294-308: ONE Store, loaded once), or -- no -c -- stages 0-2 of
// run_rcorrector.pl:262-281 on the GPU: count the canonical k-mers of every input file (mates included), keep count >= 2
static int64_t load_or_count(Startup &s, Run &run, const Options &o)
{
    int64_t stored = 0;
    // -histo without -c: the counter bins every k-mer it sees (on the first GPU's context, which holds a sharded count's result)
    if (o.histo && !o.dump) ok(run.ctx[0], rc_table_count_spectrum(run.ctx[0], (uint32_t)o.histo_max));
    if (o.dump) {
        ok(run.ctx[0], rc_table_load_jfdump(run.ctx[0], o.dump, &stored));
        return stored;
    }
    if (s.ahead)
        s.ingest->consume(&stored);
    else
        ingest_resident(run, run.resident ? run.batch_reads : std::max<size_t>(run.batch_reads, (size_t)1 << 20), &stored, run.resident);
    size_t inputs = 0;
    for_each_input(run, [&](const ReadFile &) { ++inputs; });
    if (g_timing)
        fprintf(stderr, "[rc timing] k-mer counting pass over %zu file(s): %.2f s%s\n", inputs, now_s() - s.t_start,
                run.resident ? " (one pass: the text stays in host memory, the bases in HBM)" : "");
    return stored;
}

// several GPUs: replicate the bucket array device to device (xGMI) and make sure the replicas agree
static void replicate_table(Run &run)
{
    uint64_t d0 = 0;
    ok(run.ctx[0], rc_table_digest(run.ctx[0], &d0));
    for (int g = 1; g < run.gpus; ++g)  // every copy is queued before the first one is waited for: one per xGMI link
        ok(run.ctx[g], rc_table_replicate_async(run.ctx[g], run.ctx[0]));
    for (int g = 1; g < run.gpus; ++g) {
        uint64_t dg = 0;
        ok(run.ctx[g], rc_sync(run.ctx[g]) || rc_table_digest(run.ctx[g], &dg));
        if (dg != d0) die("rcorrector: the k-mer table replica on GPU %d differs from the original\n", g);
    }
}

// -write-dump, and -histo: the spectrum of the count (without -c: singletons included; with -c: of the dump's entries)
static void write_table_outputs(Run &run, const Options &o)
{
    if (o.write_dump) ok(run.ctx[0], rc_table_write_jfdump(run.ctx[0], o.write_dump, nullptr));
    if (!o.histo) return;
    std::vector<uint64_t> freq((size_t)o.histo_max + 1);
    ok(run.ctx[0], rc_table_spectrum(run.ctx[0], o.dump ? 0 : 1, freq.data(), (uint32_t)o.histo_max, nullptr));
    if (!write_histo(o.histo, freq)) die("rcorrector: could not write %s\n", o.histo);
}

// GetBadQuality, main.cpp:88-128: first <= 1M records of the primary files, in order
static void bad_quality(Run &run)
{
    if (!run.files.empty() && run.files[0].fastq) {
        std::vector<int32_t> fh(300, 0), lh(300, 0);
        int total = 0;
        if (run.resident) {  // the same records, from the blocks the counting pass kept (primary files, in order)
            for (const auto &R : run.kept) {
                if (total >= 1000000) break;
                quality_histograms(R->a, R->lpr_a, (size_t)(1000000 - total), fh, lh, &total);
            }
        } else {
            for (size_t fi = 0; fi < run.files.size() && total < 1000000; ++fi) {
                Source s;
                s.open(run.files[fi].path);
                Block b;
                const int lpr = run.files[fi].fastq ? 4 : 2;
                while (total < 1000000) {
                    take_records(s, std::min<size_t>((size_t)(1000000 - total), (size_t)1 << 18), lpr, b);
                    if (b.records == 0) break;
                    quality_histograms(b, lpr, b.records, fh, lh, &total);
                }
                s.close();
            }
        }
        run.bad_q = rc_bad_quality_from_hist(fh.data(), lh.data(), total);
    }
    fprintf(stderr, "Bad quality threshold is '%c'\n", run.bad_q);
}

static void close_files(Run &run)
{
    for_each_input(run, [](ReadFile &f) {
        if (f.out && f.out_gz && !f.wrote) {  // an empty .gz is still one (empty) gzip member
            OutBuf none, z;
            gzip_member(none, z);
            std::vector<OutBuf> one(1);
            one[0].swap(z);
            emit_slices(f, one);
        }
        if (f.out && f.out != stdout && f.preallocated && ftruncate(fileno(f.out), f.out_off) != 0)
            die("ERROR: could not set the length of the output of %s\n", f.path.c_str());
        if (f.out && f.out != stdout) fclose(f.out);
        f.src.close();
    });
}

static void timing_lines(const Startup &s, const Run &run)
{
    if (!g_timing) return;
    fprintf(stderr, "[rc timing] start-up (dump load, table build, ERROR_RATE, bad quality) %.2f s; correction loop (read, correct, write) %.2f s; %d host threads\n",
            s.t_setup - s.t_start, s.t_loop_end - s.t_setup, g_threads);
    fprintf(stderr, "[rc timing] stage totals: read+index %.2f s (reader thread); pack %.2f s + correct_batch %.2f s + format %.2f s (sum over %d worker threads); write %.2f s (writer thread)\n",
            g_t_read, g_t_pack, g_t_gpu, g_t_format, run.nworkers, g_t_write);
    fprintf(stderr, "[rc timing] inside read+index (all files, thread-seconds): pread %.2f s, newline scan %.2f s, line index %.2f s\n", g_t_fill, g_t_nl, g_t_idx);
    fprintf(stderr, "[rc timing] blocked: reader %.2f s (no free slot), workers %.2f s (no batch), writer %.2f s (next batch not done)\n", g_w_reader, g_w_worker, g_w_writer);
}

// RC_TEARDOWN (dev): where the time between _exit and the parent's wait goes
static void teardown_report(Run &run)
{
    run.pool.clear();
    run.warm_jobs.clear();
    run.order.clear();
    run.q.clear();
    stamp("teardown: job buffers unregistered and freed");
    for (rc_ctx *c : run.ctx) rc_destroy(c);
    stamp("teardown: contexts destroyed");
    if (atoi(getenv("RC_TEARDOWN")) < 2) return;
    // ... and what is left once the helper threads, the heap and the HIP runtime are gone too
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
        for (size_t i = 0; i < maps.size() && i < 8; ++i) fprintf(stderr, "[rc timing] at exit %8ld kB resident: %s", maps[i].first, maps[i].second.c_str());
    }
    if (FILE *st = fopen("/proc/self/status", "r")) {
        char ln[256];
        while (fgets(ln, sizeof ln, st))
            if (!strncmp(ln, "VmRSS:", 6) || !strncmp(ln, "RssAnon:", 8) || !strncmp(ln, "RssFile:", 8) || !strncmp(ln, "RssShmem:", 9) || !strncmp(ln, "Threads:", 8) || !strncmp(ln, "VmPTE:", 6))
                fprintf(stderr, "[rc timing] at exit %s", ln);
        fclose(st);
    }
}

int main(int argc, char **argv)
{
    g_timing = getenv("RC_TIMING") != nullptr;
    stamp("main() entered");
    Options opt;
    if (!parse_options(argc, argv, opt)) return 0;
    // batches recycle buffers of hundreds of MB: keep freed memory in the heap instead of handing it
    // back to the kernel and faulting it in again page by page (with dozens of threads every
    // mmap/munmap/page fault also serialises on the process's memory-map lock)
    mallopt(M_MMAP_THRESHOLD, 1 << 30);
    mallopt(M_TRIM_THRESHOLD, -1);

    Run run;
    Startup s;
    apply_options(opt, run);
    open_inputs(opt, run);
    start_contexts(s, run, opt);
    size_inputs(s, run, opt);
    start_reader_ahead(s, run, opt);
    join_contexts(s, run);
    decide_one_pass(s, run, opt);
    // While the table loads: the batch buffers of the pipeline -- text blocks, page-locked arenas, output slices --
    // are allocated, sized from the head of the first input, touched and registered with the GPU runtime here, so
    // that the first batches do not pay for a few GB of page faults and hipHostRegister calls one after the other
    std::thread warm([&]() { warm_buffers(run, s.head); });
    const int64_t stored = load_or_count(s, run, opt);
    if (run.gpus > 1) replicate_table(run);
    write_table_outputs(run, opt);
    fprintf(stderr, "Stored %d kmers\n", (int)stored);
    double rate = 0.01;
    ok(run.ctx[0], rc_estimate_error_rate(run.ctx[0], opt.wk, &rate));
    fprintf(stderr, "Weak kmer threshold rate: %lf (estimated from %.3lf/1 of the chosen kmers)\n", rate, opt.wk);
    stamp("ERROR_RATE known");
    bad_quality(run);
    stamp("ERROR_RATE and bad quality known");
    for (rc_ctx *c : run.ctx) ok(c, rc_set_run_params(c, rate, run.bad_q));
    s.t_setup = now_s();
    stamp("start-up done");
    outputs_begin(run, opt);

    // pipeline: reader (this thread) -> `inflight` workers per GPU -> writer thread (input order)
    warm.join();
    stamp("batch buffers ready");
    run_pipeline(run);
    s.t_loop_end = now_s();
    close_files(run);
    // (the contexts are not torn down: the process ends here, and releasing gigabytes of device and
    // host memory piece by piece costs more than everything else after the last write)
    timing_lines(s, run);
    fprintf(stderr, "Processed %llu reads\n\tCorrected %llu bases.\n", (unsigned long long)run.total_reads, (unsigned long long)run.total_cor);
    outputs_finish(run, opt);
    stamp("outputs closed, leaving");
    if (getenv("RC_TEARDOWN")) teardown_report(run);
    fflush(NULL);
    _exit(0);  // every output is closed: skip unmapping gigabytes of buffers one by one
}
