// rc_options.h -- the command line of the `rcorrector` CLI: everything the arguments and the environment decide before a file
// is opened, parsed once from one flag table, clamped and checked.
//   flags        main.cpp:50-71,165-268     -r/-p/-i/-c/-k/-od/-t/-maxcor/-maxcorK/-wk/-stdout/-verbose
// Not in the reference: -gpus N shards batches over N GPUs (table replicated), -batch N sets the reads per batch, -inflight N
// the batches in flight per GPU, -t the host threads used for packing / formatting, -packed the packed transport, -verbose-iter
// the iterations the -verbose transcript records, -write-dump FILE keeps the k-mer table as jellyfish-dump text, -histo FILE
// [-histo-max] writes the spectrum of the count; the extra outputs (-histo-after, -report, -weak-ends / -weak-min, -depth-tags /
// -depth / -depth-max, -dups / -dups-max, -recurrent / -recurrent-min / -top / -max, -trust-by-pos, -overlap / -overlap-min /
// -overlap-mm) are described where they are written, rc_outputs.h.
#pragma once
#include "rc_pool.h"

struct Input {
    char kind;                // 'r' single-end, 'p' two files of mates, 'i' interleaved mates
    const char *path, *mate;  // mate: -p only
};

struct Options {
    int k = 23, t = 0, max_fix_per_k = 4, gpus = 1, inflight = 2, trace_iter = 64;
    int threads = 1;  // g_threads: -t above 1, or the default (parse_options)
    double wk = 0.95;
    size_t batch_reads = (size_t)1 << 20;
    bool inflight_given = false, to_stdout = false, verbose = false, packed = false;
    const char *od = "./", *dump = nullptr, *write_dump = nullptr;
    uint64_t count_mem = (uint64_t)24 << 30;  // RC_COUNT_MEM_MB: the k-mer counter's sort scratch
    // the extra outputs: a path each (nullptr: not asked for) and their bounds
    const char *histo = nullptr, *histo_after = nullptr, *report = nullptr, *dups = nullptr, *recurrent = nullptr, *trust = nullptr;
    const char *overlap = nullptr, *depth = nullptr;
    bool weak_ends = false, depth_tags = false;
    int weak_min = 1, overlap_min = 30, overlap_mm = 10;
    long histo_max = 10000, depth_max = 10000, dups_max = 10000, recur_min = 5, recur_top = 1000, recur_max = 10000;
    std::vector<Input> inputs;  // in command-line order
};

// Parses, clamps and checks.  false: leave with status 0 (-h, no arguments, an unknown argument -- the reference's main.cpp
// returns 0 there too); a usage error ends the process with status 1 (die).  Touches neither an input file nor the library:
// `rcorrector` answers every usage error without a GPU, before anything is opened or written (-od creates the directory and
// -c FILE is opened and closed while the arguments are read, as in the reference).
bool parse_options(int argc, char **argv, Options &o);
