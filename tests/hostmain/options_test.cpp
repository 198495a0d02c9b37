// options_test.cpp -- parse_options (rc_options.cpp) called directly: the clamps it applies and the order and kinds of the
// inputs it keeps.  Without arguments it runs its cases and prints "ok"; with arguments it parses them as its own command line
// and prints what came out (a usage error ends it as it ends `rcorrector`: one line on stderr, status 1).
#include "../../rcorrector_amd/csrc/rc_options.h"

static int g_bad = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("line %d: %s does not hold\n", __LINE__, #cond);       \
            ++g_bad;                                                      \
        }                                                                 \
    } while (0)

static Options parse(std::vector<const char *> args)
{
    args.insert(args.begin(), "rcorrector");
    Options o;
    if (!parse_options((int)args.size(), (char **)args.data(), o)) {
        printf("parse_options does not want to run\n");
        ++g_bad;
    }
    return o;
}

int main(int argc, char **argv)
{
    if (argc > 1) {
        Options o;
        if (!parse_options(argc, argv, o)) return 0;
        printf("k %d gpus %d inflight %d batch %zu threads %d packed %d inputs %zu\n", o.k, o.gpus, o.inflight, o.batch_reads, o.threads, (int)o.packed, o.inputs.size());
        return 0;
    }
    unsetenv("RC_TRANSPORT");
    unsetenv("RC_COUNT_MEM_MB");
    const unsigned hc = std::thread::hardware_concurrency();
    const int default_threads = (int)std::min<unsigned>(hc ? hc : 8, 16);
    {
        Options o = parse({"-k", "25"});  // the defaults
        CHECK(o.k == 25 && o.gpus == 1 && o.inflight == 2 && !o.inflight_given && o.batch_reads == ((size_t)1 << 20) && o.trace_iter == 64);
        CHECK(o.threads == default_threads && !o.packed && !o.verbose && !o.to_stdout && o.max_fix_per_k == 4 && o.wk == 0.95 && !strcmp(o.od, "./"));
        CHECK(o.count_mem == ((uint64_t)24 << 30) && o.inputs.empty() && !o.dump && !o.histo && !o.overlap && o.weak_min == 1);
    }
    CHECK(parse({"-gpus", "0"}).gpus == 1);
    CHECK(parse({"-gpus", "3"}).gpus == 3);
    CHECK(parse({"-inflight", "0"}).inflight == 1 && parse({"-inflight", "0"}).inflight_given);
    CHECK(parse({"-inflight", "99"}).inflight == std::min(8, RC_MAX_SLOTS));
    CHECK(parse({"-inflight", "3"}).inflight == std::min(3, RC_MAX_SLOTS));
    CHECK(parse({"-batch", "7"}).batch_reads == 6);
    CHECK(parse({"-batch", "0"}).batch_reads == 2);
    CHECK(parse({"-batch", "1000000"}).batch_reads == 1000000);
    CHECK(parse({"-verbose", "-batch", "1000000"}).batch_reads == 65536);
    CHECK(parse({"-verbose", "-batch", "100"}).batch_reads == 100);
    CHECK(parse({"-verbose-iter", "0"}).trace_iter == 1);
    CHECK(parse({"-verbose-iter", "7"}).trace_iter == 7);
    CHECK(parse({"-packed"}).packed);
    CHECK(!parse({"-verbose", "-packed"}).packed && !parse({"-packed", "-verbose"}).packed);
    CHECK(parse({"-t", "1"}).threads == default_threads && parse({"-t", "1"}).t == 1);
    CHECK(parse({"-t", "5"}).threads == 5);
    CHECK(parse({"-maxcor", "3", "-maxcorK", "2", "-wk", "0.5", "-stdout"}).max_fix_per_k == 2);
    setenv("RC_TRANSPORT", "packed", 1);
    CHECK(parse({"-k", "23"}).packed && !parse({"-verbose"}).packed);
    setenv("RC_TRANSPORT", "bytes", 1);
    CHECK(!parse({"-k", "23"}).packed && parse({"-packed"}).packed);
    unsetenv("RC_TRANSPORT");
    setenv("RC_COUNT_MEM_MB", "512", 1);
    CHECK(parse({"-k", "23"}).count_mem == ((uint64_t)512 << 20));
    unsetenv("RC_COUNT_MEM_MB");
    {
        Options o = parse({"-r", "a.fq", "-k", "31", "-p", "b_1.fq", "b_2.fq", "-i", "c.fa", "-histo", "h", "-r", "d.fq", "-p", "e_1.fq", "e_2.fq"});
        CHECK(o.inputs.size() == 5 && o.k == 31 && !strcmp(o.histo, "h"));
        const char *kinds = "rpirp", *paths[] = {"a.fq", "b_1.fq", "c.fa", "d.fq", "e_1.fq"}, *mates[] = {nullptr, "b_2.fq", nullptr, nullptr, "e_2.fq"};
        for (size_t i = 0; i < o.inputs.size() && i < 5; ++i) {
            CHECK(o.inputs[i].kind == kinds[i] && !strcmp(o.inputs[i].path, paths[i]));
            CHECK(mates[i] ? o.inputs[i].mate && !strcmp(o.inputs[i].mate, mates[i]) : !o.inputs[i].mate);
        }
    }
    {
        Options o;
        const char *none[] = {"rcorrector"}, *help[] = {"rcorrector", "-k", "23", "-h"}, *unknown[] = {"rcorrector", "-nope"};
        CHECK(!parse_options(1, (char **)none, o) && !parse_options(4, (char **)help, o) && !parse_options(2, (char **)unknown, o));
    }
    if (g_bad) printf("%d checks failed\n", g_bad);
    else printf("ok\n");
    return g_bad ? 1 : 0;
}
