// norm_select.cpp -- the normalisation contract (rcorrector_amd/csrc/rc_norm.h: what k_norm_select runs per unit) as a host
// program.  Prints one line per vector -- the inputs, then what the header makes of them:
//   valid1 median1 valid2 median2 index seed target min_cov max_bin : has depth draw outcome bin
// for the boundary vectors below and 2000 seeded random ones, then "ok <lines>".  tests/test_norm_select_host.py compares
// every line with tests/norm_model.py.
#include <cinttypes>
#include <cstdio>
#include <initializer_list>

#include "rc_norm.h"

static unsigned long long g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

static long g_lines = 0;

static void line(int32_t v1, int32_t m1, int32_t v2, int32_t m2, uint64_t index, uint64_t seed, uint32_t target, uint32_t min_cov, uint32_t max_bin)
{
    uint32_t depth;
    const bool has = rc_norm_unit_depth(v1, m1, v2, m2, &depth);
    const uint32_t r = rc_norm_draw(seed, index);
    printf("%d %d %d %d %" PRIu64 " %" PRIu64 " %u %u %u : %d %u %u %u %u\n", v1, m1, v2, m2, index, seed, target, min_cov, max_bin, (int)has, depth, r,
           rc_norm_outcome(has, depth, r, target, min_cov), rc_norm_bin(depth, max_bin));
    ++g_lines;
}

int main()
{
    const int32_t TOP = 0x7FFFFFFF;
    const uint64_t indices[] = {0, 1, 0xFFFFFFFFull, 1ull << 32, (1ull << 32) + 5, 1ull << 40, 0xFFFFFFFFFFFFFFFEull, 0xFFFFFFFFFFFFFFFFull};
    const uint64_t seeds[] = {0, 1, 0xDEADBEEFCAFEF00Dull};
    // single reads at every boundary depth, for three (target, min_cov) and the two extreme targets
    const uint32_t tm[][2] = {{50, 5}, {50, 0}, {7, 9}, {1, 0}, {1, 1}, {(uint32_t)TOP, 0}, {(uint32_t)TOP, (uint32_t)TOP}, {1000, 0xFFFFFFFFu}};
    for (const auto &p : tm) {
        const uint32_t target = p[0], min_cov = p[1];
        const int64_t ds[] = {0, 1, (int64_t)min_cov - 1, min_cov, target, (int64_t)target + 1, 2 * (int64_t)target, 4 * (int64_t)target, TOP - 1, TOP};
        for (const int64_t d : ds) {
            if (d < 0 || d > TOP) continue;
            for (const uint64_t idx : indices)
                for (const uint64_t seed : seeds) line(100, (int32_t)d, 0, 0, idx, seed, target, min_cov, 255);
        }
    }
    // mates with and without valid windows, all four combinations, a median left in a mate that has none; halves round up
    const int32_t meds[][2] = {{7, 8}, {7, 9}, {0, 0}, {0, 1}, {300, 41}, {TOP, TOP}, {TOP, TOP - 1}, {TOP, 0}, {1, TOP}};
    for (const auto &m : meds)
        for (int va = 0; va < 2; ++va)
            for (int vb = 0; vb < 2; ++vb)
                for (const uint64_t idx : {0ull, (1ull << 32) + 5})
                    line(va ? 3 : 0, m[0], vb ? 1 : 0, m[1], idx, 9, 100, 2, 65535);
    line(-1, 5, -2, 6, 0, 0, 10, 0, 10);  // (a valid count is never negative; were it, it is no valid mate)
    // max_bin on both sides of the depth
    for (const uint32_t max_bin : {1u, 255u, 10000u, 65535u})
        for (const uint32_t d : {0u, 1u, 2u, 254u, 255u, 256u, 9999u, 10000u, 10001u, 65534u, 65535u, 65536u, (uint32_t)TOP})
            line(1, (int32_t)d, 0, 0, 3, 4, 500, 0, max_bin);
    // the draw's threshold from both sides: D = 2 * target keeps exactly the draws below 2^31
    for (uint64_t idx = 0; idx < 64; ++idx) line(9, 40, 9, 40, idx, 12345, 20, 0, 100);
    for (int it = 0; it < 2000; ++it) {
        const uint64_t a = rnd(), b = rnd(), c = rnd();
        const int32_t v1 = a & 1 ? (int32_t)(a >> 8 & 1023) : 0, v2 = a & 2 ? (int32_t)(a >> 20 & 1023) : 0;
        const int shift = (int)(b & 31);  // medians and targets of every magnitude
        const int32_t m1 = (int32_t)((uint32_t)(a >> 32) & (uint32_t)TOP) >> shift, m2 = (int32_t)((uint32_t)(b >> 32) & (uint32_t)TOP) >> (int)(b >> 5 & 31);
        uint32_t target = ((uint32_t)(c >> 32) & (uint32_t)TOP) >> (int)(c & 31);
        if (target == 0) target = 1;
        const uint32_t min_cov = c & 32 ? 0 : (uint32_t)(c >> 8 & 0xFFFF) >> (int)(c >> 24 & 15);
        line(v1, m1, v2, m2, it & 1 ? rnd() : rnd() >> 32, rnd(), target, min_cov, 1 + (uint32_t)(rnd() % 65535));
    }
    printf("ok %ld\n", g_lines);
    return 0;
}
