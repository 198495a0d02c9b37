// depth_select.cpp -- the selection of the per-read k-mer depth (rcorrector_amd/csrc/rc_depth.h: rc_depth_select, what
// k_read_depth runs per read) as a host program against a sort.  The counts are laid out as the kernel's lanes hold them -- an
// array of 64 * ceil(windows / 64) slots, RC_DEPTH_INVALID in the slots of invalid windows and behind the read's last window
// -- and count_eq is a loop over exactly those slots (allocated to that size: a read past them is an address error).
// Prints "ok <cases>" or the first case that differs and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rc_depth.h"

static unsigned long long g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 16);
}

static long g_cases = 0;

// counts: the valid windows' counts in read order; every `gap`-th window of the read is an invalid one put in between (0: none)
static void check(const std::vector<uint32_t> &counts, unsigned gap, const char *what)
{
    std::vector<uint32_t> win;
    for (size_t i = 0; i < counts.size(); ++i) {
        if (gap && i % gap == 0) win.push_back(RC_DEPTH_INVALID);
        win.push_back(counts[i]);
    }
    if (gap) win.push_back(RC_DEPTH_INVALID);
    const size_t slots = (win.size() + 63) / 64 * 64;
    uint32_t *lane = (uint32_t *)malloc(slots ? slots * 4 : 4);
    for (size_t i = 0; i < slots; ++i) lane[i] = i < win.size() ? win[i] : RC_DEPTH_INVALID;
    uint32_t n = 0, orv = 0;
    for (size_t i = 0; i < slots; ++i)
        if (lane[i] != RC_DEPTH_INVALID) {
            ++n;
            orv |= lane[i];
        }
    const rc_depth_vals got = rc_depth_select(n, orv, [&](int shift, uint32_t key) {
        uint32_t c = 0;
        for (size_t i = 0; i < slots; ++i) c += (lane[i] >> shift) == key;
        return c;
    });
    free(lane);
    std::vector<uint32_t> c = counts;
    std::sort(c.begin(), c.end());
    rc_depth_vals want = {(int32_t)c.size(), 0, 0, 0};
    if (!c.empty()) {
        const size_t m = c.size();
        want.q1 = (int32_t)c[(m - 1) / 4];
        want.median = (int32_t)c[(m - 1) / 2];
        want.q3 = (int32_t)c[3 * (m - 1) / 4];
    }
    ++g_cases;
    if (got.valid != want.valid || got.q1 != want.q1 || got.median != want.median || got.q3 != want.q3 || got.q1 > got.median || got.median > got.q3) {
        printf("%s, n = %zu, gap %u: got %d %d %d %d, want %d %d %d %d\n", what, counts.size(), gap, got.valid, got.q1, got.median, got.q3, want.valid,
               want.q1, want.median, want.q3);
        exit(1);
    }
}

int main()
{
    const uint32_t TOP = (1u << 27) - 1u;
    std::vector<size_t> sizes;
    for (size_t n = 0; n <= 9; ++n) sizes.push_back(n);
    for (size_t n : {63, 64, 65, 127, 128, 129, 1001}) sizes.push_back(n);
    for (size_t n : sizes)
        for (unsigned gap : {0u, 3u}) {
            std::vector<uint32_t> c(n);
            for (uint32_t v : {0u, 1u, 7505u, TOP}) {  // all counts equal
                std::fill(c.begin(), c.end(), v);
                check(c, gap, "all equal");
            }
            for (size_t i = 0; i < n; ++i) c[i] = rnd() & 1u ? TOP : 0u;  // the two extremes only
            check(c, gap, "0 / 2^27 - 1");
            for (size_t i = 0; i < n; ++i) c[i] = i & 1u ? TOP : 0u;
            check(c, gap, "alternating");
            for (size_t i = 0; i < n; ++i) c[i] = (uint32_t)(3 * i + 1);  // strictly increasing
            check(c, gap, "increasing");
            for (size_t i = 0; i < n; ++i) c[i] = (uint32_t)(TOP - 5 * i);  // strictly decreasing
            check(c, gap, "decreasing");
            for (size_t i = 0; i < n; ++i) c[i] = rnd() & TOP;  // no ties to speak of
            check(c, gap, "random");
        }
    for (int it = 0; it < 200; ++it) {  // heavy ties: a handful of distinct values, some of them neighbours, some far apart
        const size_t n = rnd() % 1002;
        const uint32_t distinct = 1 + rnd() % 6;
        uint32_t vals[6];
        for (uint32_t d = 0; d < distinct; ++d) vals[d] = rnd() % 3 == 0 ? rnd() & TOP : rnd() % 8;
        std::vector<uint32_t> c(n);
        for (size_t i = 0; i < n; ++i) c[i] = vals[rnd() % distinct];
        check(c, it % 3 == 0 ? 1 + rnd() % 7 : 0, "ties");
    }
    uint32_t r[3];  // the rank arithmetic itself, where the three ranks first differ
    const uint32_t want[10][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 1, 1}, {0, 1, 2}, {1, 2, 3}, {1, 2, 3}, {1, 3, 4}, {1, 3, 5}, {2, 4, 6}};
    for (uint32_t n = 1; n <= 9; ++n) {
        rc_depth_ranks(n, r);
        ++g_cases;
        if (r[0] != want[n][0] || r[1] != want[n][1] || r[2] != want[n][2]) {
            printf("ranks of n = %u: got %u %u %u\n", n, r[0], r[1], r[2]);
            return 1;
        }
    }
    printf("ok %ld\n", g_cases);
    return 0;
}
