// screen_mask.cpp -- rc_screen.h's mask arithmetic (hits, covered, longest of a read's hit mask) as a host program against a
// brute force that marks every base and scans every window.  Prints "ok <cases>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rc_screen.h"

static int g_cases = 0;

// bit i of the mask = window i; the words are allocated to exactly (nwin + 63) / 64
static void check(const std::vector<uint8_t> &hit, int k, const char *what)
{
    const uint32_t nwin = (uint32_t)hit.size();
    std::vector<uint64_t> words((nwin + 63) / 64, 0);
    for (uint32_t i = 0; i < nwin; ++i)
        if (hit[i]) words[i >> 6] |= 1ull << (i & 63);
    // the definition: a base is covered if it lies in a hit window; a run is consecutive hit windows
    std::vector<uint8_t> base(nwin ? nwin + (uint32_t)k - 1 : 0, 0);
    int32_t hits = 0, longest = 0, run = 0, covered = 0;
    for (uint32_t i = 0; i < nwin; ++i) {
        if (hit[i]) {
            ++hits;
            ++run;
            if (run > longest) longest = run;
            for (int j = 0; j < k; ++j) base[i + (uint32_t)j] = 1;
        } else {
            run = 0;
        }
    }
    for (uint8_t b : base) covered += b;
    const rc_screen_vals v = rc_screen_mask(words.data(), nwin, nwin, k);
    if (v.valid != (int32_t)nwin || v.hits != hits || v.covered != covered || v.longest != longest) {
        printf("FAIL %s: nwin %u k %d: got hits %d covered %d longest %d, want %d %d %d\n", what, nwin, k, v.hits, v.covered, v.longest, hits, covered,
               longest);
        exit(1);
    }
    // the sum the header states, hit by hit
    int64_t sum = 0, prev = -1;
    for (uint32_t i = 0; i < nwin; ++i)
        if (hit[i]) {
            if (prev >= 0) sum += (int64_t)i - prev < k ? (int64_t)i - prev : k;
            prev = i;
        }
    if (prev >= 0) sum += k;
    if (sum != covered) {
        printf("FAIL %s: nwin %u k %d: the sum of min(k, next - i) is %lld, the bases are %d\n", what, nwin, k, (long long)sum, covered);
        exit(1);
    }
    ++g_cases;
}

int main()
{
    const uint32_t sizes[] = {0, 1, 63, 64, 65, 127, 128, 129, 1001};
    const int ks[] = {3, 15, 23, 32};
    for (uint32_t n : sizes)
        for (int k : ks) {
            std::vector<uint8_t> m(n, 0);
            check(m, k, "no hit");
            check(std::vector<uint8_t>(n, 1), k, "all hits");
            for (uint32_t i = 0; i < n; ++i) m[i] = (uint8_t)(i & 1u ? 0 : 1);
            check(m, k, "alternating");
            m.assign(n, 0);
            if (n) m[0] = 1;
            check(m, k, "first window");
            m.assign(n, 0);
            if (n) m[n - 1] = 1;
            check(m, k, "last window");
        }
    for (int k : ks) {
        // two hits k - 1, k and k + 1 windows apart: the intervals overlap by one base, touch, leave one base out
        for (int d = k - 1; d <= k + 1; ++d)
            for (uint32_t p : {0u, 60u}) {
                std::vector<uint8_t> m(200, 0);
                m[p] = m[p + (uint32_t)d] = 1;
                check(m, k, "two hits");
            }
        std::vector<uint8_t> m(200, 0);
        for (uint32_t i = 50; i <= 63; ++i) m[i] = 1;  // a run that ends at bit 63
        m[70] = 1;
        check(m, k, "run to bit 63");
        m.assign(200, 0);
        for (uint32_t i = 64; i < 90; ++i) m[i] = 1;  // one that starts at bit 64
        m[10] = 1;
        check(m, k, "run from bit 64");
        m.assign(200, 0);
        for (uint32_t i = 40; i < 140; ++i) m[i] = 1;  // one that crosses two word boundaries, a shorter one in front
        for (uint32_t i = 0; i < 30; ++i) m[i] = 1;
        check(m, k, "run across");
    }
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    };
    for (int c = 0; c < 200; ++c) {
        const uint32_t n = 1 + (uint32_t)(rnd() % 1001);
        const int k = ks[rnd() % 4];
        std::vector<uint8_t> m(n, 0);
        if (c & 1) {  // runs of random lengths, long ones included
            uint32_t i = 0;
            uint8_t bit = (uint8_t)(rnd() & 1);
            while (i < n) {
                uint32_t len = 1 + (uint32_t)(rnd() % (c % 4 == 1 ? 5 : 90));
                for (; len && i < n; --len) m[i++] = bit;
                bit ^= 1;
            }
        } else {  // independent bits at a density of c / 200
            for (uint32_t i = 0; i < n; ++i) m[i] = (uint8_t)(rnd() % 200 < (uint64_t)c + 1);
        }
        check(m, k, "random");
    }
    printf("ok %d\n", g_cases);
    return 0;
}
