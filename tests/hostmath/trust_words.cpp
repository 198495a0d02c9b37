// trust_words -- the word extraction of the trust profile's accumulate (rcorrector_amd/csrc/rc_trust.h: a read's window string
// taken 64 windows a word from the 5' end, rc_weak_word, and right-aligned and reversed from the 3' end, rc_trust_word3, plus
// rc_trust_have, rc_trust_rev and rc_trust_nwin) against a bit-by-bit loop: random planes of three densities, nwin = 0 .. 200
// and 1000 .. 1024, the read starting at every bit offset 0 .. 63 of a plane word and of a word further in.  The planes hold
// exactly the words the read's windows lie in, random bits in front of window 0 and behind the last window included: a word
// that lets a neighbour's bit through differs from the loop, a fetch past the read's words is the sanitizers' to catch.
// Prints "ok <cases>" or the first difference.  `trust_words dropmask` runs the same comparison on a right-aligned word that
// takes the 64 bits in front of the read's last window as they lie in the plane, without the cut where the string starts
// inside the word: it must NOT pass (the planes then have one more word in front of the read).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rc_trust.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static bool bit(const std::vector<uint64_t> &p, uint64_t b) { return (p[b >> 6] >> (b & 63)) & 1u; }

// the right-aligned word without its negative-start cut (bit0 + nwin >= 64 (j + 1) here)
static uint64_t word3_dropmask(const uint64_t *plane, uint64_t bit0, uint32_t j, uint32_t nwin)
{
    return rc_trust_rev(rc_weak_word(plane, bit0 + nwin - 64u * (j + 1), 0, 64u));
}

int main(int argc, char **argv)
{
    const bool drop = argc > 1 && !strcmp(argv[1], "dropmask");
    long cases = 0;
    for (int l = 0; l < 64; ++l) {
        const uint64_t x = rnd();
        const uint64_t r = rc_trust_rev(x);
        for (int b = 0; b < 64; ++b)
            if (((r >> b) & 1u) != ((x >> (63 - b)) & 1u)) {
                printf("rev: %016llx -> %016llx, bit %d\n", (unsigned long long)x, (unsigned long long)r, b);
                return 1;
            }
    }
    for (int k = 1; k <= 32; ++k)
        for (int L = -1; L <= 1100; ++L) {
            const uint32_t want = L < k ? 0u : (uint32_t)(L - k + 1) > (uint32_t)RC_TRUST_LEN ? (uint32_t)RC_TRUST_LEN : (uint32_t)(L - k + 1);
            if (rc_trust_nwin(L, k) != want) {
                printf("nwin: L %d k %d: got %u, want %u\n", L, k, rc_trust_nwin(L, k), want);
                return 1;
            }
        }
    for (int density = 0; density < 3; ++density)
        for (uint32_t nwin = 0; nwin <= 1024; nwin = nwin == 200 ? 1000 : nwin + 1)
            for (int in = 0; in < 2; ++in)
                for (uint32_t s = 0; s < 64; ++s) {
                    const uint64_t bit0 = 64ull * (drop ? 1 + 2 * in : 3 * in) + s;
                    std::vector<uint64_t> plane((size_t)(nwin ? (bit0 + nwin + 63) / 64 : 0));
                    for (uint64_t &w : plane) w = density == 0 ? rnd() : density == 1 ? rnd() & rnd() & rnd() : rnd() | rnd() | rnd();
                    ++cases;
                    for (uint32_t j = 0; 64u * j < nwin; ++j) {
                        const uint64_t w5 = rc_weak_word(plane.data(), bit0, j, nwin), have = rc_trust_have(j, nwin);
                        const uint64_t w3 = drop ? word3_dropmask(plane.data(), bit0, j, nwin) : rc_trust_word3(plane.data(), bit0, j, nwin);
                        for (uint32_t l = 0; l < 64; ++l) {
                            const uint32_t p = 64u * j + l;
                            const bool in_read = p < nwin;
                            const bool want5 = in_read && bit(plane, bit0 + p), want3 = in_read && bit(plane, bit0 + (nwin - 1 - p));
                            if (((have >> l) & 1u) != (uint64_t)in_read) {
                                printf("have: nwin %u word %u lane %u\n", nwin, j, l);
                                return 1;
                            }
                            if (((w5 >> l) & 1u) != (uint64_t)want5) {
                                printf("word5: nwin %u bit0 %llu word %u lane %u: got %d\n", nwin, (unsigned long long)bit0, j, l, (int)!want5);
                                return 1;
                            }
                            if (((w3 >> l) & 1u) != (uint64_t)want3) {
                                printf("word3: nwin %u bit0 %llu word %u lane %u: got %d\n", nwin, (unsigned long long)bit0, j, l, (int)!want3);
                                return 1;
                            }
                        }
                    }
                }
    printf("ok %ld\n", cases);
    return 0;
}
