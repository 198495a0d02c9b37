// weak_reduce -- rc_weak_reduce (rcorrector_amd/csrc/rc_weak.h: a read's weak windows, bad prefix, bad suffix and uncovered bases
// from its words of the solid / weak bit planes) against a per-base loop over the same bits: random planes of three
// densities, k in {3, 15, 23, 31, 32}, the read lengths at which the word arithmetic changes, the read starting at every bit
// offset 0..63 of a plane word (and a few words further in).  Prints "ok <cases>" or the first difference.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rc_weak.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static bool bit(const std::vector<uint64_t> &p, uint64_t b) { return (p[b >> 6] >> (b & 63)) & 1u; }

static rc_weak_vals brute(const std::vector<uint64_t> &solid, const std::vector<uint64_t> &weak, uint64_t bit0, int L, int k)
{
    rc_weak_vals r = {0, L, L, L};
    std::vector<char> cov((size_t)(L > 0 ? L : 0), 0);
    int first = -1, last = -1;
    for (int i = 0; i + k <= L; ++i) {
        if (bit(weak, bit0 + (uint64_t)i)) ++r.weak;
        if (!bit(solid, bit0 + (uint64_t)i)) continue;
        if (first < 0) first = i;
        last = i;
        for (int d = 0; d < k; ++d) cov[(size_t)(i + d)] = 1;
    }
    if (first >= 0) {
        int c = 0;
        for (char x : cov) c += x;
        r.bad_prefix = first;
        r.bad_suffix = L - (last + k);
        r.uncovered = L - c;
    }
    return r;
}

int main()
{
    const int ks[] = {3, 15, 23, 31, 32};
    long cases = 0;
    for (int density = 0; density < 3; ++density) {
        for (int k : ks) {
            const int lens[] = {0, 1, k - 1, k, k + 1, 63, 64, 65, 127, 128, 129, 1023};
            for (int L : lens) {
                for (int word0 = 0; word0 < 2; ++word0) {
                    for (int o = 0; o < 64; ++o) {
                        const uint64_t bit0 = 64ull * (uint64_t)word0 + (uint64_t)o;
                        // exactly the words the read's L bits touch: a read past them is the sanitizers' to find
                        const size_t nwords = (size_t)((bit0 + (uint64_t)(L > 0 ? L : 1) + 63) / 64);
                        std::vector<uint64_t> solid(nwords), weak(nwords);
                        for (size_t w = 0; w < nwords; ++w) {
                            uint64_t a = rnd(), b = rnd();
                            if (density == 1) {  // sparse: isolated solid windows, gaps in the middle
                                a &= rnd() & rnd() & rnd();
                                b &= rnd() & rnd();
                            } else if (density == 2) {  // dense
                                a |= rnd() | rnd();
                            }
                            solid[w] = a;
                            weak[w] = b & ~a;
                        }
                        const rc_weak_vals got = rc_weak_reduce(solid.data(), weak.data(), bit0, L, k), want = brute(solid, weak, bit0, L, k);
                        ++cases;
                        if (got.weak != want.weak || got.bad_prefix != want.bad_prefix || got.bad_suffix != want.bad_suffix || got.uncovered != want.uncovered) {
                            printf("differs: density %d k %d L %d bit0 %llu: got %d %d %d %d, want %d %d %d %d\n", density, k, L, (unsigned long long)bit0, got.weak,
                                   got.bad_prefix, got.bad_suffix, got.uncovered, want.weak, want.bad_prefix, want.bad_suffix, want.uncovered);
                            return 1;
                        }
                        if (want.bad_prefix != L && !(want.bad_prefix + want.bad_suffix <= want.uncovered && want.uncovered <= L)) {
                            printf("the definitions' own invariant fails: k %d L %d\n", k, L);
                            return 1;
                        }
                    }
                }
            }
        }
    }
    printf("ok %ld cases\n", cases);
    return 0;
}
