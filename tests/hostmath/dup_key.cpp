// dup_key -- the duplicate census's keys (rcorrector_amd/csrc/rc_dups.h) on the host.
//   dup_key              self-test: the keys are distinct exactly where the strings are.  Every length 0..70, 255, 256, 257,
//                        1023 (each string in a buffer of exactly its length: a read past it is the sanitizers' to find); two
//                        16-byte chunks swapped; the first / last byte changed; a string against itself with A appended; N
//                        against n against A; pairs against swapped pairs; every split of one 40-byte string into two mates;
//                        1 M seeded random reads of 20..160 bases, no two keys equal -- in either 64-bit lane on its own.
//                        Prints "ok <cases>" or the first failure.
//   dup_key keys MODE    the reads on stdin, one per line (an empty line is an empty read), as rc_read_keys_device keys them:
//                        MODE 0 a unit per read, 1 read r of the first half with read r of the second, 2 reads 2u and 2u + 1.
//                        Prints one line of two 16-digit hex words per unit.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rc_dups.h"

struct Key {
    uint64_t w[2];
    bool operator==(const Key &o) const { return w[0] == o.w[0] && w[1] == o.w[1]; }
};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static std::string random_read(size_t len)
{
    std::string s(len, 'A');
    for (size_t i = 0; i < len; ++i) s[i] = "ACGT"[rnd() & 3];
    return s;
}

// (from a heap block of exactly the string's bytes)
static Key key_of(const std::string &s)
{
    std::vector<uint8_t> exact(s.begin(), s.end());
    Key k;
    rc_dup_read_key(exact.data(), (uint32_t)exact.size(), k.w);
    return k;
}

static Key key_of(const std::string &a, const std::string &b)
{
    std::vector<uint8_t> ea(a.begin(), a.end()), eb(b.begin(), b.end());
    Key k;
    rc_dup_pair_key(ea.data(), (uint32_t)ea.size(), eb.data(), (uint32_t)eb.size(), k.w);
    return k;
}

static long cases = 0;
static bool fail(const char *what, size_t len)
{
    printf("fails: %s (length %zu)\n", what, len);
    return false;
}
// two different strings: both lanes must tell them apart
static bool apart(const Key &x, const Key &y, const char *what, size_t len)
{
    ++cases;
    return (x.w[0] != y.w[0] && x.w[1] != y.w[1]) || fail(what, len);
}
static bool same(const Key &x, const Key &y, const char *what, size_t len)
{
    ++cases;
    return x == y || fail(what, len);
}

static bool self_test()
{
    std::vector<size_t> lens;
    for (size_t l = 0; l <= 70; ++l) lens.push_back(l);
    for (size_t l : {255, 256, 257, 1023}) lens.push_back(l);
    std::vector<std::string> strs;
    std::vector<Key> keys;
    for (size_t L : lens) {
        const std::string s = random_read(L);
        const Key k = key_of(s);
        if (!same(k, key_of(std::string(s)), "a copy of the string has another key", L)) return false;
        for (size_t i = 0; i < strs.size(); ++i)
            if (!apart(k, keys[i], "two strings of different length share a key", L)) return false;
        // a prefix of the same letters: the length alone tells them apart from the bytes they share
        if (L > 0 && !apart(k, key_of(s.substr(0, L - 1)), "a string and its prefix share a key", L)) return false;
        if (!apart(k, key_of(s + "A"), "a string and itself with A appended share a key", L)) return false;
        if (!apart(key_of(std::string(L, 'A')), key_of(std::string(L + 1, 'A')), "A^L and A^(L+1) share a key", L)) return false;
        if (L > 0) {
            std::string t = s;
            t[L - 1] = t[L - 1] == 'A' ? 'C' : 'A';
            if (!apart(k, key_of(t), "the last byte changed, the key did not", L)) return false;
            t = s;
            t[0] = t[0] == 'A' ? 'C' : 'A';
            if (!apart(k, key_of(t), "the first byte changed, the key did not", L)) return false;
            for (size_t p : {(size_t)0, L / 2, L - 1}) {
                std::string a = s, n = s, N = s;
                a[p] = 'A';
                n[p] = 'n';
                N[p] = 'N';
                if (!apart(key_of(a), key_of(n), "A and n share a key", L) || !apart(key_of(a), key_of(N), "A and N share a key", L) ||
                    !apart(key_of(n), key_of(N), "n and N share a key", L))
                    return false;
            }
        }
        // two 16-byte chunks swapped, every pair of whole chunks
        for (size_t c1 = 0; 16 * (c1 + 1) <= L && c1 < 5; ++c1)
            for (size_t c2 = c1 + 1; 16 * (c2 + 1) <= L && c2 < 6; ++c2) {
                std::string t = s;
                std::swap_ranges(t.begin() + 16 * c1, t.begin() + 16 * c1 + 16, t.begin() + 16 * c2);
                if (t == s) continue;
                if (!apart(k, key_of(t), "two 16-byte chunks swapped, the key did not change", L)) return false;
            }
        strs.push_back(s);
        keys.push_back(k);
    }
    // pairs
    for (size_t i = 0; i + 1 < strs.size(); ++i) {
        const std::string &a = strs[i], &b = strs[i + 1];
        if (!apart(key_of(a, b), key_of(b, a), "(a, b) and (b, a) share a key", a.size())) return false;
        if (!same(key_of(a, b), key_of(std::string(a), std::string(b)), "a copy of the pair has another key", a.size())) return false;
        if (!apart(key_of(a, b), key_of(a + b), "a pair and its concatenation as one read share a key", a.size())) return false;
        if (!apart(key_of(a, a), key_of(a), "(a, a) and a share a key", a.size())) return false;
    }
    {
        const std::string s = random_read(40);
        std::vector<Key> ks;
        for (size_t cut = 0; cut <= 40; ++cut) ks.push_back(key_of(s.substr(0, cut), s.substr(cut)));
        for (size_t i = 0; i < ks.size(); ++i)
            for (size_t j = i + 1; j < ks.size(); ++j)
                if (!apart(ks[i], ks[j], "two splits of one string into mates share a key", i)) return false;
        const std::string h(40, 'A');  // (the same with nothing but the split to go by)
        ks.clear();
        for (size_t cut = 0; cut <= 40; ++cut) ks.push_back(key_of(h.substr(0, cut), h.substr(cut)));
        for (size_t i = 0; i < ks.size(); ++i)
            for (size_t j = i + 1; j < ks.size(); ++j)
                if (!apart(ks[i], ks[j], "two splits of A^40 into mates share a key", i)) return false;
    }
    // 1 M random reads: no two keys equal, in either lane (equal strings, should the generator make any, excepted)
    {
        const size_t n = 1000000;
        std::vector<std::string> rs(n);
        std::vector<std::pair<uint64_t, uint32_t>> l0(n), l1(n);
        for (size_t i = 0; i < n; ++i) {
            rs[i] = random_read(20 + (size_t)(rnd() % 141));
            Key k;
            rc_dup_read_key(reinterpret_cast<const uint8_t *>(rs[i].data()), (uint32_t)rs[i].size(), k.w);
            l0[i] = {k.w[0], (uint32_t)i};
            l1[i] = {k.w[1], (uint32_t)i};
        }
        for (auto *l : {&l0, &l1}) {
            std::sort(l->begin(), l->end());
            for (size_t i = 1; i < n; ++i)
                if ((*l)[i].first == (*l)[i - 1].first && rs[(*l)[i].second] != rs[(*l)[i - 1].second]) return fail("two random reads share a 64-bit lane", i);
        }
        cases += (long)n;
    }
    return true;
}

static int print_keys(int mode)
{
    std::vector<std::string> reads;
    std::string cur;
    int ch;
    bool open = false;
    while ((ch = getchar()) != EOF) {
        if (ch == '\n') {
            reads.push_back(cur);
            cur.clear();
            open = false;
        } else {
            cur.push_back((char)ch);
            open = true;
        }
    }
    if (open) reads.push_back(cur);
    const size_t n = reads.size(), units = mode == 0 ? n : n / 2;
    if (mode != 0 && (n & 1)) {
        fprintf(stderr, "dup_key: modes 1 and 2 need an even number of reads\n");
        return 2;
    }
    for (size_t u = 0; u < units; ++u) {
        const Key k = mode == 0 ? key_of(reads[u]) : (mode == 1 ? key_of(reads[u], reads[units + u]) : key_of(reads[2 * u], reads[2 * u + 1]));
        printf("%016llx %016llx\n", (unsigned long long)k.w[0], (unsigned long long)k.w[1]);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "keys")) return print_keys(atoi(argv[2]));
    if (argc != 1) {
        fprintf(stderr, "usage: dup_key | dup_key keys MODE < reads\n");
        return 2;
    }
    if (!self_test()) return 1;
    printf("ok %ld cases\n", cases);
    return 0;
}
