// recur_key -- the recurrence census's site keys (rcorrector_amd/csrc/rc_recur.h) on the host.
//   recur_key            self-test of the arithmetic alone: reverse complement is an involution and never a fixed point on
//                        seeded random 29-mers; the key of a window and of its reverse-strand twin are one; the centre and the
//                        from code are complemented with it, 4 stays 4; rc_recur_window packs what a letter-by-letter loop
//                        packs and refuses every byte value outside ACGT in every one of the 29 positions, whatever bytes
//                        29..31 hold.  Prints "ok <cases>" or the first failure.
//   recur_key keys       pairs on stdin, one per line, "before<TAB>after" (equal lengths; an empty line is an empty read):
//                        prints per pair "<changes> <contexted>" and the keys of its contexted changes in position order,
//                        16-digit hex.  Every string is read from a heap block of exactly its bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rc_recur.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static long cases = 0;
static bool check(bool ok, const char *what, long at)
{
    ++cases;
    if (!ok) printf("fails: %s (case %ld)\n", what, at);
    return ok;
}

static uint64_t pack_slow(const std::string &s)
{
    uint64_t w = 0;
    for (char c : s) w = (w << 2) | (uint64_t)(c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3);
    return w;
}

static bool window_of(const std::string &s32, uint64_t *w)  // 32 bytes, the window first
{
    uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < 32; ++i) d[i >> 2] |= (uint32_t)(uint8_t)s32[i] << (8 * (i & 3));
    return rc_recur_window(d, w);
}

static bool self_test()
{
    for (long t = 0; t < 200000; ++t) {
        std::string s(RC_RECUR_WINDOW, 'A');
        for (char &c : s) c = "ACGT"[rnd() & 3];
        const uint64_t w = pack_slow(s), r = rc_recur_revcomp(w);
        if (!check(w <= RC_RECUR_W_MASK && r <= RC_RECUR_W_MASK, "a window of more than 58 bits", t)) return false;
        if (!check(rc_recur_revcomp(r) == w, "reverse complement is no involution", t)) return false;
        if (!check(r != w, "a 29-mer is its own reverse complement", t)) return false;
        // the centre: complemented, and still the centre
        const unsigned cw = (unsigned)(w >> (2 * RC_RECUR_FLANK)) & 3u, cr = (unsigned)(r >> (2 * RC_RECUR_FLANK)) & 3u;
        if (!check(cr == 3u - cw, "the centre is not complemented", t)) return false;
        for (int f = 0; f <= 4; ++f) {
            const uint64_t k = rc_recur_key(w, f), kt = rc_recur_key(r, f == 4 ? 4 : 3 - f);
            if (!check(k == kt, "a change and its reverse-strand twin have two keys", t)) return false;
            if (!check((k >> 3) == (w < r ? w : r), "the smaller window is not the canonical one", t)) return false;
            if (!check((int)(k & 7u) == (w < r ? f : (f == 4 ? 4 : 3 - f)), "the from code of the canonical orientation", t)) return false;
            if (!check((k >> 61) == 0, "a key of more than 61 bits", t)) return false;
        }
        // the SWAR packer against the loop, whatever lies behind the window
        std::string s32 = s + "ACG";
        for (size_t i = RC_RECUR_WINDOW; i < 32; ++i) s32[i] = (char)(rnd() & 0xff);
        uint64_t w2 = 0;
        if (!check(window_of(s32, &w2) && w2 == w, "rc_recur_window packs another word", t)) return false;
    }
    // every byte value in every window position
    std::string base(32, 'A');
    for (size_t i = 0; i < 32; ++i) base[i] = "ACGT"[rnd() & 3];
    for (int p = 0; p < RC_RECUR_WINDOW; ++p)
        for (int v = 0; v < 256; ++v) {
            std::string s = base;
            s[(size_t)p] = (char)v;
            uint64_t w;
            const bool letter = v == 'A' || v == 'C' || v == 'G' || v == 'T';
            const bool ok = window_of(s, &w);
            if (!check(ok == letter, "a byte outside ACGT in the window is not refused (or a letter is)", p * 256 + v)) return false;
            if (letter && !check(w == pack_slow(s.substr(0, RC_RECUR_WINDOW)), "the packed word", p * 256 + v)) return false;
        }
    for (int v = 0; v < 256; ++v)
        if (!check(rc_recur_from((uint32_t)v) == (v == 'A' ? 0 : v == 'C' ? 1 : v == 'G' ? 2 : v == 'T' ? 3 : 4), "the from code", v)) return false;
    return true;
}

static int print_keys()
{
    std::vector<std::string> lines;
    std::string cur;
    int ch;
    bool open = false;
    while ((ch = getchar()) != EOF) {
        if (ch == '\n') {
            lines.push_back(cur);
            cur.clear();
            open = false;
        } else {
            cur.push_back((char)ch);
            open = true;
        }
    }
    if (open) lines.push_back(cur);
    for (const std::string &ln : lines) {
        const size_t tab = ln.find('\t');
        const std::string b = tab == std::string::npos ? std::string() : ln.substr(0, tab), a = tab == std::string::npos ? std::string() : ln.substr(tab + 1);
        if (a.size() != b.size()) {
            fprintf(stderr, "recur_key: the two strings of a pair differ in length\n");
            return 2;
        }
        const std::vector<uint8_t> eb(b.begin(), b.end()), ea(a.begin(), a.end());  // (heap blocks of exactly the strings' bytes)
        unsigned long changes = 0, contexted = 0;
        std::vector<uint64_t> keys;
        for (uint32_t p = 0; p < (uint32_t)ea.size(); ++p) {
            uint64_t key = 0;
            const int st = rc_recur_change_at(eb.data(), ea.data(), (uint32_t)ea.size(), p, &key);
            changes += st != 0;
            if (st == 2) {
                ++contexted;
                keys.push_back(key);
            }
        }
        printf("%lu %lu", changes, contexted);
        for (uint64_t k : keys) printf(" %016llx", (unsigned long long)k);
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "keys")) return print_keys();
    if (argc != 1) {
        fprintf(stderr, "usage: recur_key | recur_key keys < pairs\n");
        return 2;
    }
    if (!self_test()) return 1;
    printf("ok %ld cases\n", cases);
    return 0;
}
