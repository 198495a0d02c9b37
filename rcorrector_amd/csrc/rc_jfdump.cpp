// rc_jfdump.cpp -- the text of a `jellyfish dump`, host only (rc_jfdump.h).
#include "rc_jfdump.h"

#include <fcntl.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <thread>

#include "rc_common.h"

unsigned rc_host_threads(size_t bytes, size_t threshold)
{
    if (bytes < threshold) return 1;
    const unsigned T = std::thread::hardware_concurrency();
    return T == 0 ? 4 : (T > 32 ? 32 : T);
}

// f(t) for t in [0, T), each on a thread of its own where there are several
template <class F>
static void on_threads(unsigned T, F f)
{
    if (T == 1) return f(0u);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; ++t) th.emplace_back(f, t);
    for (auto &x : th) x.join();
}

static int read_fd(int fd, const char *path, rc_dump_text *out, char *err, size_t err_len)
{
    const off_t sz = lseek(fd, 0, SEEK_END);
    if (sz < 0 || (unsigned long long)sz >= (unsigned long long)SIZE_MAX) {
        snprintf(err, err_len, "short read on %s", path);
        return RC_ERR_IO;
    }
    const size_t n = (size_t)sz;
    char *p = (char *)malloc(n + 1);  // uninitialised: the readers fill it
    if (!p) {
        snprintf(err, err_len, "out of memory reading %s (%ld bytes)", path, (long)sz);
        return RC_ERR_NOMEM;
    }
    free(out->p);
    out->p = p;
    out->n = n;
    const unsigned T = rc_host_threads(n, (size_t)8 << 20);
    std::vector<char> ok(T, 1);
    on_threads(T, [&](unsigned t) {
        size_t at = n * t / T;
        const size_t hi = n * (t + 1) / T;
        while (at < hi) {
            const ssize_t got = pread(fd, p + at, hi - at, (off_t)at);
            if (got <= 0) {
                ok[t] = 0;
                return;
            }
            at += (size_t)got;
        }
    });
    p[n] = 0;
    if (memchr(ok.data(), 0, T)) {
        snprintf(err, err_len, "short read on %s", path);
        return RC_ERR_IO;
    }
    return RC_OK;
}

int rc_dump_read_file(const char *path, rc_dump_text *out, char *err, size_t err_len)
{
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) {
        snprintf(err, err_len, "Could not open file %s", path);
        return RC_ERR_IO;
    }
    const int rc = read_fd(fd, path, out, err, err_len);
    close(fd);
    return rc;
}

static inline bool is_ws(char ch) { return ch == ' ' || ch == '\n' || ch == '\t' || ch == '\r' || ch == '\f' || ch == '\v'; }

std::vector<size_t> rc_dump_cut(const char *text, size_t n, unsigned pieces)
{
    std::vector<size_t> cut(pieces + 1, n);
    cut[0] = 0;
    for (unsigned t = 1; t < pieces; ++t) {
        size_t pos = n * t / pieces;
        if (pos < cut[t - 1]) pos = cut[t - 1];
        while (pos < n && !(text[pos] == '>' && (pos == 0 || is_ws(text[pos - 1])))) ++pos;
        cut[t] = pos;
    }
    return cut;
}

// atoi() of the decimal digits in [q, end) as glibc implements it, (int)strtol(): the long value saturates at LONG_MAX /
// LONG_MIN and the conversion to int keeps its low 32 bits (main.cpp:297 applies it to the count token).  *stop: the first
// character that is no digit
static inline int atoi_digits(const char *q, const char *end, bool neg, const char **stop)
{
    unsigned long long v = 0;
    bool ovf = false;
    for (; q < end && (unsigned)(*q - '0') <= 9u; ++q) {
        const unsigned d = (unsigned)(*q - '0');
        if (v > (0x7fffffffffffffffULL - d) / 10) ovf = true;
        if (!ovf) v = v * 10 + d;
    }
    *stop = q;
    long long lv;
    if (ovf)
        lv = neg ? (long long)0x8000000000000000ULL : 0x7fffffffffffffffLL;
    else
        lv = neg ? -(long long)v : (long long)v;
    return (int)(uint32_t)(uint64_t)lv;
}

void rc_dump_parse_piece(const char *text, size_t lo, size_t hi, int k, rc_dump_piece *piece)
{
    rc_dump_piece &P = *piece;
    const uint64_t mask = rc_kmer_mask(k);
    int8_t base_code[256];
    memset(base_code, -1, sizeof base_code);
    base_code[(unsigned char)'A'] = 0;
    base_code[(unsigned char)'C'] = 1;
    base_code[(unsigned char)'G'] = 2;
    base_code[(unsigned char)'T'] = 3;
    const char *p = text + lo, *end = text + hi;
    const size_t guess = (size_t)(end - p) / (size_t)(k + 4) + 16;
    P.codes.reserve(P.codes.size() + guess);
    P.inv_mid.reserve(P.inv_mid.size() + guess);
    P.put_codes.reserve(P.put_codes.size() + guess);
    P.put_counts.reserve(P.put_counts.size() + guess);
    while (true) {
        // fast path for the layout `jellyfish dump` writes: ">DIGITS\nKMER\n" with exactly k
        // letters out of ACGT -- everything else goes through the general tokeniser below,
        // which is what defines the result
        if (end - p > 1 && *p == '>' && (unsigned)(p[1] - '0') <= 9u) {
            const char *q;
            const int cnt = atoi_digits(p + 1, end, false, &q);
            if (end - q > 1 + k && *q == '\n' && q[1 + k] == '\n') {
                const unsigned char *s2 = reinterpret_cast<const unsigned char *>(q + 1);
                uint64_t code = 0;
                int bad = 0;
                for (int i = 0; i < k; ++i) {
                    const int b = base_code[s2[i]];
                    bad |= b;
                    code = (code << 2) | (uint64_t)(b & 3);
                }
                if (bad >= 0) {  // all four codes are non-negative: no other letter in the k-mer
                    p = q + 2 + k;
                    P.codes.push_back(code);
                    P.inv_mid.push_back(0);
                    if (cnt <= 1) continue;
                    P.last_state_invalid = 0;
                    ++P.accepted;
                    P.put_codes.push_back(code);
                    P.put_counts.push_back((int32_t)cnt);
                    continue;
                }
            }
        }
        while (p < end && is_ws(*p)) ++p;
        if (p >= end) break;
        const char *t0 = p;
        while (p < end && !is_ws(*p)) ++p;
        const char *q = t0 + 1;  // atoi(&token[1])
        const bool neg = q < p && *q == '-';
        if (q < p && (*q == '-' || *q == '+')) ++q;
        const int cnt = atoi_digits(q, p, neg, &q);
        while (p < end && is_ws(*p)) ++p;
        const char *k0 = p;
        while (p < end && !is_ws(*p)) ++p;
        uint64_t code = 0;
        int inv = -1;
        for (q = k0; q < p; ++q) {
            const int b = base_code[(unsigned char)*q];
            if (inv != -1) ++inv;
            code = ((code << 2) & mask) | (uint64_t)(b & 3);
            if (b == -1) inv = 0;
            if (inv >= k) inv = -1;
        }
        P.codes.push_back(code);
        P.inv_mid.push_back(inv > 0 ? 1 : 0);
        if (cnt <= 1) continue;
        P.last_state_invalid = (inv != -1);
        ++P.accepted;
        if (inv == -1) {  // Store::Put ignores invalid k-mers, Store.h:53-54
            P.put_codes.push_back(code);
            P.put_counts.push_back((int32_t)cnt);
        }
    }
}

std::vector<rc_dump_piece> rc_dump_parse(const char *text, size_t n, int k, unsigned pieces)
{
    const std::vector<size_t> cut = rc_dump_cut(text, n, pieces);
    std::vector<rc_dump_piece> out(pieces);
    on_threads(pieces, [&](unsigned t) { rc_dump_parse_piece(text, cut[t], cut[t + 1], k, &out[t]); });
    return out;
}

void rc_dump_join(std::vector<rc_dump_piece> &pieces, rc_dump_cache *D, size_t *n_put, int64_t *accepted)
{
    *D = rc_dump_cache();
    *n_put = 0;
    *accepted = 0;
    for (rc_dump_piece &P : pieces) {
        D->n += P.codes.size();
        *n_put += P.put_codes.size();
        *accepted += P.accepted;
        if (P.last_state_invalid >= 0) D->load_state_invalid = P.last_state_invalid;
        D->codes.emplace_back(std::move(P.codes));
        D->inv_mid.emplace_back(std::move(P.inv_mid));
    }
}

size_t rc_dump_scan_length(const rc_dump_cache &D)
{
    size_t n = 0;
    if (D.load_state_invalid) return 0;
    for (const std::vector<int8_t> &inv : D.inv_mid) {
        const void *hit = inv.empty() ? nullptr : memchr(inv.data(), 1, inv.size());
        if (hit) return n + (size_t)((const int8_t *)hit - inv.data());
        n += inv.size();
    }
    return n;
}

void rc_dump_format(const uint64_t *codes, const int32_t *counts, size_t lo, size_t hi, int k, std::vector<char> *out)
{
    const size_t at = out->size();
    out->resize(at + (hi - lo) * (size_t)(k + 14));  // '>', at most 10 digits, two newlines, k letters
    char *w = out->data() + at;
    for (size_t i = lo; i < hi; ++i) {
        *w++ = '>';
        char tmp[12];
        int nd = 0;
        uint32_t v = (uint32_t)counts[i];
        do {
            tmp[nd++] = (char)('0' + v % 10);
            v /= 10;
        } while (v);
        while (nd) *w++ = tmp[--nd];
        *w++ = '\n';
        for (int j = k - 1; j >= 0; --j) *w++ = "ACGT"[(codes[i] >> (2 * j)) & 3];
        *w++ = '\n';
    }
    out->resize((size_t)(w - out->data()));
}
