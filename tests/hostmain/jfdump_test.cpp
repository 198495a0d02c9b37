// The k-mer dump's text on the host alone (rcorrector_amd/csrc/rc_jfdump.cpp; no library, no GPU), for tests/test_jfdump_host.py.
//   jfdump_test parse DUMP K P1[,P2...]   read the file, parse it into P1 pieces, then P2, ...; one line per piece count:
//       pieces P accepted A invalid I scan S entries N puts M same B
//     (B: codes, inv_mid and the put list equal those of P1, element for element), then the put list of P1 folded the way
//     Store::Put does -- canonical code -> count, a later entry replacing an earlier one -- as "put CODE COUNT" lines
//   jfdump_test format OUT K N P          N entries (code i = i * 0x9E3779B97F4A7C15 + 12345 under the mask, counts 2, 65535, 65536,
//     2^31 - 1 in turn) formatted in two calls that append to one buffer, written to OUT, parsed back in P pieces: "roundtrip B"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>

#include "rc_common.h"
#include "rc_jfdump.h"

struct parsed {
    std::vector<uint64_t> codes, put_codes;
    std::vector<int8_t> inv_mid;
    std::vector<int32_t> put_counts;
    int64_t accepted = 0;
    size_t n_put = 0, scan = 0;
    rc_dump_cache D;
};

static parsed parse_in(const char *text, size_t n, int k, unsigned pieces)
{
    parsed R;
    std::vector<rc_dump_piece> ps = rc_dump_parse(text, n, k, pieces);
    for (const rc_dump_piece &P : ps) {
        R.put_codes.insert(R.put_codes.end(), P.put_codes.begin(), P.put_codes.end());
        R.put_counts.insert(R.put_counts.end(), P.put_counts.begin(), P.put_counts.end());
    }
    rc_dump_join(ps, &R.D, &R.n_put, &R.accepted);
    for (size_t c = 0; c < R.D.codes.size(); ++c) {
        R.codes.insert(R.codes.end(), R.D.codes[c].begin(), R.D.codes[c].end());
        R.inv_mid.insert(R.inv_mid.end(), R.D.inv_mid[c].begin(), R.D.inv_mid[c].end());
    }
    R.scan = rc_dump_scan_length(R.D);
    return R;
}

static int do_parse(const char *path, int k, const char *list)
{
    rc_dump_text text;
    char err[512];
    if (const int rc = rc_dump_read_file(path, &text, err, sizeof err)) {
        printf("error %d %s\n", rc, err);
        return 1;
    }
    parsed first;
    bool have = false, all_same = true;
    for (const char *s = list; *s;) {
        char *e;
        const unsigned pieces = (unsigned)strtoul(s, &e, 10);
        if (e == s || pieces < 1) return 2;
        s = *e == ',' ? e + 1 : e;
        parsed R = parse_in(text.p, text.n, k, pieces);
        const bool sizes = R.D.n == R.codes.size() && R.n_put == R.put_codes.size() && R.inv_mid.size() == R.codes.size();
        if (!have) first = R;
        const bool same = sizes && R.codes == first.codes && R.inv_mid == first.inv_mid && R.put_codes == first.put_codes && R.put_counts == first.put_counts;
        all_same = all_same && same;
        printf("pieces %u accepted %lld invalid %d scan %zu entries %zu puts %zu same %d\n", pieces, (long long)R.accepted, R.D.load_state_invalid, R.scan,
               R.D.n, R.n_put, same ? 1 : 0);
        have = true;
    }
    std::map<uint64_t, int32_t> table;
    for (size_t i = 0; i < first.put_codes.size(); ++i) table[rc_canonical(first.put_codes[i], k)] = first.put_counts[i];
    for (const auto &kv : table) printf("put %llu %d\n", (unsigned long long)kv.first, kv.second);
    return all_same ? 0 : 3;
}

static int do_format(const char *out_path, int k, size_t n, unsigned pieces)
{
    static const int32_t some[4] = {2, 65535, 65536, 2147483647};
    std::vector<uint64_t> codes(n);
    std::vector<int32_t> counts(n);
    for (size_t i = 0; i < n; ++i) {
        codes[i] = ((uint64_t)i * 0x9E3779B97F4A7C15ull + 12345u) & rc_kmer_mask(k);
        counts[i] = some[i & 3];
    }
    std::vector<char> text;
    rc_dump_format(codes.data(), counts.data(), 0, n / 2, k, &text);
    rc_dump_format(codes.data(), counts.data(), n / 2, n, k, &text);
    FILE *fp = fopen(out_path, "wb");
    if (!fp || fwrite(text.data(), 1, text.size(), fp) != text.size() || fclose(fp) != 0) return 2;
    text.push_back(0);
    const parsed R = parse_in(text.data(), text.size() - 1, k, pieces);
    const bool ok = R.codes == codes && R.put_codes == codes && R.put_counts == counts && R.accepted == (int64_t)n && R.scan == n &&
                    R.D.load_state_invalid == 0;
    printf("roundtrip %d\n", ok ? 1 : 0);
    return ok ? 0 : 3;
}

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "parse")) return do_parse(argv[2], atoi(argv[3]), argv[4]);
    if (argc == 6 && !strcmp(argv[1], "format")) return do_format(argv[2], atoi(argv[3]), (size_t)strtoull(argv[4], nullptr, 10), (unsigned)atoi(argv[5]));
    fprintf(stderr, "usage: jfdump_test parse DUMP K P1[,P2...] | format OUT K N P\n");
    return 2;
}
