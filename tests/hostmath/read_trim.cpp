// The trimming contract (rcorrector_amd/csrc/rc_trim.h) as a host program that runs the kernel's lanes one after the other: stage
// 16 bytes a lane, reverse and complement mate 2 a word a lane, an offset a lane for the pair scan and for the adapter scan, 16
// quality bytes a lane with the suffix scan over the lanes done as the shuffles do it.  Reads units from a text file -- per mate
// two lines, '=' and the bases, then '=' and the quality bytes or '-' for none -- and prints one line per read, "keep_len
// cut_qual cut_adapter cut_pair", and one per unit, "unit <kept> <overlapping>"; tests/test_read_trim_host.py compares them with
// tests/trim_model.py.
//   read_trim FILE NW MATES QUAL_MIN QUAL_BASE ADAPTER1 ADAPTER2 ADAPTER_MIN ADAPTER_MM PAIR_OVERLAP PAIR_MIN PAIR_MM MIN_LEN
//   (NW: words a mate, 8 or 32, as k_read_trim's instances; an adapter of no bases is written '-')
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "rc_trim.h"

// bytes [16 c, 16 c + 16) of s as four dwords, bytes at or behind len as 0
static void load16(const std::string &s, int len, int c, uint32_t (&w)[4])
{
    w[0] = w[1] = w[2] = w[3] = 0;
    for (int j = 0; j < 16; ++j)
        if (16 * c + j < len) w[j >> 2] |= (uint32_t)(uint8_t)s[16 * c + j] << (8 * (j & 3));
}

static void stage(const std::string &s, int len, int nw, uint64_t *code, uint64_t *val)
{
    std::vector<uint32_t> c32(2 * nw), v32(2 * nw);
    for (int c = 0; c < 2 * nw; ++c) {
        uint32_t w[4], code16, val16;
        load16(s, len, c, w);
        rc_ov_pack16(w, code16, val16);
        c32[c ^ 1] = code16;  // (chunk 2 w is the high half of word w)
        v32[c ^ 1] = val16;
    }
    for (int w = 0; w < nw; ++w) {
        code[w] = ((uint64_t)c32[2 * w + 1] << 32) | c32[2 * w];
        val[w] = ((uint64_t)v32[2 * w + 1] << 32) | v32[2 * w];
    }
}

static int quality_cut(const std::string &q, int L, int qual_min, int qual_base)
{
    int suf[64][16], incl[64];
    for (int c = 0; c < 64; ++c) {
        const int left = L - 16 * c < 0 ? 0 : (L - 16 * c > 16 ? 16 : L - 16 * c);
        uint32_t w[4];
        load16(q, L, c, w);
        rc_trim_qual_suffix(w, left, qual_min, qual_base, suf[c]);
        incl[c] = suf[c][0];
    }
    for (int sft = 1; sft < 64; sft <<= 1) {  // (every lane reads the lane sft above it, then all add)
        int other[64];
        for (int c = 0; c < 64; ++c) other[c] = c + sft < 64 ? incl[c + sft] : 0;
        for (int c = 0; c < 64; ++c)
            if (c + sft < 64) incl[c] += other[c];
    }
    int i0 = -1;
    for (int c = 0; c < 64; ++c) {
        const int left = L - 16 * c < 0 ? 0 : (L - 16 * c > 16 ? 16 : L - 16 * c);
        const int x = rc_trim_qual_neg(suf[c], incl[c] - suf[c][0], left, 16 * c);
        i0 = x > i0 ? x : i0;
    }
    uint32_t best = rc_trim_qual_key(0, L);
    for (int c = 0; c < 64; ++c) {
        const int left = L - 16 * c < 0 ? 0 : (L - 16 * c > 16 ? 16 : L - 16 * c);
        const uint32_t key = rc_trim_qual_best(suf[c], incl[c] - suf[c][0], left, 16 * c, i0);
        best = key > best ? key : best;
    }
    return rc_trim_qual_key_pos(best);
}

int main(int argc, char **argv)
{
    if (argc < 14) return 2;
    const int nw = atoi(argv[2]), mates = atoi(argv[3]), qual_min = atoi(argv[4]), qual_base = atoi(argv[5]);
    const std::string ad_text[2] = {strcmp(argv[6], "-") ? argv[6] : "", strcmp(argv[7], "-") ? argv[7] : ""};
    const int ad_min = atoi(argv[8]), ad_mm = atoi(argv[9]), pair_on = atoi(argv[10]), pair_min = atoi(argv[11]), pair_mm = atoi(argv[12]);
    const int min_len = atoi(argv[13]);
    const int lmax = 32 * nw < RC_TRIM_MAX_LEN ? 32 * nw : RC_TRIM_MAX_LEN;
    uint64_t ad[2][2 * RC_TRIM_AD_WORDS];
    for (int mt = 0; mt < 2; ++mt)
        if (!rc_trim_pack_adapter((const uint8_t *)ad_text[mt].data(), (int)ad_text[mt].size(), ad[mt], ad[mt] + RC_TRIM_AD_WORDS)) {
            printf("bad adapter %d\n", mt + 1);
            return 1;
        }
    std::ifstream in(argv[1]);
    std::vector<uint64_t> str(6 * nw);
    std::string seq[2], qual[2];
    for (;;) {
        bool ok = true, has_q[2] = {false, false};
        for (int mt = 0; mt < mates && ok; ++mt) {
            std::string q;
            if (!std::getline(in, seq[mt]) || seq[mt].empty() || seq[mt][0] != '=' || !std::getline(in, q) || q.empty()) ok = false;
            else {
                seq[mt].erase(0, 1);
                has_q[mt] = q[0] == '=';
                qual[mt] = has_q[mt] ? q.substr(1) : "";
            }
        }
        if (!ok) break;
        int len[2] = {0, 0};
        for (int mt = 0; mt < mates; ++mt) {
            len[mt] = std::min<int>((int)seq[mt].size(), lmax);
            stage(seq[mt], len[mt], nw, &str[mt ? 4 * nw : 0], &str[(mt ? 4 * nw : 0) + nw]);
        }
        const int La = len[0], Lb = len[1];
        int cut_q[2] = {La, Lb}, cut_ad[2] = {La, Lb}, cut_pair[2] = {La, Lb}, overlapping = 0;
        if (mates == 2 && pair_on) {
            for (int what = 0; what < 2; ++what)
                for (int w = 0; w < nw; ++w) str[(2 + what) * nw + w] = rc_ov_rc_word(&str[4 * nw + what * nw], nw, Lb, w, what == 0);
            const uint64_t *a_code = &str[0], *a_val = a_code + nw, *r_code = a_code + 2 * nw, *r_val = a_code + 3 * nw;
            const int nwa = (La + 31) >> 5;
            int d_lo, d_hi;
            rc_ov_offsets(La, Lb, pair_min, d_lo, d_hi);
            uint32_t best = 0;
            for (int d0 = d_lo; d0 <= d_hi; d0 += 64)
                for (int lane = 0; lane < 64; ++lane) {
                    const int d = d0 + lane;
                    if (d > d_hi) continue;
                    int v, m;
                    rc_ov_count(a_code, a_val, nwa, r_code, r_val, nw, d, v, m);
                    const uint32_t key = rc_ov_key(v, m, d, pair_min, pair_mm);
                    best = key > best ? key : best;
                }
            if (best) {
                rc_trim_pair_cuts(La, Lb, rc_ov_key_d(best), cut_pair[0], cut_pair[1]);
                overlapping = 1;
            }
        }
        bool kept = true;
        for (int mt = 0; mt < mates; ++mt) {
            const int L = len[mt];
            if (!ad_text[mt].empty()) {
                const uint64_t *m_code = &str[mt ? 4 * nw : 0], *m_val = m_code + nw;
                bool found = false;
                for (int d0 = 0; d0 < L && !found; d0 += 64)
                    for (int lane = 0; lane < 64 && !found; ++lane) {  // (the lowest lane of the first round with a hit)
                        const int d = d0 + lane;
                        if (d >= L) continue;
                        int v, m;
                        rc_trim_ad_count(m_code, m_val, (L + 31) >> 5, ad[mt], ad[mt] + RC_TRIM_AD_WORDS, d, v, m);
                        if (rc_trim_ad_accepts(v, m, ad_min, ad_mm)) {
                            cut_ad[mt] = d;
                            found = true;
                        }
                    }
            }
            if (has_q[mt] && qual_min > 0) cut_q[mt] = quality_cut(qual[mt], L, qual_min, qual_base);
            const int keep_len = rc_trim_keep_len(cut_q[mt], cut_ad[mt], cut_pair[mt]);
            kept = kept && keep_len >= min_len;
            printf("%d %d %d %d\n", keep_len, cut_q[mt], cut_ad[mt], cut_pair[mt]);
        }
        printf("unit %d %d\n", kept ? 1 : 0, overlapping);
    }
    return 0;
}
