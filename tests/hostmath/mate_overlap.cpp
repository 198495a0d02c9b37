// The per-pair arithmetic of the mate-overlap report (rcorrector_amd/csrc/rc_overlap.h) as a host program that runs the kernel's
// lanes one after the other: stage 16 bytes a lane, reverse and complement mate 2 a word a lane, an offset a lane and the
// largest key, a position a lane at d*.  Reads pairs from a text file -- four lines a pair, mate 1 and mate 2 as read, mate 1
// and mate 2 as corrected, each line '=' and the bases -- and prints the counts of an rc_mate_overlap; tests/
// test_mate_overlap_host.py compares them with a brute-force restatement of the definitions.
//   mate_overlap FILE MIN_OVERLAP MAX_MISMATCH_PCT NW      (NW: words a mate, 8 or 32, as k_mate_overlap's instances)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "rc_overlap.h"

static uint64_t tot[12], frag[RC_OV_FRAG], cmp5[2][RC_OV_POS], disb5[2][RC_OV_POS], disa5[2][RC_OV_POS];

// the strings of one mate: chunk c is bytes [16 c, 16 c + 16) of the read, bytes behind its end as 0
static void stage(const std::string &s, int len, int nw, uint64_t *code, uint64_t *val)
{
    std::vector<uint32_t> c32(2 * nw), v32(2 * nw);
    for (int c = 0; c < 2 * nw; ++c) {
        uint32_t w[4] = {0, 0, 0, 0};
        for (int j = 0; j < 16; ++j)
            if (16 * c + j < len) w[j >> 2] |= (uint32_t)(uint8_t)s[16 * c + j] << (8 * (j & 3));
        uint32_t code16, val16;
        rc_ov_pack16(w, code16, val16);
        c32[c ^ 1] = code16;  // (chunk 2 w is the high half of word w)
        v32[c ^ 1] = val16;
    }
    for (int w = 0; w < nw; ++w) {
        code[w] = ((uint64_t)c32[2 * w + 1] << 32) | c32[2 * w];
        val[w] = ((uint64_t)v32[2 * w + 1] << 32) | v32[2 * w];
    }
}

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const int min_ov = atoi(argv[2]), pct = atoi(argv[3]), nw = atoi(argv[4]);
    const int lmax = 32 * nw < RC_OV_MAX_LEN ? 32 * nw : RC_OV_MAX_LEN;
    std::ifstream in(argv[1]);
    std::string ln[4];
    std::vector<uint64_t> str(12 * nw);
    for (;;) {
        bool ok = true;
        for (int q = 0; q < 4; ++q) {
            if (!std::getline(in, ln[q]) || ln[q].empty() || ln[q][0] != '=') ok = false;
            else ln[q].erase(0, 1);
        }
        if (!ok) break;
        const int La = std::min<int>((int)ln[0].size(), lmax), Lb = std::min<int>((int)ln[1].size(), lmax);
        ++tot[0];
        for (int vr = 0; vr < 2; ++vr) {
            stage(ln[2 * vr], La, nw, &str[vr * 4 * nw], &str[vr * 4 * nw + nw]);
            stage(ln[2 * vr + 1], Lb, nw, &str[8 * nw + vr * 2 * nw], &str[8 * nw + vr * 2 * nw + nw]);
            for (int what = 0; what < 2; ++what)
                for (int w = 0; w < nw; ++w)
                    str[vr * 4 * nw + (2 + what) * nw + w] = rc_ov_rc_word(&str[8 * nw + vr * 2 * nw + what * nw], nw, Lb, w, what == 0);
        }
        const uint64_t *a_code = &str[0], *a_val = a_code + nw, *r_code = a_code + 2 * nw, *r_val = a_code + 3 * nw;
        const uint64_t *c_code = &str[4 * nw], *c_val = c_code + nw, *q_code = c_code + 2 * nw, *q_val = c_code + 3 * nw;
        const int nwa = (La + 31) >> 5;
        int d_lo, d_hi;
        rc_ov_offsets(La, Lb, min_ov, d_lo, d_hi);
        uint32_t best = 0;
        for (int d0 = d_lo; d0 <= d_hi; d0 += 64)
            for (int lane = 0; lane < 64; ++lane) {
                const int d = d0 + lane;
                if (d > d_hi) continue;
                int v, m;
                rc_ov_count(a_code, a_val, nwa, r_code, r_val, nw, d, v, m);
                const uint32_t key = rc_ov_key(v, m, d, min_ov, pct);
                best = key > best ? key : best;
            }
        if (!best) continue;
        const int ds = rc_ov_key_d(best);
        uint64_t cb = 0, db = 0, ca = 0, da = 0;
        for (int i = 0; i < ((La + 63) & ~63); ++i) {
            const int w = i >> 5;
            const rc_ov_faced fb = rc_ov_face(a_code, a_val, r_code, r_val, nw, ds, w), fa = rc_ov_face(c_code, c_val, q_code, q_val, nw, ds, w);
            const uint64_t bit = rc_ov_bit(i);
            const bool vb = fb.both & bit, xb = fb.differ & bit, va = fa.both & bit, xa = fa.differ & bit;
            const int p1 = i & (RC_OV_POS - 1), p2 = (Lb - 1 - (i - ds)) & (RC_OV_POS - 1);
            if (vb) ++cmp5[0][p1], ++cmp5[1][p2];
            if (xb) ++disb5[0][p1], ++disb5[1][p2];
            if (xa) ++disa5[0][p1], ++disa5[1][p2];
            cb += vb, db += xb, ca += va, da += xa;
            tot[6] += xb && va && !xa;
            tot[7] += vb && !xb && xa;
            tot[8] += xb && xa;
        }
        ++tot[1];
        tot[2] += cb, tot[3] += db, tot[4] += ca, tot[5] += da;
        ++tot[da < db ? 9 : (da > db ? 10 : 11)];
        ++frag[(ds + Lb) & (RC_OV_FRAG - 1)];
    }
    printf("tot");
    for (int t = 0; t < 12; ++t) printf(" %llu", (unsigned long long)tot[t]);
    printf("\n");
    for (int f = 0; f < RC_OV_FRAG; ++f)
        if (frag[f]) printf("frag %d %llu\n", f, (unsigned long long)frag[f]);
    for (int m = 0; m < 2; ++m)
        for (int p = 0; p < RC_OV_POS; ++p)
            if (cmp5[m][p] || disb5[m][p] || disa5[m][p])
                printf("pos %d %d %llu %llu %llu\n", m, p, (unsigned long long)cmp5[m][p], (unsigned long long)disb5[m][p], (unsigned long long)disa5[m][p]);
    return 0;
}
