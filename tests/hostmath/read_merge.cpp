// The merging contract (rcorrector_amd/csrc/rc_merge.h) as a host program that runs the kernels' lanes one after the other.  The
// plan: stage 16 bytes a lane, reverse and complement mate 2 a word a lane, an offset a lane for the pair scan, the row from the
// best key.  The write: the mates' bytes staged 16 a lane, then one aligned 16-byte granule of the output arena a lane, whole
// granules stored whole and the others byte by byte -- into arenas filled with a poison byte, the units one behind the other as
// the exclusive scan places them.  Reads units from a text file -- per mate two lines, '=' and the bases, then '=' and the
// quality bytes or '-' for none -- and prints per unit "row <merged_len> <d> <v> <m>", "seq <hex>" and "qual <hex>" (the unit's
// bytes of the output arenas, its NUL included; "qual -" without qualities), then "took <mate1> <mate2> <ties>" and "tail clean"
// if no byte at or behind the arena's end was written; tests/test_read_merge_host.py compares them with tests/merge_model.py.
//   read_merge FILE NW MIN_OVERLAP MAX_MISMATCH_PCT QUAL_BASE QUAL_CAP
//   (NW: words a mate, 8 or 32, as the kernels' instances)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "rc_merge.h"

static const uint8_t POISON = 0xEE;

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

// the write kernel's staging: 16 bytes a lane into a string of 32 nw bytes
static void stage_bytes(const std::string &s, int len, int nw, uint8_t *out)
{
    for (int c = 0; c < 2 * nw; ++c) {
        uint32_t w[4];
        load16(s, len, c, w);
        memcpy(out + 16 * c, w, 16);
    }
}

static void hex(const char *what, const std::vector<uint8_t> &arena, size_t beg, size_t end)
{
    printf("%s ", what);
    for (size_t i = beg; i < end; ++i) printf("%02x", arena[i]);
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    const int nw = atoi(argv[2]);
    rc_merge_rule R;
    R.min_overlap = atoi(argv[3]);
    R.max_mismatch_pct = atoi(argv[4]);
    R.qual_base = atoi(argv[5]);
    R.qual_cap = atoi(argv[6]);
    if (!rc_merge_rule_ok(R) || (nw != 8 && nw != 32)) {
        printf("bad parameters\n");
        return 1;
    }
    const int lmax = 32 * nw < RC_MERGE_MAX_LEN ? 32 * nw : RC_MERGE_MAX_LEN;
    std::ifstream in(argv[1]);
    std::vector<std::string> seq, qual;
    bool has_q = false;
    size_t in_bytes = 0;
    for (;;) {
        std::string s, q;
        if (!std::getline(in, s) || s.empty() || s[0] != '=' || !std::getline(in, q) || q.empty()) break;
        seq.push_back(s.substr(1));
        has_q = q[0] == '=';
        qual.push_back(has_q ? q.substr(1) : "");
        in_bytes += seq.back().size() + 1;
    }
    const size_t units = seq.size() / 2;
    // the plan
    std::vector<int> row(4 * units);
    std::vector<uint32_t> moff(units + 1, 0);
    std::vector<uint64_t> str(6 * nw);
    for (size_t u = 0; u < units; ++u) {
        const std::string &a = seq[2 * u], &b = seq[2 * u + 1];
        const int La = std::min<int>((int)a.size(), lmax), Lb = std::min<int>((int)b.size(), lmax);
        stage(a, La, nw, &str[0], &str[nw]);
        stage(b, Lb, nw, &str[4 * nw], &str[5 * nw]);
        for (int what = 0; what < 2; ++what)
            for (int w = 0; w < nw; ++w) str[(2 + what) * nw + w] = rc_ov_rc_word(&str[4 * nw + what * nw], nw, Lb, w, what == 0);
        const uint64_t *a_code = &str[0], *a_val = a_code + nw, *r_code = a_code + 2 * nw, *r_val = a_code + 3 * nw;
        const int nwa = (La + 31) >> 5;
        int d_lo, d_hi;
        rc_ov_offsets(La, Lb, R.min_overlap, d_lo, d_hi);
        uint32_t best = 0;
        for (int d0 = d_lo; d0 <= d_hi; d0 += 64)
            for (int lane = 0; lane < 64; ++lane) {
                const int d = d0 + lane;
                if (d > d_hi) continue;
                int v, m;
                rc_ov_count(a_code, a_val, nwa, r_code, r_val, nw, d, v, m);
                const uint32_t key = rc_ov_key(v, m, d, R.min_overlap, R.max_mismatch_pct);
                best = key > best ? key : best;
            }
        rc_merge_row(best, Lb, row[4 * u], row[4 * u + 1], row[4 * u + 2], row[4 * u + 3]);
        moff[u + 1] = moff[u] + (uint32_t)row[4 * u] + 1u;  // (the exclusive scan)
    }
    // the write, into arenas of the input's size with poison behind them too
    const size_t cap = in_bytes, total = moff[units];
    if (total > cap) {
        printf("the merged arena of %zu bytes exceeds the input's %zu\n", total, cap);
        return 1;
    }
    std::vector<uint8_t> mseq(cap + 64, POISON), mqual(cap + 64, POISON);
    std::vector<uint8_t> raw(4 * 32 * nw);
    uint32_t tk[3] = {0, 0, 0};
    for (size_t u = 0; u < units; ++u) {
        const int F = row[4 * u];
        const size_t beg = moff[u];
        if (F == 0) {
            mseq[beg] = 0;
            if (has_q) mqual[beg] = 0;
            continue;
        }
        const std::string &a = seq[2 * u], &b = seq[2 * u + 1];
        rc_merge_unit U;
        U.La = std::min<int>((int)a.size(), lmax);
        U.Lb = std::min<int>((int)b.size(), lmax);
        U.d = row[4 * u + 1];
        U.F = F;
        stage_bytes(a, U.La, nw, &raw[0]);
        stage_bytes(b, U.Lb, nw, &raw[2 * 32 * nw]);
        if (has_q) {
            stage_bytes(qual[2 * u], U.La, nw, &raw[32 * nw]);
            stage_bytes(qual[2 * u + 1], U.Lb, nw, &raw[3 * 32 * nw]);
        }
        U.a = &raw[0];
        U.qa = has_q ? &raw[32 * nw] : nullptr;
        U.b = &raw[2 * 32 * nw];
        U.qb = has_q ? &raw[3 * 32 * nw] : nullptr;
        const uint32_t lead = (uint32_t)(beg & 15u), n_gran = (lead + (uint32_t)F + 1u + 15u) >> 4;
        for (uint32_t g0 = 0; g0 < n_gran; g0 += 64)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t g = g0 + lane;
                if (g >= n_gran) continue;
                uint32_t ws[4], wq[4];
                const uint32_t mask = rc_merge_granule(R, U, (int)(16u * g) - (int)lead, ws, wq, tk);
                const size_t at = beg - lead + 16u * (size_t)g;
                if (mask == 0xFFFFu) {
                    memcpy(&mseq[at], ws, 16);
                    if (has_q) memcpy(&mqual[at], wq, 16);
                } else {
                    for (int k = 0; k < 16; ++k)
                        if ((mask >> k) & 1u) {
                            mseq[at + k] = (uint8_t)(ws[k >> 2] >> (8 * (k & 3)));
                            if (has_q) mqual[at + k] = (uint8_t)(wq[k >> 2] >> (8 * (k & 3)));
                        }
                }
            }
    }
    for (size_t u = 0; u < units; ++u) {
        printf("row %d %d %d %d\n", row[4 * u], row[4 * u + 1], row[4 * u + 2], row[4 * u + 3]);
        hex("seq", mseq, moff[u], moff[u + 1]);
        if (has_q) hex("qual", mqual, moff[u], moff[u + 1]);
        else printf("qual -\n");
    }
    printf("took %u %u %u\n", tk[0], tk[1], tk[2]);
    bool clean = true;
    for (size_t i = total; i < mseq.size(); ++i) clean = clean && mseq[i] == POISON && mqual[i] == POISON;
    if (!has_q)
        for (size_t i = 0; i < total; ++i) clean = clean && mqual[i] == POISON;
    printf(clean ? "tail clean\n" : "tail WRITTEN\n");
    return 0;
}
