// rc_format.cpp -- see rc_format.h
#include "rc_format.h"

#include <zlib.h>

// Reads.h:224-266 for a whole block: sequence -> NUL-terminated arena, quality cut / padded to the
// sequence length for the kernels (the output prints the quality line verbatim, see put_record)
uint64_t index_arena(Arena &A, const std::string &path)
{
    const size_t n = A.n();
    A.off.resize(n + 1);
    A.off[0] = 0;
    uint64_t total = 0;
    for (size_t r = 0; r < n; ++r) {
        uint32_t sl, il;
        A.line(r, 1, &sl);
        A.line(r, 0, &il);
        if (sl > MAX_READ_LENGTH - 1)
            die("ERROR: %s: a read of %u bases exceeds the limit of %d (utils.h:7)\n", path.c_str(), sl, MAX_READ_LENGTH - 1);
        if (il > MAX_ID_LENGTH - 1) die("ERROR: %s: a header line longer than %d characters\n", path.c_str(), MAX_ID_LENGTH - 1);
        total += sl + 1;
        A.off[r + 1] = (uint32_t)total;
    }
    if (total >= (1ull << 32)) die("ERROR: batch too large; lower -batch\n");
    return total;
}

// the sequences alone, NUL-terminated, at dst (A.off must be set): what the k-mer counter is given
void pack_sequences(const Arena &A, char *dst)
{
    parallel_for(A.n(), [&](size_t lo, size_t hi) {
        for (size_t r = lo; r < hi; ++r) {
            uint32_t sl;
            const char *s = A.line(r, 1, &sl);
            char *d = dst + A.off[r];
            memcpy(d, s, sl);
            d[sl] = 0;
        }
    });
}

void pack_arena(Arena &A, const std::string &path)
{
    const size_t n = A.n();
    const uint64_t total = index_arena(A, path);
    A.seq_in_text = false;
    A.seq.need(total);
    A.qual.need(total);
    parallel_for(n, [&](size_t lo, size_t hi) {
        for (size_t r = lo; r < hi; ++r) {
            uint32_t sl, ql = 0;
            const char *s = A.line(r, 1, &sl);
            char *d = A.seq.data() + A.off[r];
            memcpy(d, s, sl);
            d[sl] = 0;
            char *dq = A.qual.data() + A.off[r];
            uint32_t qc = 0;
            if (A.lpr == 4) {
                const char *q = A.line(r, 3, &ql);
                qc = std::min(ql, sl);
                memcpy(dq, q, qc);
            }
            memset(dq + qc, 0, sl + 1 - qc);
        }
    });
}

bool pack_quality_bits_from_text(const QualView &V, char bad_q, size_t lo, size_t hi, uint8_t *bits)
{
    bool ok = true;
    uint64_t acc = 0;
    int nacc = 0;
    uint8_t *out = bits + (lo >> 3);
    auto put = [&](uint64_t v, int nb) {  // nb <= 16 bits at a time; four bytes leave at once (they all belong to this range)
        acc |= v << nacc;
        nacc += nb;
        if (nacc >= 32) {
            const uint32_t w = (uint32_t)acc;
            memcpy(out, &w, 4);
            out += 4;
            acc >>= 32;
            nacc -= 32;
        }
    };
    const __m128i thr = _mm_set1_epi8(bad_q);
    const bool zero_above = (signed char)0 > (signed char)bad_q;  // (a negative threshold: the padding compares as "good")
    size_t pos = lo;
    while (pos < hi) {
        const int sd = pos >= V.bytes1 ? 1 : 0;
        const Arena &A = *V.A[sd];
        const size_t base = sd ? V.bytes1 : 0, p = pos - base;
        const size_t r = (size_t)(std::upper_bound(A.off.begin(), A.off.begin() + (ptrdiff_t)A.n() + 1, (uint32_t)p) - A.off.begin()) - 1;
        const size_t end_side = std::min(hi, sd ? V.nbytes : V.bytes1);
        for (size_t rr = r; rr < A.n() && base + A.off[rr] < end_side; ++rr) {
            const uint32_t sl = A.off[rr + 1] - A.off[rr] - 1;
            uint32_t ql = 0;
            const char *q = A.line(rr, 3, &ql);
            const uint32_t qc = std::min(ql, sl);
            if (sl && (qc == 0 || q[0] == 0)) ok = false;
            // this read's positions inside [lo, hi): characters j0 .. j1 - 1 of its sl + 1 bytes
            const size_t r0 = base + A.off[rr];
            const uint32_t j0 = r0 < pos ? (uint32_t)(pos - r0) : 0;
            const uint32_t j1 = (uint32_t)std::min<size_t>(sl + 1, end_side - r0);
            uint32_t j = j0;
            while (j < j1) {
                const uint32_t nb = std::min<uint32_t>(16, j1 - j);
                uint32_t m = 0;
                if (j < qc) {  // (the text buffer carries 64 bytes of slack behind its last line)
                    m = (uint32_t)_mm_movemask_epi8(_mm_cmpgt_epi8(_mm_loadu_si128((const __m128i *)(q + j)), thr));
                    if (qc - j < 16) {
                        const uint32_t keep = (1u << (qc - j)) - 1u;
                        m = (m & keep) | (zero_above ? (0xffffu & ~keep) : 0u);
                    }
                } else if (zero_above) {
                    m = 0xffffu;
                }
                put(m & ((1u << nb) - 1u), (int)nb);
                j += nb;
            }
            pos = r0 + j1;
        }
        if (pos < end_side) pos = end_side;  // (cannot happen: the reads tile the arena)
    }
    for (; nacc > 0; nacc -= 8) {  // (the last byte is a partial one only at the arena's end)
        *out++ = (uint8_t)acc;
        acc >>= 8;
    }
    return ok;
}

void pack_quality_bits_from_arenas(const QualView &V, char bad_q, size_t lo, size_t hi, uint8_t *bits)
{
    const char *q1 = V.A[0]->qual.data(), *q2 = V.A[1]->qual.data();
    for (size_t p8 = lo; p8 < hi; p8 += 8) {
        unsigned v = 0;
        for (size_t q = p8; q < std::min(p8 + 8, hi); ++q) {
            const signed char c = (signed char)(q < V.bytes1 ? q1[q] : q2[q - V.bytes1]);
            v |= (unsigned)(c > (signed char)bad_q) << (q - p8);
        }
        bits[p8 >> 3] = (uint8_t)v;
    }
}

// One bit per quality cannot say "this read has no quality string" (qual[0] == 0: an empty quality line in a FASTQ file;
// ErrorCorrection.cpp:1316 asks): such a batch takes the bytes
bool has_empty_quality_read(const Job &J)
{
    if (!J.fastq) return false;
    for (int sd = 0; sd < (J.mode == 1 ? 2 : 1); ++sd) {
        const Arena &A = sd ? J.b : J.a;
        for (size_t r = 0; r < A.n(); ++r)
            if (A.off[r + 1] - A.off[r] > 1 && A.qual.data()[A.off[r]] == 0) return true;
    }
    return false;
}

void combined_offsets(const Job &J, uint32_t *off)
{
    const size_t n = J.a.n();
    memcpy(off, J.a.off.data(), (n + 1) * 4);
    if (J.mode == 1)
        for (size_t r = 0; r <= n; ++r) off[n + r] = J.a.off[n] + J.b.off[r];
}

size_t pack_bases_of(Job &J, size_t nbytes, size_t bytes1)
{
    const size_t n_words = (nbytes + 15) / 16;
    J.pk_bases.need(n_words * 4 + 64);
    uint32_t *bases = (uint32_t *)J.pk_bases.data();
    const size_t P = std::max<size_t>(1, std::min<size_t>((size_t)g_threads, n_words / 4096 + 1));
    std::vector<std::vector<uint32_t>> ep(P);  // the exceptions of each piece
    std::vector<std::vector<uint8_t>> ec(P);
    g_pool.run(P, [&](size_t t) {
        const size_t lo = (n_words * t / P) * 16, hi = std::min((n_words * (t + 1) / P) * 16, nbytes);
        for (int pass = 0; pass < 2; ++pass) {  // (first pass counts the exceptions, second stores them)
            uint32_t *pp = pass ? ep[t].data() : nullptr;
            uint8_t *pc = pass ? ec[t].data() : nullptr;
            const size_t room = pass ? ep[t].size() : 0;
            size_t got = 0, cnt = 0;
            if (lo < bytes1) cnt += (got = rc_pack_bases(J.a.seq.data(), lo, std::min(hi, bytes1), bases, pp, pc, room));
            if (hi > bytes1) {  // arena 2's share, behind what arena 1's left in the lists
                const size_t used = std::min(got, room);
                cnt += rc_pack_bases(J.b.seq.data() - bytes1, std::max(lo, bytes1), hi, bases, pp ? pp + used : nullptr, pc ? pc + used : nullptr, room - used);
            }
            if (pass == 0) {
                if (cnt == 0) break;
                ep[t].resize(cnt);
                ec[t].resize(cnt);
            }
        }
    });
    size_t n_exc = 0;
    for (size_t t = 0; t < P; ++t) n_exc += ep[t].size();
    J.pk_exc_pos.need(n_exc * 4 + 64);
    J.pk_exc_chr.need(n_exc + 64);
    size_t at = 0;
    for (size_t t = 0; t < P; ++t) {
        if (ep[t].empty()) continue;
        memcpy(J.pk_exc_pos.data() + at * 4, ep[t].data(), ep[t].size() * 4);
        memcpy(J.pk_exc_chr.data() + at, ec[t].data(), ec[t].size());
        at += ep[t].size();
    }
    return n_exc;
}

void apply_fixes(Job &J, size_t bytes1, const uint32_t *fix_pos, const uint8_t *fix_chr, size_t n_fix)
{
    const size_t F = std::max<size_t>(1, std::min<size_t>((size_t)g_threads, n_fix / 16384 + 1));
    g_pool.run(F, [&](size_t t) {
        const size_t lo = n_fix * t / F, hi = n_fix * (t + 1) / F;
        if (J.a.seq_in_text) {
            apply_fixes_to_text(J.a, J.mode == 1 ? &J.b : nullptr, bytes1, fix_pos, fix_chr, lo, hi);
            return;
        }
        for (size_t q = lo; q < hi; ++q) {
            const size_t pos = fix_pos[q];
            (pos < bytes1 ? J.a.seq.data()[pos] : J.b.seq.data()[pos - bytes1]) = (char)fix_chr[q];
        }
    });
}

void apply_fixes_to_text(Arena &A1, Arena *A2, size_t bytes1, const uint32_t *fix_pos, const uint8_t *fix_chr, size_t lo, size_t hi)
{
    for (size_t q = lo; q < hi; ++q) {
        size_t p = fix_pos[q];
        Arena &A = (A2 && p >= bytes1) ? *A2 : A1;
        if (&A == A2) p -= bytes1;
        const size_t n = A.n();
        size_t r;
        const uint32_t stride = A.off[1];
        if ((uint64_t)stride * n == A.off[n] && A.off[p / stride] == (p / stride) * (size_t)stride && A.off[p / stride + 1] == (p / stride + 1) * (size_t)stride)
            r = p / stride;  // reads of one length
        else
            r = (size_t)(std::upper_bound(A.off.begin(), A.off.begin() + (ptrdiff_t)n + 1, (uint32_t)p) - A.off.begin()) - 1;
        A.blk.text.p[A.blk.line[r * (size_t)A.lpr + 1] + (p - A.off[r])] = (char)fix_chr[q];
    }
}

bool write_histo(const char *path, const std::vector<uint64_t> &freq)
{
    FILE *fp = fopen(path, "wb");
    if (!fp) return false;
    bool ok = true;
    for (size_t c = 1; c < freq.size() && ok; ++c)
        if (freq[c]) ok = fprintf(fp, "%zu %llu\n", c, (unsigned long long)freq[c]) > 0;
    return fclose(fp) == 0 && ok;
}

bool write_dup_census(const char *path, const rc_dup_census &D, uint32_t max_bin, const char *unit)
{
    FILE *fp = fopen(path, "wb");
    if (!fp) return false;
    typedef unsigned long long ull;
    bool ok = fprintf(fp, "units\t%llu\t%s\ndistinct\tbefore\t%llu\ndistinct\tafter\t%llu\n", (ull)D.units, unit, (ull)D.distinct_before, (ull)D.distinct_after) > 0;
    for (uint32_t c = 1; c <= max_bin && ok; ++c)
        if (D.copies_before[c] || D.copies_after[c]) ok = fprintf(fp, "copies\t%u\t%llu\t%llu\n", c, (ull)D.copies_before[c], (ull)D.copies_after[c]) > 0;
    return fclose(fp) == 0 && ok;
}

bool write_recur_census(const char *path, const rc_recur_census &R, uint32_t max_bin, uint32_t min_count)
{
    FILE *fp = fopen(path, "wb");
    if (!fp) return false;
    typedef unsigned long long ull;
    bool ok = fprintf(fp, "flank\t%d\nmin_count\t%u\nchanges\t%llu\ncontexted\t%llu\nclipped\t%llu\nsites\t%llu\n", RC_RECUR_FLANK, min_count, (ull)R.changes,
                      (ull)R.contexted, (ull)R.clipped, (ull)R.sites) > 0;
    for (uint32_t c = 1; c <= max_bin && ok; ++c)
        if (R.recur[c]) ok = fprintf(fp, "recur\t%u\t%llu\n", c, (ull)R.recur[c]) > 0;
    const int n = 2 * RC_RECUR_FLANK + 1;
    for (uint32_t i = 0; i < R.n_top && ok; ++i) {
        const uint64_t w = R.top_key[i] >> 3;
        const unsigned f = (unsigned)(R.top_key[i] & 7u);
        char text[2 * RC_RECUR_FLANK + 2];
        for (int j = 0; j < n; ++j) text[j] = "ACGT"[(w >> (2 * (n - 1 - j))) & 3u];
        text[n] = 0;
        ok = fprintf(fp, "site\t%llu\t%c\t%c\t%s\n", (ull)R.top_count[i], f < 4 ? "ACGT"[f] : 'N', text[RC_RECUR_FLANK], text) > 0;
    }
    return fclose(fp) == 0 && ok;
}

bool write_depth_report(const char *path, int k, const uint64_t reads[2], const uint64_t novalid[2], const std::vector<uint64_t> hist[2], bool two_mates)
{
    FILE *fp = fopen(path, "wb");
    if (!fp) return false;
    typedef unsigned long long ull;
    const int mates = two_mates ? 2 : 1;
    bool ok = fprintf(fp, "k\t%d\n", k) > 0;
    for (int m = 0; m < mates; ++m) ok = ok && fprintf(fp, "reads\t%d\t%llu\n", m + 1, (ull)reads[m]) > 0;
    for (int m = 0; m < mates; ++m) ok = ok && fprintf(fp, "novalid\t%d\t%llu\n", m + 1, (ull)novalid[m]) > 0;
    for (size_t d = 0; d < std::max(hist[0].size(), hist[1].size()) && ok; ++d) {
        const uint64_t h1 = d < hist[0].size() ? hist[0][d] : 0, h2 = d < hist[1].size() ? hist[1][d] : 0;
        if (!h1 && !(two_mates && h2)) continue;
        ok = (two_mates ? fprintf(fp, "median\t%zu\t%llu\t%llu\n", d, (ull)h1, (ull)h2) : fprintf(fp, "median\t%zu\t%llu\n", d, (ull)h1)) > 0;
    }
    return fclose(fp) == 0 && ok;
}

size_t depth_median_of_medians(const std::vector<uint64_t> hist[2])
{
    uint64_t n = 0;
    for (int m = 0; m < 2; ++m)
        for (uint64_t c : hist[m]) n += c;
    if (!n) return 0;
    uint64_t seen = 0;
    for (size_t d = 0; d < std::max(hist[0].size(), hist[1].size()); ++d) {
        seen += (d < hist[0].size() ? hist[0][d] : 0) + (d < hist[1].size() ? hist[1][d] : 0);
        if (seen > (n - 1) / 2) return d;
    }
    return 0;
}

void add_trust_profile(rc_trust_profile &to, const rc_trust_profile &from)
{
    to.reads[0] += from.reads[0];
    to.reads[1] += from.reads[1];
    static_assert(sizeof(rc_trust_counts) % 8 == 0, "64-bit counts throughout");
    uint64_t *t = (uint64_t *)&to.before;
    const uint64_t *f = (const uint64_t *)&from.before;
    for (size_t i = 0; i < 2 * sizeof(rc_trust_counts) / 8; ++i) t[i] += f[i];  // (before | after)
}

bool write_trust_profile(const char *path, const rc_trust_profile &T, bool two_mates)
{
    FILE *fp = fopen(path, "wb");
    if (!fp) return false;
    typedef unsigned long long ull;
    const int mates = two_mates ? 2 : 1;
    bool ok = fprintf(fp, "k\t%d\nmin_count\t%d\n", T.k, T.min_count) > 0;
    for (int m = 0; m < mates; ++m) ok = ok && fprintf(fp, "reads\t%d\t%llu\n", m + 1, (ull)T.reads[m]) > 0;
    const rc_trust_counts *ver[2] = {&T.before, &T.after};
    const char *name[2] = {"before", "after"};
    for (int v = 0; v < 2; ++v)
        for (int m = 0; m < mates; ++m) {
            ull w = 0, s = 0, k = 0;
            for (int p = 0; p < RC_TRUST_MAX_LEN; ++p) {
                w += ver[v]->windows[m][p];
                s += ver[v]->solid5[m][p];
                k += ver[v]->weak5[m][p];
            }
            ok = ok && fprintf(fp, "total\t%s\t%d\t%llu\t%llu\t%llu\t%llu\n", name[v], m + 1, w, s, k, w - s - k) > 0;
        }
    for (int end = 0; end < 2; ++end)
        for (int v = 0; v < 2; ++v)
            for (int m = 0; m < mates; ++m)
                for (int p = 0; p < RC_TRUST_MAX_LEN && ok; ++p) {
                    const ull w = ver[v]->windows[m][p], s = end ? ver[v]->solid3[m][p] : ver[v]->solid5[m][p],
                              k = end ? ver[v]->weak3[m][p] : ver[v]->weak5[m][p];
                    if (w) ok = fprintf(fp, "%s\t%s\t%d\t%d\t%llu\t%llu\t%llu\t%llu\n", end ? "pos3" : "pos5", name[v], m + 1, p, w, s, k, w - s - k) > 0;
                }
    return fclose(fp) == 0 && ok;
}

void add_mate_overlap(rc_mate_overlap &to, const rc_mate_overlap &from)
{
    static_assert(sizeof(rc_mate_overlap) % 8 == 0, "64-bit counts throughout");
    uint64_t *t = (uint64_t *)&to.pairs;
    const uint64_t *f = (const uint64_t *)&from.pairs;
    for (size_t i = 0; i < (sizeof(rc_mate_overlap) - offsetof(rc_mate_overlap, pairs)) / 8; ++i) t[i] += f[i];
}

std::string mate_overlap_text(const rc_mate_overlap &M)
{
    typedef unsigned long long ull;
    std::string out;
    char ln[256];
    auto put = [&](const char *fmt, auto... a) {
        snprintf(ln, sizeof ln, fmt, a...);
        out += ln;
    };
    put("min_overlap\t%llu\nmax_mismatch_pct\t%llu\npairs\t%llu\noverlapping\t%llu\n", (ull)M.min_overlap, (ull)M.max_mismatch_pct, (ull)M.pairs, (ull)M.overlapping);
    put("compared\tbefore\t%llu\ncompared\tafter\t%llu\n", (ull)M.compared_before, (ull)M.compared_after);
    put("disagree\tbefore\t%llu\ndisagree\tafter\t%llu\n", (ull)M.disagree_before, (ull)M.disagree_after);
    put("resolved\t%llu\nkept\t%llu\nintroduced\t%llu\n", (ull)M.resolved, (ull)M.kept, (ull)M.introduced);
    put("pairs\timproved\t%llu\npairs\tworsened\t%llu\npairs\tsame\t%llu\n", (ull)M.pairs_improved, (ull)M.pairs_worsened, (ull)M.pairs_same);
    for (int f = 0; f < RC_OVERLAP_FRAG_LEN; ++f)
        if (M.frag[f]) put("frag\t%d\t%llu\n", f, (ull)M.frag[f]);
    for (int m = 0; m < 2; ++m)
        for (int p = 0; p < RC_OVERLAP_MAX_LEN; ++p)
            if (M.compared5[m][p])
                put("pos5\t%d\t%d\t%llu\t%llu\t%llu\n", m + 1, p, (ull)M.compared5[m][p], (ull)M.disagree5_before[m][p], (ull)M.disagree5_after[m][p]);
    return out;
}

bool write_mate_overlap(const char *path, const rc_mate_overlap &M)
{
    FILE *fp = fopen(path, "wb");
    if (!fp) return false;
    const std::string text = mate_overlap_text(M);
    const bool ok = fwrite(text.data(), 1, text.size(), fp) == text.size();
    return fclose(fp) == 0 && ok;
}

bool write_change_report(const char *path, const rc_change_report &R, bool two_mates)
{
    FILE *fp = fopen(path, "wb");
    if (!fp) return false;
    typedef unsigned long long ull;
    const int mates = two_mates ? 2 : 1;
    bool ok = true;
    for (int m = 0; m < mates && ok; ++m)
        ok = fprintf(fp, "reads\t%d\t%llu\t%llu\t%llu\n", m + 1, (ull)R.reads[m], (ull)R.reads_changed[m], (ull)R.reads_unfixable[m]) > 0;
    for (int m = 0; m < mates && ok; ++m) ok = fprintf(fp, "changes\t%d\t%llu\n", m + 1, (ull)R.changes[m]) > 0;
    int longest[2] = {0, 0};
    for (int m = 0; m < mates; ++m)
        for (int l = 0; l < RC_REPORT_MAX_LEN; ++l)
            if (R.len_hist[m][l]) longest[m] = l;
    for (int m = 0; m < mates && ok; ++m) {
        // reads covering position p (counted from 1): those of at least p bases -- a suffix sum of the lengths
        std::vector<uint64_t> cover((size_t)longest[m] + 2, 0);
        for (int l = longest[m]; l >= 1; --l) cover[(size_t)l] = cover[(size_t)l + 1] + R.len_hist[m][l];
        for (int p = 1; p <= longest[m] && ok; ++p) ok = fprintf(fp, "pos5\t%d\t%d\t%llu\t%llu\n", m + 1, p, (ull)R.by_pos5[m][p - 1], (ull)cover[(size_t)p]) > 0;
    }
    for (int m = 0; m < mates && ok; ++m)
        for (int p = 1; p <= longest[m] && ok; ++p) ok = fprintf(fp, "pos3\t%d\t%d\t%llu\n", m + 1, p, (ull)R.by_pos3[m][p - 1]) > 0;
    for (int a = 0; a < 5 && ok; ++a)
        for (int b = 0; b < 4 && ok; ++b) ok = fprintf(fp, "subst\t%c\t%c\t%llu\n", "ACGTN"[a], "ACGT"[b], (ull)R.subst[a][b]) > 0;
    for (int q = 0; q < 3 && ok; ++q) ok = fprintf(fp, "qual\t%s\t%llu\n", q == 0 ? "low" : (q == 1 ? "high" : "none"), (ull)R.by_qual[q]) > 0;
    for (int c = 0; c <= RC_REPORT_MAX_PER_READ && ok; ++c) {
        if (!R.per_read[c]) continue;
        if (c < RC_REPORT_MAX_PER_READ)
            ok = fprintf(fp, "perread\t%d\t%llu\n", c, (ull)R.per_read[c]) > 0;
        else
            ok = fprintf(fp, "perread\t%d+\t%llu\n", c, (ull)R.per_read[c]) > 0;
    }
    return fclose(fp) == 0 && ok;
}

void quality_histograms(const Block &b, int lpr, size_t room, std::vector<int32_t> &fh, std::vector<int32_t> &lh, int *total)
{
    static char qbuf[MAX_READ_LENGTH];  // Reads::qual, reused from record to record
    for (size_t r = 0; r < b.records && r < room; ++r) {
        const uint32_t *L = b.line.data() + r * (size_t)lpr;
        const uint32_t sl = L[2] - L[1] - 1, ql = lpr == 4 ? L[4] - L[3] - 1 : 0;
        ++*total;
        if (lpr != 4) continue;
        const char *q = b.text.data() + L[3];
        // qual[strlen(seq)-1] and qual[0] as GetBadQuality sees them: Reads::Next reads every
        // quality line into ONE reused buffer (bytes behind a short line keep what earlier
        // records left there) and strips a newline only at index strlen(seq)
        // (Reads.h:204-219); qual[-1], for an empty sequence, is the last byte of the
        // sequence buffer in front of it, 0.
        const uint32_t qn = std::min<uint32_t>(ql, MAX_READ_LENGTH - 1);
        memcpy(qbuf, q, qn);
        if (qn + 1 < MAX_READ_LENGTH) {
            qbuf[qn] = '\n';
            qbuf[qn + 1] = 0;
        } else {
            qbuf[qn] = 0;
        }
        if (sl < MAX_READ_LENGTH && qbuf[sl] == '\n') qbuf[sl] = 0;
        const unsigned char lastq = sl ? (unsigned char)qbuf[sl - 1] : 0;
        const unsigned char firstq = (unsigned char)qbuf[0];
        ++lh[lastq];
        ++fh[firstq];
    }
}

void gzip_member(const OutBuf &in, OutBuf &out)
{
    const LibDeflate &LD = libdeflate();
    if (LD.ok) {
        static thread_local void *c = nullptr;  // (a compressor per thread: they are not shareable, and cost a few hundred KB)
        if (!c) c = LD.alloc_c(1);
        if (c) {
            out.resize(LD.gzip_bound(c, in.size()) + 64);
            const size_t n = LD.gzip(c, in.data(), in.size(), out.data(), out.size());
            if (n) {
                out.resize(n);
                return;
            }
        }
    }
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, 1, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) die("ERROR: zlib deflateInit2 failed\n");
    out.resize(deflateBound(&z, (uLong)in.size()) + 64);
    z.next_in = (Bytef *)in.data();
    z.avail_in = (uInt)in.size();
    z.next_out = (Bytef *)out.data();
    z.avail_out = (uInt)out.size();
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) die("ERROR: zlib deflate failed\n");
    out.resize(z.total_out);
    deflateEnd(&z);
}

void put_transcript(std::vector<char> &out, const Job &J, const Arena &A, size_t r, size_t gi, size_t ab, int k)
{
    uint32_t il, ol;
    const char *id = A.line(r, 0, &il);
    const char *orig = A.line(r, 1, &ol);
    const char *seq = A.seq.data() + A.off[r];
    const int len = (int)(A.off[r + 1] - A.off[r] - 1);
    const int kcnt = len >= k ? len - k + 1 : 0;
    const size_t a0 = ab + A.off[r];
    auto put = [&](const char *p, size_t n) { out.insert(out.end(), p, p + n); };
    auto puts_ = [&](const char *p) { put(p, strlen(p)); };
    auto puti = [&](int v) {
        char tmp[16];
        char *e = put_int(tmp, v);
        put(tmp, (size_t)(e - tmp));
    };
    put(id, il);
    puts_("\n");
    if (J.tr_flags[gi] & 1) {
        puts_("Before correction:\n");
        put(orig, (size_t)len);
        puts_("\n");
        for (int i = 0; i < kcnt; ++i) {
            const int c = J.tr_before[a0 + (size_t)i];
            puti(c != 0 ? c : 1);
            puts_(" ");
        }
        puts_("\n");
        const int n_it = J.tr_niter[gi];
        if (n_it > g_trace_iter)
            die("rcorrector: -verbose: read %.*s went through %d threshold iterations, more than the %d recorded; raise -verbose-iter\n",
                (int)il, id, n_it, g_trace_iter);
        for (int it = 0; it < n_it; ++it) {
            const int32_t *e = J.tr_iter.data() + (gi * (size_t)g_trace_iter + (size_t)it) * RC_TRACE_ITER_WORDS;
            puts_("strong trust threshold=");
            puti(e[0]);
            puts_(" threshold=");
            puti(e[1]);
            puts_("\n");
            if (e[2]) {
                puts_("Is corresponding base strong trusted?\n");
                for (int b = 0; b < len; ++b) out.push_back((char)('0' + (((uint32_t)e[4 + (b >> 5)] >> (b & 31)) & 1u)));
                puts_("\n");
            }
        }
    }
    // GetKmerInformation: the counts of the k-mers without a non-ACGT letter, 0 shown as 1
    int bad = 0, n_valid = 0;
    std::vector<int> cnt;
    for (int i = 0; i < len; ++i) {
        const char ch = seq[i];
        const bool ok = ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T';
        bad = ok ? (bad > 0 ? bad - 1 : 0) : k;  // windows ending at i are invalid while bad > 0
        if (i >= k - 1 && bad == 0) {
            const int c = J.tr_after[a0 + (size_t)(i - k + 1)];
            cnt.push_back(c != 0 ? c : 1);
            ++n_valid;
        }
    }
    if (n_valid > 0) {
        puts_("After coorrection:\n");
        put(seq, (size_t)len);
        puts_("\n");
        for (int c : cnt) {
            puti(c);
            puts_(" ");
        }
        puts_("\n");
    }
}
