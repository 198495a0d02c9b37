// rc_format.h -- a batch between the reader and the writer of the `rcorrector` CLI: the SoA arenas of the C ABI packed from
// the text, the host steps of the resident and packed transports (offsets, quality bits, 2-bit bases, fixes), and the output records.
//   record       Reads.h:224-266,360-421    4 lines in; "<id> l:%d m:%d h:%d[ cor| unfixable_error]" out
//   -weak-ends   Reads.h:396-412            " bad_prefix=%d" / " bad_suffix=%d" behind " cor": the reference's dormant tags
//   -depth-tags  (no reference counterpart) " kdepth=Q1:MED:Q3" behind those: the quartiles of the read's k-mer counts
//   transcript   ErrorCorrection.cpp:686-689,759-770,856-857,1088-1094,1590-1597 (-verbose)
#pragma once
#include <emmintrin.h>

#include "rc_reader.h"

// ---- one batch travelling through the pipeline -------------------------------------------------
struct Arena {  // one file's share of a batch
    Block blk;
    int lpr = 4;  // lines per record
    PinBuf seq, qual;
    std::vector<uint32_t> off;
    // resident batches (the reads are in HBM since they were counted): there is no byte arena here, the fixes are applied
    // to the sequence lines of the text itself
    bool seq_in_text = false;
    size_t n() const { return blk.records; }
    const char *sequence(size_t r) const { return seq_in_text ? blk.text.data() + blk.line[r * (size_t)lpr + 1] : seq.data() + off[r]; }
    const char *line(size_t rec, int which, uint32_t *len) const
    {
        const size_t li = rec * (size_t)lpr + (size_t)which;
        *len = blk.line[li + 1] - blk.line[li] - 1;
        return blk.text.data() + blk.line[li];
    }
};

struct Job {
    int file = 0;
    int mode = 0;
    bool fastq = true;
    Arena a, b;
    std::vector<int32_t> ret, l, m, h;
    std::vector<int32_t> tr_before, tr_after, tr_flags, tr_niter, tr_iter;  // -verbose only
    std::vector<rc_read_weak> weak;  // -weak-ends only: the corrected reads' profile, indexed like ret (rc_weak_profile_into)
    uint64_t weak_prefix = 0, weak_suffix = 0, weak_nosolid = 0;  // ... and the reads with a bad prefix / a bad suffix / no solid k-mer
    std::vector<rc_read_depth> depth;  // -depth-tags / -depth only: the corrected reads' k-mer depth, indexed like ret (rc_read_depth_into)
    std::vector<uint64_t> depth_hist[2];  // ... and per mate the reads by median (the last bin: -depth-max or more), all of its reads, those
    uint64_t depth_reads[2] = {0, 0}, depth_novalid[2] = {0, 0};  // without a valid window
    bool resident = false;        // the batch's reads are arenas the k-mer counter kept in HBM (rc_submit_resident)
    int arena_a = 0, arena_b = 0;
    int gpu = -1;                 // the GPU that holds them (-1: any GPU may take the batch)
    // -packed: the batch as rc_packed_batch wants it (one offset array over both arenas, 2-bit codes, quality bits, the
    // letters outside ACGT) and the room for the fix list
    PinBuf pk_bases, pk_exc_pos, pk_exc_chr;
    // offsets, quality bits and the room for the fix list: ONE page-locked allocation per job -- a registration costs
    // milliseconds to make and to undo (at exit, too) whatever its size, and four of them per job were 0.1 s of a 1.5 s run
    PinBuf pk_slab;
    struct PkView {
        uint32_t *off;
        uint8_t *qbits;
        uint32_t *fix_pos;
        uint8_t *fix_chr;
    };
    PkView pk_carve(size_t total_reads, size_t nbytes, size_t fix_cap)
    {
        auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t o_q = up((total_reads + 1) * 4), o_fp = o_q + up((nbytes + 7) / 8 + 64), o_fc = o_fp + up(fix_cap * 4), end = o_fc + up(fix_cap + 1);
        pk_slab.need(end);
        char *p = pk_slab.data();
        return PkView{(uint32_t *)p, (uint8_t *)(p + o_q), (uint32_t *)(p + o_fp), (uint8_t *)(p + o_fc)};
    }
    std::vector<OutBuf> o1, o2;  // the formatted (and, for .gz, deflated) output records, in slices
    uint64_t cor_bases = 0;  // sum of the positive return values (UpdateSummary, main.cpp:73-79), added up by the formatter
    bool done = false;
    int rc = 0;
    std::string err;
};

// Reads.h:224-266 for a whole block: sequence -> NUL-terminated arena, quality cut / padded to the
// sequence length for the kernels (the output prints the quality line verbatim, see put_record)
uint64_t index_arena(Arena &A, const std::string &path);
// the sequences alone, NUL-terminated, at dst (A.off must be set): what the k-mer counter is given
void pack_sequences(const Arena &A, char *dst);
void pack_arena(Arena &A, const std::string &path);

// Quality bits of a resident batch straight from the text: bit p of the batch's arena (arena 1's bytes, then arena 2's)
// = the quality character of that base is above the threshold; positions without one (the NUL behind a read, a
// quality line shorter than its sequence: pack_arena pads with 0) compare as 0.  [lo, hi) is a range of arena positions
// that starts and ends at multiples of 8 (or at the arena's end): ranges are packed side by side by different threads.
// Returns false if a read with bases has no first quality character (qual[0] == 0 asks for the byte path,
// ErrorCorrection.cpp:1316).
struct QualView {
    const Arena *A[2];
    size_t bytes1;
    size_t nbytes;
};
bool pack_quality_bits_from_text(const QualView &V, char bad_q, size_t lo, size_t hi, uint8_t *bits);
// The same bits from the byte arenas pack_arena made (a packed batch): same view, same ranges.  The arenas cannot say "no
// quality string" in one bit either; the caller has asked has_empty_quality_read() before.
void pack_quality_bits_from_arenas(const QualView &V, char bad_q, size_t lo, size_t hi, uint8_t *bits);
// The ranges both are called with: piece(lo, hi) over up to g_threads pieces of [0, nbytes) side by side on g_pool, one per
// `grain` bytes, cut at multiples of 8 so that no two pieces share a byte of the bit array.  False if a piece returned false.
template <class F>
inline bool for_quality_pieces(size_t nbytes, F piece, size_t grain = 65536)
{
    const size_t Q = std::max<size_t>(1, std::min<size_t>((size_t)g_threads, nbytes / grain + 1));
    std::vector<char> ok(Q, 1);
    g_pool.run(Q, [&](size_t t) {
        const size_t lo = (nbytes * t / Q) & ~(size_t)7, hi = t + 1 == Q ? nbytes : ((nbytes * (t + 1) / Q) & ~(size_t)7);
        if (lo < hi) ok[t] = piece(lo, hi) ? 1 : 0;
    });
    return std::find(ok.begin(), ok.end(), 0) == ok.end();
}
// a FASTQ batch (its byte arenas) with a read that has bases and no first quality character: see above
bool has_empty_quality_read(const Job &J);

// one offset array over both arenas, n + 1 or 2 n + 1 entries: arena 2's offsets follow arena 1's, moved up by its size
void combined_offsets(const Job &J, uint32_t *off);

// The bases of a packed batch (nbytes of byte arena, the first bytes1 of them arena 1's) into J.pk_bases, and the letters
// outside ACGT into J.pk_exc_pos / J.pk_exc_chr in ascending order; returns how many of those there are.  rc_pack_bases over
// up to g_threads 16-byte-aligned pieces of the combined arena side by side, one per 4096 words, each counting its exceptions
// before it stores them; the piece that holds the seam between the arenas packs either side of it in turn.
size_t pack_bases_of(Job &J, size_t nbytes, size_t bytes1);

// the substitutions of a resident batch, applied to the sequence lines of the text
void apply_fixes_to_text(Arena &A1, Arena *A2, size_t bytes1, const uint32_t *fix_pos, const uint8_t *fix_chr, size_t lo, size_t hi);
// a fix list (positions in the combined arena, distinct: any number of threads) applied where the batch's sequences are: the
// text's sequence lines (seq_in_text) or the byte arenas
void apply_fixes(Job &J, size_t bytes1, const uint32_t *fix_pos, const uint8_t *fix_chr, size_t n_fix);

static inline char *put_int(char *p, int v)
{
    char tmp[16];
    int n = 0;
    unsigned u = v < 0 ? 0u - (unsigned)v : (unsigned)v;
    do {
        tmp[n++] = (char)('0' + u % 10);
        u /= 10;
    } while (u);
    if (v < 0) *p++ = '-';
    while (n) *p++ = tmp[--n];
    return p;
}

// Reads.h:360-421: one record.  The quality line is printed as fgets left it in the reference:
// stripped of its newline only when it is exactly as long as the sequence line (Reads.h:255-262).
// wk (-weak-ends): the read's weak-k-mer profile -- the tags of the reference's dormant branch (Reads.h:396-412) follow " cor",
// each only where its value is above 0; the unfixable branch (:389) has none.  nullptr: the record as without the flag.
// dp (-depth-tags): the read's k-mer depth -- " kdepth=Q1:MED:Q3" last of all, on every record whose read has a valid window.
template <class B>
static inline void put_record(B &out, const Arena &A, size_t r, bool fastq, int cor, int l, int m, int h, const rc_read_weak *wk = nullptr,
                              const rc_read_depth *dp = nullptr)
{
    uint32_t il, ql = 0;
    const char *id = A.line(r, 0, &il);
    const char *seq = A.sequence(r);
    const uint32_t sl = A.off[r + 1] - A.off[r] - 1;
    const char *q = fastq ? A.line(r, 3, &ql) : nullptr;
    const size_t need = (size_t)il + sl + ql + 96 + (wk ? 48 : 0) + (dp ? 48 : 0);
    const size_t at = out.size();
    out.resize(at + need);
    char *p = out.data() + at;
    memcpy(p, id, il);
    p += il;
    memcpy(p, " l:", 3);
    p = put_int(p + 3, l);
    memcpy(p, " m:", 3);
    p = put_int(p + 3, m);
    memcpy(p, " h:", 3);
    p = put_int(p + 3, h);
    if (cor == -1) {
        memcpy(p, " unfixable_error", 16);
        p += 16;
    } else if (cor > 0) {
        memcpy(p, " cor", 4);
        p += 4;
    }
    if (wk && cor != -1) {
        if (wk->bad_prefix > 0) {
            memcpy(p, " bad_prefix=", 12);
            p = put_int(p + 12, wk->bad_prefix);
        }
        if (wk->bad_suffix > 0) {
            memcpy(p, " bad_suffix=", 12);
            p = put_int(p + 12, wk->bad_suffix);
        }
    }
    if (dp && dp->valid > 0) {
        memcpy(p, " kdepth=", 8);
        p = put_int(p + 8, dp->q1);
        *p++ = ':';
        p = put_int(p, dp->median);
        *p++ = ':';
        p = put_int(p, dp->q3);
    }
    *p++ = '\n';
    memcpy(p, seq, sl);
    p += sl;
    *p++ = '\n';
    if (fastq) {
        *p++ = '+';
        *p++ = '\n';
        memcpy(p, q, ql);
        p += ql;
        // fgets kept the quality line's own newline (Reads.h strips it only at index strlen(seq)) --
        // unless this is the last line of a file that does not end with one
        if (ql != sl && !(A.blk.unterminated_last && r + 1 == A.n())) *p++ = '\n';
        *p++ = '\n';
    }
    out.resize((size_t)(p - out.data()));
}

// what the reference prints to stdout for one read under -verbose (ErrorCorrection.cpp:686-689,
// 759-770,856-857,1088-1094 and GetKmerInformation :1590-1597), from the data
// rc_correct_batch_traced returns.  gi = the read's index in ret/l/m/h order, ab = offset of its
// arena in the batch's device arena (0, or the size of arena 1 for second mates)
void put_transcript(std::vector<char> &out, const Job &J, const Arena &A, size_t r, size_t gi, size_t ab, int k);

// a k-mer count spectrum as `jellyfish histo` prints it: "<count> <frequency>\n" per non-zero bin, ascending; false: not written
bool write_histo(const char *path, const std::vector<uint64_t> &freq);
// the correction report (rcorrector_amd.h: rc_change_report) as tab-separated text, one fact per line, the first field naming
// the section; mates are written 1 and 2 (mate 2 only with two_mates), positions count from 1:
//   reads <mate> <reads> <with changes> <unfixable> / changes <mate> <count> / pos5 <mate> <position> <changes> <reads covering it>
//   and pos3 <mate> <distance from the last base, 1 = the last base> <changes>, a line per position up to the mate's longest
//   read / subst <A|C|G|T|N> <A|C|G|T> <count>, all 20 / qual <low|high|none> <count> / perread <n | 64+> <reads>, non-zero ones
bool write_change_report(const char *path, const rc_change_report &R, bool two_mates);
// the duplicate census (rcorrector_amd.h: rc_dup_census, binned to max_bin) as tab-separated text: units <n> <unit> / distinct
// before <n> / distinct after <n> / copies <c> <distinct before> <distinct after>, a line per c where either is non-zero (the
// line of c = max_bin: that many copies or more)
bool write_dup_census(const char *path, const rc_dup_census &D, uint32_t max_bin, const char *unit);
// the recurrence census (rcorrector_amd.h: rc_recur_census, binned to max_bin, its top list taken at min_count) as tab-separated
// text: flank 14 / min_count <n> / changes <n> / contexted <n> / clipped <n> / sites <n> / recur <c> <sites>, a line per c
// that occurs (the line of c = max_bin: that many changes or more) / site <count> <from A|C|G|T|N> <to> <29-mer>, the top
// sites in the library's order (the canonical window: <to> is its centre)
bool write_recur_census(const char *path, const rc_recur_census &R, uint32_t max_bin, uint32_t min_count);
// the trust profile by read position (rcorrector_amd.h: rc_trust_profile) as tab-separated text: k <k> / min_count <n> / reads
// <mate 1|2> <n> / total <before|after> <mate> <windows> <solid> <weak> <invalid> / pos5 and pos3 <before|after> <mate> <p>
// <windows> <solid> <weak> <invalid>, a line per position p that some read has a window at; mate 2 only with two_mates.
// add_trust_profile: to += from, every count (what several GPUs' profiles become one with)
bool write_trust_profile(const char *path, const rc_trust_profile &T, bool two_mates);
void add_trust_profile(rc_trust_profile &to, const rc_trust_profile &from);
// the mate-overlap report (rcorrector_amd.h: rc_mate_overlap) as tab-separated text: min_overlap <n> / max_mismatch_pct <n> /
// pairs <n> / overlapping <n> / compared <before|after> <n> / disagree <before|after> <n> / resolved <n> / kept <n> / introduced
// <n> / pairs <improved|worsened|same> <n> / frag <F> <pairs>, a line per non-zero F / pos5 <mate 1|2> <p> <compared> <disagree
// before> <disagree after>, a line per position p (from 0, from that mate's 5' end) with compared > 0.
// add_mate_overlap: to += from, every count (what several GPUs' reports become one with; the two parameters stay to's)
std::string mate_overlap_text(const rc_mate_overlap &M);
bool write_mate_overlap(const char *path, const rc_mate_overlap &M);
void add_mate_overlap(rc_mate_overlap &to, const rc_mate_overlap &from);
// the k-mer depth report (rcorrector_amd.h: rc_read_depth, the corrected reads' medians) as tab-separated text: k <k> / reads
// <mate 1|2> <n> / novalid <mate> <n> (reads without a valid k-mer window: they have no median) / median <d> <reads of mate 1>
// [<reads of mate 2>], a line per d that some read has; the line of d = hist[m].size() - 1: that or more.  Mate 2 only with two_mates.
// depth_median_of_medians: the lower median of the reads' medians over both mates (bin index; the last bin: that or more), 0 of none
bool write_depth_report(const char *path, int k, const uint64_t reads[2], const uint64_t novalid[2], const std::vector<uint64_t> hist[2], bool two_mates);
size_t depth_median_of_medians(const std::vector<uint64_t> hist[2]);
// GetBadQuality's two histograms over the records of one block (main.cpp:88-128), at most `room` of them
void quality_histograms(const Block &b, int lpr, size_t room, std::vector<int32_t> &fh, std::vector<int32_t> &lh, int *total);

// one gzip member (RFC 1952) holding `in`, deflate level 1
void gzip_member(const OutBuf &in, OutBuf &out);
