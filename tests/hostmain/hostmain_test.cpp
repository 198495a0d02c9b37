// The host-side arithmetic of rcorrector's batches (rc_format.cpp, rc_reader.cpp) checked without a GPU, on ragged, empty and over-long
// quality lines, Ns, single and paired arenas.  Per seed, a job whose sequences are in the text (a resident batch's) beside its
// twin through pack_arena (byte arenas: the reference):
//   quality bits   pack_quality_bits_from_text (SSE compares, bit streams cut at byte-aligned piece boundaries) and
//                  pack_quality_bits_from_arenas, each through for_quality_pieces, against rc_pack_quality_bits over the
//                  concatenated byte arenas
//   offsets        combined_offsets against the concatenation made by hand
//   bases          pack_bases_of (pieces, the seam between the arenas inside one, exceptions counted and then stored) against
//                  rc_pack_bases over the concatenated byte arenas, at one piece and at several
//   fixes          apply_fixes_to_text and apply_fixes on the text against the same fixes on the byte arenas, by hand and by apply_fixes
// Test infrastructure: links the CLI's host units (rc_pool, rc_reader, rc_format) through their headers.
#include <unistd.h>

#include "../../rcorrector_amd/csrc/rc_dispatch.h"
#include <random>

static int fail(const char *what, unsigned seed)
{
    printf("FAIL %s (seed %u)\n", what, seed);
    return 1;
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : "/tmp";
    g_threads = 4;
    g_pool.start(8);
    size_t seam_inside_a_word = 0, several_pieces = 0;
    for (unsigned seed = 1; seed <= 60; ++seed) {
        std::mt19937 rng(seed);
        const bool uniform = seed % 3 == 0;
        const bool big = seed % 7 == 0;     // arenas of several of pack_bases_of's pieces (one per 4096 words of 16 bases)
        const bool n_seam = seed == 20;     // arena 1 ends in, arena 2 begins with, a read of Ns: exceptions on both sides of the seam
        const int n = (1 + (int)(rng() % 700)) * (big ? 8 : 1), L0 = 1 + (int)(rng() % 200);
        std::string paths[2] = {dir + "/hm_1.fq", dir + "/hm_2.fq"};
        for (int sd = 0; sd < 2; ++sd) {
            FILE *f = fopen(paths[sd].c_str(), "wb");
            for (int r = 0; r < n; ++r) {
                const int sl = uniform ? L0 : (int)(rng() % (unsigned)(L0 + 1));
                int ql = sl;
                const unsigned u = rng() % 10;
                if (!uniform && u == 0) ql = sl ? (int)(rng() % (unsigned)sl) : 0;  // short (or empty) quality line
                if (!uniform && u == 1) ql = sl + 1 + (int)(rng() % 5);            // long one
                std::string s(sl, 'A'), q(ql, 'I');
                for (auto &c : s) c = "ACGTN"[rng() % 5];
                for (auto &c : q) c = (char)(33 + rng() % 60);
                if (n_seam && r == (sd ? 0 : n - 1)) s.assign(37, 'N');
                fprintf(f, "@r%d\n%s\n+\n%s\n", r, s.c_str(), q.c_str());
            }
            fclose(f);
        }
        const bool paired = seed % 2 == 0;
        Job T, Y;  // T: the sequences in the text; Y: the same blocks through pack_arena, byte arenas (the reference for every check)
        Arena *A[2] = {&T.a, &T.b}, *B[2] = {&Y.a, &Y.b};
        T.mode = Y.mode = paired ? 1 : 0;
        for (int sd = 0; sd < 2; ++sd) {
            Source s;
            s.open(paths[sd]);
            A[sd]->lpr = 4;
            take_records(s, (size_t)n, 4, A[sd]->blk);
            s.close();
            if ((int)A[sd]->blk.records != n) return fail("records", seed);
        }
        for (int sd = 0; sd < 2; ++sd) {
            B[sd]->lpr = 4;
            B[sd]->blk.text.need(A[sd]->blk.text.cap);
            memcpy(B[sd]->blk.text.p, A[sd]->blk.text.p, A[sd]->blk.text.cap);
            B[sd]->blk.line = A[sd]->blk.line;
            B[sd]->blk.records = A[sd]->blk.records;
            pack_arena(*B[sd], paths[sd]);
            index_arena(*A[sd], paths[sd]);
            A[sd]->seq_in_text = true;
        }
        const size_t bytes1 = A[0]->off[n], bytes2 = paired ? A[1]->off[n] : 0, nbytes = bytes1 + bytes2;
        if (paired && bytes1 % 16) ++seam_inside_a_word;
        if (n_seam && !(paired && bytes1 % 16)) return fail("the seam seed's seam is not inside a word", seed);
        const char bad_q = (char)(33 + rng() % 60);
        // reference bits: rc_pack_quality_bits over the concatenated byte arenas
        std::vector<char> qcat(nbytes), scat(nbytes);
        memcpy(qcat.data(), B[0]->qual.data(), bytes1);
        memcpy(scat.data(), B[0]->seq.data(), bytes1);
        if (paired) memcpy(qcat.data() + bytes1, B[1]->qual.data(), bytes2);
        if (paired) memcpy(scat.data() + bytes1, B[1]->seq.data(), bytes2);
        std::vector<uint8_t> want((nbytes + 7) / 8 + 8, 0), got((nbytes + 7) / 8 + 8, 0), got2((nbytes + 7) / 8 + 8, 0);
        rc_pack_quality_bits(qcat.data(), nbytes, bad_q, want.data());
        QualView V{{A[0], paired ? A[1] : A[0]}, paired ? bytes1 : nbytes, nbytes}, W{{B[0], paired ? B[1] : B[0]}, bytes1, nbytes};
        // one to seven pieces, whatever the arena's size: a piece per eighth of it, as many as there are threads
        g_threads = 1 + (int)(rng() % 7);
        const size_t grain = nbytes / 8 + 1;
        const bool ok = for_quality_pieces(nbytes, [&](size_t lo, size_t hi) { return pack_quality_bits_from_text(V, bad_q, lo, hi, got.data()); }, grain);
        bool expect_ok = true;
        for (int sd = 0; sd < (paired ? 2 : 1); ++sd)
            for (int r = 0; r < n; ++r)
                if (B[sd]->off[r + 1] - B[sd]->off[r] > 1 && B[sd]->qual.data()[B[sd]->off[r]] == 0) expect_ok = false;
        if (ok != expect_ok) return fail("empty-quality flag", seed);
        if (has_empty_quality_read(Y) == expect_ok) return fail("empty-quality read in the byte arenas", seed);
        if (memcmp(want.data(), got.data(), (nbytes + 7) / 8) != 0) return fail("quality bits", seed);
        for_quality_pieces(nbytes, [&](size_t lo, size_t hi) {
            pack_quality_bits_from_arenas(W, bad_q, lo, hi, got2.data());
            return true;
        }, grain);
        if (memcmp(want.data(), got2.data(), (nbytes + 7) / 8) != 0) return fail("quality bits from the byte arenas", seed);
        // offsets
        std::vector<uint32_t> off((size_t)(paired ? 2 * n : n) + 1, 0xffffffffu);
        combined_offsets(Y, off.data());
        for (int r = 0; r <= n; ++r)
            if (off[(size_t)r] != B[0]->off[r] || (paired && off[(size_t)(n + r)] != bytes1 + B[1]->off[r])) return fail("combined offsets", seed);
        // bases: at one piece, and at as many as the arena's size and the threads give
        const size_t n_words = (nbytes + 15) / 16;
        std::vector<uint32_t> wb(n_words + 16, 0), wp(nbytes + 1);
        std::vector<uint8_t> wc(nbytes + 1);
        const size_t want_exc = rc_pack_bases(scat.data(), 0, nbytes, wb.data(), wp.data(), wc.data(), nbytes);
        const int threads = g_threads;
        for (int pass = 0; pass < 2; ++pass) {
            g_threads = pass ? threads : 1;
            if (Y.pk_bases.p) memset(Y.pk_bases.p, 0xA5, Y.pk_bases.cap);
            const size_t n_exc = pack_bases_of(Y, nbytes, bytes1);
            if (n_exc != want_exc) return fail("packed bases: number of exceptions", seed);
            if (memcmp(Y.pk_bases.data(), wb.data(), n_words * 4) != 0) return fail("packed bases: words", seed);
            if (memcmp(Y.pk_exc_pos.data(), wp.data(), n_exc * 4) != 0) return fail("packed bases: exception positions", seed);
            if (memcmp(Y.pk_exc_chr.data(), wc.data(), n_exc) != 0) return fail("packed bases: exception letters", seed);
            for (size_t i = 1; i < n_exc; ++i)
                if (wp[i] <= wp[i - 1]) return fail("packed bases: positions not ascending", seed);
            if (pass && g_threads >= 2 && n_words >= 2 * 4096) ++several_pieces;
        }
        if (n_seam && !(scat[bytes1 - 2] == 'N' && scat[bytes1] == 'N')) return fail("the seam seed's Ns", seed);
        g_threads = 4;
        // fixes: random positions that hold a base, new letters
        std::vector<uint32_t> pos;
        std::vector<uint8_t> chr;
        for (size_t p = 0; p < nbytes; ++p) {
            if (scat[p] != 0 && rng() % 50 == 0) {
                pos.push_back((uint32_t)p);
                chr.push_back((uint8_t)"ACGT"[rng() % 4]);
            }
        }
        for (size_t i = 0; i < pos.size(); ++i) {
            if (pos[i] < bytes1)
                B[0]->seq.data()[pos[i]] = (char)chr[i];
            else
                B[1]->seq.data()[pos[i] - bytes1] = (char)chr[i];
        }
        const size_t F = 1 + rng() % 3;
        for (size_t t = 0; t < F; ++t)
            apply_fixes_to_text(*A[0], paired ? A[1] : nullptr, bytes1, pos.data(), chr.data(), pos.size() * t / F, pos.size() * (t + 1) / F);
        auto same_sequences = [&]() {
            for (int sd = 0; sd < (paired ? 2 : 1); ++sd)
                for (int r = 0; r < n; ++r) {
                    const uint32_t sl = A[sd]->off[r + 1] - A[sd]->off[r] - 1;
                    if (memcmp(A[sd]->sequence((size_t)r), B[sd]->sequence((size_t)r), sl) != 0) return false;
                }
            return true;
        };
        if (!same_sequences()) return fail("fixes applied to the text", seed);
        // a second list, at the same positions, through apply_fixes on the job in the text and on its byte-arena twin
        for (auto &c : chr) c = (uint8_t)"ACGT"[rng() % 4];
        apply_fixes(T, bytes1, pos.data(), chr.data(), pos.size());
        apply_fixes(Y, bytes1, pos.data(), chr.data(), pos.size());
        for (size_t i = 0; i < pos.size(); ++i)
            if ((pos[i] < bytes1 ? B[0]->seq.data()[pos[i]] : B[1]->seq.data()[pos[i] - bytes1]) != (char)chr[i]) return fail("apply_fixes on the byte arenas", seed);
        if (!same_sequences()) return fail("apply_fixes: text against byte arenas", seed);
    }
    if (!seam_inside_a_word) return fail("no seed with the seam between the arenas inside a word", 0);
    if (!several_pieces) return fail("no seed whose bases were packed in several pieces", 0);
    {   // a file of several read slices (the reader cuts a request into 8 MB slices read side by side, each a megabyte at a
        // time with its newlines found on the way): the blocks, put end to end, are the file, and the line index is exact
        const std::string big = dir + "/hm_big.fq";
        std::mt19937 rng(99);
        std::string content;
        const int n = 260000;
        for (int r = 0; r < n; ++r) {
            const int sl = 40 + (int)(rng() % 120);
            std::string sq(sl, 'A'), q(sl, 'I');
            for (auto &c : sq) c = "ACGT"[rng() % 4];
            content += "@big" + std::to_string(r) + "\n" + sq + "\n+\n" + q + "\n";
        }
        FILE *f = fopen(big.c_str(), "wb");
        fwrite(content.data(), 1, content.size(), f);
        fclose(f);
        Source s;
        s.open(big);
        Block b;
        size_t at = 0, recs = 0;
        for (int round = 0;; ++round) {
            take_records(s, round % 2 ? 90000 : 50001, 4, b);
            if (b.records == 0) break;
            const size_t nl = b.records * 4, end = b.line[nl];
            if (at + end > content.size() || memcmp(b.text.p, content.data() + at, end) != 0) return fail("big file: block bytes", (unsigned)round);
            for (size_t i = 0; i < nl; ++i) {
                if (b.text.p[b.line[i + 1] - 1] != '\n') return fail("big file: line end", (unsigned)round);
                if (memchr(b.text.p + b.line[i], '\n', b.line[i + 1] - 1 - b.line[i])) return fail("big file: newline inside a line", (unsigned)round);
            }
            at += end;
            recs += b.records;
        }
        s.close();
        if (at != content.size() || recs != (size_t)n) return fail("big file: size", 0);
        unlink(big.c_str());
    }
    {   // the one-pass reader that runs ahead of the GPU runtime (Ingest::start): stopped with blocks in its queue (abort), the
        // sources rewound as rcorrector's main does, started again and drained by hand -- both mates' blocks, put end to end,
        // are the files, whole pairs per block, in order (no GPU: consume() is not called)
        Run run;
        std::string content[2];
        const int n = 70001;
        std::mt19937 rng(7);
        for (int sd = 0; sd < 2; ++sd) {
            for (int r = 0; r < n; ++r) {
                const int sl = 30 + (int)(rng() % 100);
                std::string sq(sl, 'A'), q(sl, 'I');
                for (auto &c : sq) c = "ACGT"[rng() % 4];
                content[sd] += "@p" + std::to_string(r) + "/" + std::to_string(sd + 1) + "\n" + sq + "\n+\n" + q + "\n";
            }
            FILE *f = fopen((dir + (sd ? "/ra_2.fq" : "/ra_1.fq")).c_str(), "wb");
            fwrite(content[sd].data(), 1, content[sd].size(), f);
            fclose(f);
        }
        run.files.emplace_back();
        run.mates.emplace_back();
        open_file(run.files.back(), (dir + "/ra_1.fq").c_str(), true, false, dir);
        open_file(run.mates.back(), (dir + "/ra_2.fq").c_str(), true, false, dir);
        for (int attempt = 0; attempt < 2; ++attempt) {
            Ingest I(run, 9000, true);
            I.depth = attempt ? 3 : 4;
            I.start();
            if (attempt == 0) {
                for (;;) {  // let it get ahead, then change our mind
                    std::unique_lock<std::mutex> lk(I.mu);
                    if (I.q.size() >= 3 || I.done) break;
                    lk.unlock();
                    usleep(1000);
                }
                I.abort();
                if (!I.q.empty()) return fail("read-ahead: blocks left after abort", 0);
                for (ReadFile *f : {&run.files[0], &run.mates[0]}) {
                    f->src.rewind();
                    f->src.left.need(4096);
                    f->src.left_len = f->src.fill(f->src.left.p, 4096);
                }
                continue;
            }
            size_t at[2] = {0, 0}, recs = 0;
            for (;;) {
                std::unique_ptr<Retained> B;
                {
                    std::unique_lock<std::mutex> lk(I.mu);
                    I.cv.wait(lk, [&] { return I.done || !I.q.empty(); });
                    if (I.q.empty()) break;
                    B = std::move(I.q.front());
                    I.q.pop_front();
                    I.cv.notify_all();
                }
                if (B->a.records != B->b.records || B->mode != 1) return fail("read-ahead: pairs", (unsigned)recs);
                for (int sd = 0; sd < 2; ++sd) {
                    const Block &b = sd ? B->b : B->a;
                    const size_t end = b.line[b.records * 4];
                    if (at[sd] + end > content[sd].size() || memcmp(b.text.p, content[sd].data() + at[sd], end) != 0) return fail("read-ahead: block bytes", (unsigned)recs);
                    at[sd] += end;
                }
                recs += B->a.records;
            }
            I.reader.join();
            if (recs != (size_t)n || at[0] != content[0].size() || at[1] != content[1].size()) return fail("read-ahead: size", 0);
        }
        for (const char *f : {"/ra_1.fq", "/ra_2.fq", "/ra_1.cor.fq", "/ra_2.cor.fq"}) unlink((dir + f).c_str());
    }
    printf("ok 60 cases\n");
    fflush(stdout);
    _exit(0);
}
