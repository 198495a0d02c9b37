// rc_dispatch.cpp -- see rc_dispatch.h
#include "rc_dispatch.h"

#include <sys/stat.h>
#include <unistd.h>

// room for the substitutions of a batch of nbytes arena bytes: one per sixteen bases (0.5 % errors fill a twelfth of it, 5 %
// two thirds; the reference's bound, MAX_FIX_PER_K per k-mer window and more with -maxcorK, is about a third of the bases: a
// batch that needs more comes back with RC_STATUS_NOSPACE and is run again through the byte path).  The list is page-locked,
// and page-locking touches every page whether a fix ever lands there or not: at one entry per four bases it was 190 MB per
// job of a million 150-base reads, most of what a run locks and unlocks.  RC_FIX_CAP=<entries>: tests.
static size_t fix_list_room(size_t nbytes)
{
    static const char *e = getenv("RC_FIX_CAP");
    return e ? (size_t)atoll(e) : nbytes / 16 + 64;
}

// how a file is cut into batches: 0 single, 1 paired with `mate` (null otherwise), 2 interleaved; lines per record of either side
struct BatchShape {
    int mode, lpr_a, lpr_b;
};
static BatchShape batch_shape(const ReadFile &f, const ReadFile *mate)
{
    const int lpr = f.fastq ? 4 : 2;
    return BatchShape{f.paired ? 1 : (f.interleaved ? 2 : 0), lpr, mate ? (mate->fastq ? 4 : 2) : lpr};
}

// Up to `want` records of f from src_a into A and, for a pair, as many of its mate's from src_b into B on a second thread (two
// inflate streams run side by side for .gz pairs).  False: the input has ended.  refuse: mates' files of different lengths and
// an interleaved file with an odd number of reads end the run.
static bool take_batch(const ReadFile &f, Source &src_a, Source *src_b, const BatchShape &S, size_t want, Block &A, Block &B, bool refuse)
{
    const double tr0 = now_s();
    B.records = 0;
    if (src_b) {
        std::thread mate([&]() { take_records(*src_b, want, S.lpr_b, B); });
        take_records(src_a, want, S.lpr_a, A);
        mate.join();
        if (refuse && B.records != A.records) die("ERROR: The files are not paired!\n");
    } else {
        take_records(src_a, want, S.lpr_a, A);
    }
    if (A.records == 0 && B.records == 0) return false;
    if (refuse && S.mode == 2 && (A.records & 1)) die("ERROR: interleaved file %s holds an odd number of reads\n", f.path.c_str());
    g_t_read += now_s() - tr0;
    return true;
}

// the reader of the one-pass ingest: host memory only (text blocks and their line index), so that it can run while the GPU
// runtime is still starting up
void Ingest::start()
{
    reader = std::thread([this]() {
        for (size_t fi = 0; fi < R.files.size() && !stop; ++fi) {
            ReadFile &f = R.files[fi];
            ReadFile *mate = f.paired ? &R.mates[fi] : nullptr;
            const BatchShape S = batch_shape(f, mate);
            Source own_a, own_b;
            if (!keep) {
                own_a.open(f.path);
                if (mate) own_b.open(mate->path);
            }
            Source &src_a = keep ? f.src : own_a, *src_b = !mate ? nullptr : keep ? &mate->src : &own_b;
            while (!stop) {
                std::unique_ptr<Retained> B;
                {
                    std::lock_guard<std::mutex> lk(mu);
                    if (!spare.empty()) {
                        B = std::move(spare.back());
                        spare.pop_back();
                    }
                }
                if (!B) B.reset(new Retained);
                B->file = (int)fi;
                B->mode = S.mode;
                B->fastq = f.fastq;
                B->lpr_a = S.lpr_a;
                B->lpr_b = S.lpr_b;
                // (two passes: files that are not paired are the correction loop's to refuse, with the reference's message
                // in the reference's place on stderr; the counter takes whatever reads there are)
                if (!take_batch(f, src_a, src_b, S, batch_reads, B->a, B->b, keep)) break;
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || q.size() < depth; });
                q.emplace_back(std::move(B));
                cv.notify_all();
            }
            if (!keep) {
                own_a.close();
                if (mate) own_b.close();
            }
        }
        std::lock_guard<std::mutex> lk(mu);
        done = true;
        cv.notify_all();
    });
}

// a reader that ran ahead of a decision that then went the other way (Ingest::depth blocks at most): its blocks are dropped; the
// caller rewinds the sources
void Ingest::abort()
{
    {
        std::lock_guard<std::mutex> lk(mu);
        stop = true;
    }
    cv.notify_all();
    reader.join();
    q.clear();
}

void Ingest::consume(int64_t *stored)
{
    rc_ctx *ctx = R.ctx[0];
    {
        std::lock_guard<std::mutex> lk(mu);
        depth = 3;  // (a reader that ran ahead may hold more)
    }
    if (rc_table_count_keep(ctx, keep ? 1 : 0) || rc_table_count_begin(ctx)) die("rcorrector: %s\n", rc_last_error(ctx));
    // Several GPUs, one pass: the batches are dealt round-robin, each arena uploaded to the GPU that will correct it, and the
    // GPUs count together (rc_table_count_finish_sharded: every GPU scans its own reads, the key space is shared out; one
    // Store for all workers, main.cpp:294-308): the files are read once, and a batch is corrected where its bases already
    // are.  RC_COUNT_SHARDED=0: every arena goes to GPU 0 as well, which counts alone (the others rc_table_count_park).
    const int n_gpus = keep ? R.gpus : 1;
    const bool sharded = n_gpus > 1 && !(getenv("RC_COUNT_SHARDED") && !strcmp(getenv("RC_COUNT_SHARDED"), "0"));
    for (int g = 1; g < n_gpus; ++g)
        if (rc_table_count_begin(R.ctx[(size_t)g])) die("rcorrector: %s\n", rc_last_error(R.ctx[(size_t)g]));
    PinBuf stage;  // the sequences of one file's share of a batch on their way to HBM
    std::vector<int> next_arena((size_t)n_gpus, 0);
    size_t n_batches = 0;
    for (;;) {
        std::unique_ptr<Retained> B;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return done || !q.empty(); });
            if (q.empty()) break;
            B = std::move(q.front());
            q.pop_front();
            cv.notify_all();
        }
        const double tp0 = now_s();
        B->gpu = (int)(n_batches++ % (size_t)n_gpus);
        for (int sd = 0; sd < (B->mode == 1 ? 2 : 1); ++sd) {
            if ((sd ? B->b : B->a).records == 0) continue;  // (keep = false: one mate's file ended before the other's)
            Arena A;  // (a view for index_arena / pack_sequences: the block is swapped in and out)
            A.lpr = sd ? B->lpr_b : B->lpr_a;
            A.blk.swap(sd ? B->b : B->a);
            A.off.swap(sd ? B->off_b : B->off_a);  // (its capacity, when the block is a recycled one)
            const uint64_t total = index_arena(A, sd ? R.mates[(size_t)B->file].path : R.files[(size_t)B->file].path);
            stage.need(total + 64);
            pack_sequences(A, stage.data());
            // (an arena without a byte is not kept: cannot happen, every record has at least its NUL)
            int idx;
            if (sharded) {  // to the GPU that will correct it, and nowhere else
                rc_ctx *cg = R.ctx[(size_t)B->gpu];
                if (rc_table_count_add(cg, stage.data(), total)) die("rcorrector: %s\n", rc_last_error(cg));
                idx = next_arena[(size_t)B->gpu]++;
            } else {
                if (rc_table_count_add(ctx, stage.data(), total)) die("rcorrector: %s\n", rc_last_error(ctx));
                idx = next_arena[0]++;
                if (B->gpu != 0) {
                    rc_ctx *cg = R.ctx[(size_t)B->gpu];
                    if (rc_table_count_add(cg, stage.data(), total)) die("rcorrector: %s\n", rc_last_error(cg));
                    idx = next_arena[(size_t)B->gpu]++;
                }
            }
            (sd ? B->arena_b : B->arena_a) = idx;
            (sd ? B->off_b : B->off_a).swap(A.off);
            A.blk.swap(sd ? B->b : B->a);
        }
        g_t_pack += now_s() - tp0;
        if (keep) {
            R.kept.emplace_back(std::move(B));
        } else {
            std::lock_guard<std::mutex> lk(mu);
            spare.emplace_back(std::move(B));
        }
    }
    reader.join();
    stamp(keep ? "inputs read, indexed and uploaded" : "inputs read and uploaded for the k-mer count");
    if (sharded) {
        if (rc_table_count_finish_sharded(R.ctx.data(), n_gpus, 2, stored)) die("rcorrector: %s\n", rc_last_error(ctx));
    } else {
        for (int g = 1; g < n_gpus; ++g)
            if (rc_table_count_park(R.ctx[(size_t)g])) die("rcorrector: %s\n", rc_last_error(R.ctx[(size_t)g]));
        if (rc_table_count_finish(ctx, 2, stored)) die("rcorrector: %s\n", rc_last_error(ctx));
    }
    stamp("k-mers counted, table built");
}

void ingest_resident(Run &R, size_t batch_reads, int64_t *stored, bool keep)
{
    Ingest I(R, batch_reads, keep);
    I.start();
    I.consume(stored);
}

// the head of the first input is what the buffers are sized from: a plain seekable file, no -verbose
static bool head_is_usable(const Run &R) { return !R.files.empty() && !g_verbose && !R.files[0].src.is_gz && R.files[0].src.seekable; }

HeadStats head_stats(const Run &R)
{
    HeadStats H;
    if (!head_is_usable(R)) return H;
    const ReadFile &f = R.files[0];
    const size_t lpr = f.fastq ? 4 : 2;
    const char *h = f.src.left.p;
    size_t l1 = 0;
    for (size_t i = 0; i < f.src.left_len; ++i)
        if (h[i] == '\n') {
            ++H.nl;
            if (H.nl == 1) l1 = i;
            if (H.nl == 2) H.seq_len = i - l1 - 1;
            if (H.nl % lpr == 0) H.last = i + 1;
        }
    return H;
}

void warm_buffers(Run &R, const HeadStats &H)
{
    if (!head_is_usable(R) || H.last == 0 || H.seq_len == 0) return;
    const ReadFile &f = R.files[0];
    const int lpr = f.fastq ? 4 : 2;
    const double rec_bytes = (double)H.last / (double)(H.nl / (size_t)lpr);
    struct stat st;
    if (stat(f.path.c_str(), &st) != 0) return;
    const double file_recs = (double)st.st_size / rec_bytes;
    size_t recs = R.batch_reads;  // (a batch of an interleaved file holds batch_reads records as well)
    if ((double)recs > file_recs * 1.02 + 16) recs = (size_t)(file_recs * 1.02) + 16;
    const size_t njobs = std::min((size_t)(file_recs / (double)recs) + 1, R.max_in_flight);
    const size_t text_bytes = (size_t)((double)recs * rec_bytes * 1.04) + ((size_t)1 << 20);
    const size_t arena_bytes = (size_t)((double)recs * (double)(H.seq_len + 1) * 1.02) + 4096;
    const size_t S = std::max<size_t>(1, std::min<size_t>((size_t)g_threads, (recs + 8191) / 8192));
    const size_t out_slice = (size_t)(((double)recs / (double)S + 1.0) * (rec_bytes + 48.0));
    for (size_t jn = 0; jn < njobs; ++jn) {
        auto j = std::make_shared<Job>();
        const int sides = f.paired ? 2 : 1;
        for (int sd = 0; sd < sides; ++sd) {
            Arena &A = sd ? j->b : j->a;
            if (!R.resident) {
                A.blk.text.need(text_bytes);
                A.blk.line.reserve(recs * (size_t)lpr + 8);
                A.off.reserve(recs + 1);
                A.seq.need(arena_bytes);   // (page-locked here: rc_host_register)
                A.qual.need(arena_bytes);
            }
            std::vector<OutBuf> &o = sd ? j->o2 : j->o1;
            o.resize(S);
            for (auto &v : o) v.reserve(out_slice);
        }
        // touch what malloc handed out untouched (the arenas were touched by the registration)
        g_pool.run(16, [&](size_t t) {
            for (int sd = 0; sd < sides; ++sd) {
                Arena &A = sd ? j->b : j->a;
                const size_t lo = text_bytes * t / 16, hi = text_bytes * (t + 1) / 16;
                if (!R.resident) memset(A.blk.text.p + lo, 0, hi - lo);
                std::vector<OutBuf> &o = sd ? j->o2 : j->o1;
                for (size_t s2 = t; s2 < S; s2 += 16) {
                    o[s2].resize(out_slice);
                    memset(o[s2].data(), 0, out_slice);
                    o[s2].clear();
                }
            }
        });
        const size_t total = (size_t)sides * recs;
        if (R.resident) {  // what a resident batch sends and receives (page-locked)
            const size_t nb = (size_t)sides * arena_bytes;
            (void)j->pk_carve(total, nb, fix_list_room(nb));
        }
        j->ret.reserve(total);
        j->l.reserve(total);
        j->m.reserve(total);
        j->h.reserve(total);
        R.warm_jobs.push_back(j);
    }
}

// the output records of a finished batch, formatted (and deflated for .gz outputs) in slices by
// the worker that ran it; the writer thread only writes
static void format_job(Run &R, Job &J)
{
    const size_t n = J.a.n();
    const bool alternate = J.mode == 1 && g_stdout;  // main.cpp:487-495
    // compression is a property of each output file (Reads::AddReadFile picks it per input name):
    // `-p a.fq.gz b.fq` writes a gzip stream for the first mates and plain text for the second
    const bool gz1 = R.files[(size_t)J.file].out_gz && !g_stdout, gz2 = J.mode == 1 && R.mates[(size_t)J.file].out_gz && !g_stdout;
    // (slices of plain output are copied by at most g_threads threads -- memory-bound, more get in each other's way --
    // slices that are deflated by as many as the pool has: that is arithmetic)
    const size_t width = (gz1 || gz2) ? std::max<size_t>((size_t)g_threads, g_deflate_threads) : (size_t)g_threads;
    const size_t S = std::max<size_t>(1, std::min<size_t>(width, (n + 8191) / 8192));
    J.o1.resize(S);
    J.o2.resize(S);
    for (auto &v : J.o1) v.clear();
    for (auto &v : J.o2) v.clear();
    std::vector<uint64_t> cor(S, 0);  // (the writer thread is the pipeline's narrow place: it only writes)
    const rc_read_weak *wk = R.weak_ends ? J.weak.data() : nullptr;  // -weak-ends: the tags, and the reads that have them
    const size_t WS = wk ? S : 0;
    std::vector<uint64_t> wpre(WS, 0), wsuf(WS, 0), wnone(WS, 0);
    auto tally = [&](size_t s, const Arena &A, size_t r, size_t gi) {
        const int32_t L = (int32_t)(A.off[r + 1] - A.off[r]) - 1;
        wpre[s] += wk[gi].bad_prefix > 0;
        wsuf[s] += wk[gi].bad_suffix > 0;
        wnone[s] += L > 0 && wk[gi].uncovered == L;
    };
    // -depth-tags / -depth: the reads of either mate (mode 2: the odd reads are the second mates) without a valid window, and the
    // others by their median, the last bin holding every median of at least depth_max
    const rc_read_depth *dp = R.depth_on ? J.depth.data() : nullptr;
    const rc_read_depth *dtag = R.depth_tags ? dp : nullptr;
    const size_t DS = dp ? S : 0, bins = (size_t)R.depth_max + 1;
    std::vector<std::vector<uint64_t>> dhist(2 * DS);
    std::vector<uint64_t> dnone(2 * DS, 0);
    auto tally_depth = [&](size_t s, int mate, size_t gi) {
        if (dp[gi].valid <= 0) {
            ++dnone[2 * s + (size_t)mate];
            return;
        }
        std::vector<uint64_t> &hgm = dhist[2 * s + (size_t)mate];
        if (hgm.empty()) hgm.assign(bins, 0);
        ++hgm[std::min<size_t>((size_t)dp[gi].median, bins - 1)];
    };
    // read r of arena A, the gi-th of the batch in ret / l / m / h order
    auto put = [&](OutBuf &out, const Arena &A, size_t r, size_t gi) {
        put_record(out, A, r, J.fastq, J.ret[gi], J.l[gi], J.m[gi], J.h[gi], wk ? wk + gi : nullptr, dtag ? dtag + gi : nullptr);
    };
    auto fmt = [&](size_t lo, size_t hi) {
        for (size_t s = lo; s < hi; ++s) {
            const size_t r0 = n * s / S, r1 = n * (s + 1) / S;
            uint64_t c = 0;
            for (size_t r = r0; r < r1; ++r) {
                if (J.ret[r] > 0) c += (uint64_t)J.ret[r];
                if (J.mode == 1 && J.ret[n + r] > 0) c += (uint64_t)J.ret[n + r];
                if (wk) {
                    tally(s, J.a, r, r);
                    if (J.mode == 1) tally(s, J.b, r, n + r);
                }
                if (dp) {
                    tally_depth(s, J.mode == 2 ? (int)(r & 1) : 0, r);
                    if (J.mode == 1) tally_depth(s, 1, n + r);
                }
            }
            cor[s] = c;
            J.o1[s].reserve((r1 - r0) * 300);
            for (size_t r = r0; r < r1; ++r) {
                put(J.o1[s], J.a, r, r);
                if (alternate) put(J.o1[s], J.b, r, n + r);
            }
            if (J.mode == 1 && !alternate) {
                J.o2[s].reserve((r1 - r0) * 300);
                for (size_t r = r0; r < r1; ++r) put(J.o2[s], J.b, r, n + r);
            }
        }
    };
    g_pool.run(S, [&](size_t s) { fmt(s, s + 1); });
    J.cor_bases = 0;
    for (uint64_t c : cor) J.cor_bases += c;
    J.weak_prefix = J.weak_suffix = J.weak_nosolid = 0;
    for (size_t s = 0; s < WS; ++s) {
        J.weak_prefix += wpre[s];
        J.weak_suffix += wsuf[s];
        J.weak_nosolid += wnone[s];
    }
    for (int mate = 0; mate < 2; ++mate) {
        J.depth_hist[mate].assign(dp ? bins : 0, 0);
        J.depth_novalid[mate] = 0;
        J.depth_reads[mate] = !dp ? 0 : J.mode == 1 ? n : J.mode == 2 ? (n + 1 - (size_t)mate) / 2 : mate == 0 ? n : 0;
        for (size_t s = 0; s < DS; ++s) {
            J.depth_novalid[mate] += dnone[2 * s + (size_t)mate];
            const std::vector<uint64_t> &hgm = dhist[2 * s + (size_t)mate];
            for (size_t d = 0; d < hgm.size(); ++d) J.depth_hist[mate][d] += hgm[d];
        }
    }
    if (gz1 || gz2) {  // deflate every slice into its own gzip member, in parallel
        std::vector<OutBuf> z1(S), z2(S);
        g_pool.run(S, [&](size_t s) {
            if (gz1 && !J.o1[s].empty()) gzip_member(J.o1[s], z1[s]);
            if (gz2 && !J.o2[s].empty()) gzip_member(J.o2[s], z2[s]);
        });
        if (gz1) J.o1.swap(z1);
        if (gz2) J.o2.swap(z2);
    }
}

// (Run::lane_limit; called with R.mu held) the GPU is what this run waits for: as many batches in flight as there are workers, each in its slot lane
static void raise_lane_limit(Run &R, const char *why)
{
    if (!R.adaptive || R.lane_limit >= R.inflight) return;
    R.lane_limit = R.inflight;  // (all the way: 25 M reads of the stress preset, loop 3.3-3.4 s one step per three batches, 2.3 s with four from the start)
    if (!getenv("RC_SLOT_LANES"))
        for (size_t g = 0; g < R.ctx.size(); ++g) {  // (between two submits of that GPU)
            std::lock_guard<std::mutex> sk(R.submit_mu[g]);
            rc_set_slot_lanes(R.ctx[g], 1);
        }
    if (g_timing) fprintf(stderr, "[rc timing] %s: %d batches in flight per GPU from now on\n", why, R.lane_limit);
}

// -histo-after with several GPUs: the corrected bases of one file's share of a batch, as the host holds them -- the byte arena,
// or (a resident batch: the fixes were applied to the text) the sequence lines gathered into one -- to the recount session
static int recount_feed(rc_ctx *c0, const Arena &A)
{
    const size_t n = A.n();
    if (n == 0) return 0;
    if (!A.seq_in_text) return rc_recount_add(c0, A.seq.data(), A.off[n]);
    std::vector<char> buf;
    buf.reserve(A.off[n]);
    for (size_t r = 0; r < n; ++r) {
        uint32_t len = 0;
        const char *s = A.line(r, 1, &len);
        buf.insert(buf.end(), s, s + len);
        buf.push_back(0);
    }
    return rc_recount_add(c0, buf.data(), buf.size());
}

// ---- the four ways a batch reaches slot `slot` of GPU g's context; each returns the library's status ----

// the bytes of a batch's arenas: the first mates' (or all reads'), the second mates', both
struct Extent {
    size_t bytes1, bytes2, nbytes;
};
static Extent extent_of(const Job &J)
{
    const size_t n = J.a.n(), bytes1 = J.a.off[n], bytes2 = J.mode == 1 ? J.b.off[n] : 0;
    return Extent{bytes1, bytes2, bytes1 + bytes2};
}
// (arena 2's bits start at bit bytes1 of the same array: the two arenas' qualities go through one view)
static QualView qual_view(const Job &J, const Extent &E) { return QualView{{&J.a, J.mode == 1 ? &J.b : &J.a}, E.bytes1, E.nbytes}; }

// Submits on one context are serialised, and in front of each the batch registers what it also wants of its corrected reads
// (one shot: a batch that is submitted again registers again): -weak-ends their weak-k-mer profile, -depth-tags / -depth their k-mer depth
template <class F>
static int submit_locked(Run &R, int g, int slot, Job &J, F submit)
{
    std::lock_guard<std::mutex> lk(R.submit_mu[(size_t)g]);
    int rc = R.weak_ends ? rc_weak_profile_into(R.ctx[g], slot, J.weak.data(), R.weak_min) : 0;
    if (!rc && R.depth_on) rc = rc_read_depth_into(R.ctx[g], slot, J.depth.data());
    return rc ? rc : submit();
}

// The reads are in HBM since they were counted: offsets and quality bits go down, the results and the substitutions come back
// and are applied to the sequence lines of the text.  *t_sent: when the host's share of the packing was done.
// RC_STATUS_NOSPACE: not as a resident batch, and the text is untouched -- a read has an empty quality line (see
// has_empty_quality_read), or there are more substitutions than the list has room for (a heavily corrected tail batch: the
// list is sized for one fix per sixteen bases, -maxcorK allows more).
static int run_resident(Run &R, int g, int slot, Job &J, double *t_sent)
{
    const Extent E = extent_of(J);
    const size_t cap = fix_list_room(E.nbytes);
    const Job::PkView pk = J.pk_carve(J.ret.size(), E.nbytes, cap);
    combined_offsets(J, pk.off);
    bool bits_ok = true;
    if (J.fastq) {
        const QualView V = qual_view(J, E);
        bits_ok = for_quality_pieces(E.nbytes, [&](size_t lo, size_t hi) { return pack_quality_bits_from_text(V, R.bad_q, lo, hi, pk.qbits); });
    }
    *t_sent = now_s();
    if (!bits_ok) return RC_STATUS_NOSPACE;
    rc_resident_batch rb;
    memset(&rb, 0, sizeof rb);
    rb.mode = J.mode;
    rb.n = J.a.n();
    rb.arena_a = J.arena_a;
    rb.bytes_a = E.bytes1;
    rb.arena_b = J.arena_b;
    rb.bytes_b = E.bytes2;
    rb.off = pk.off;
    rb.qual_bits = J.fastq ? (const uint8_t *)pk.qbits : nullptr;
    rb.ret = J.ret.data();
    rb.l = J.l.data();
    rb.m = J.m.data();
    rb.h = J.h.data();
    rb.fix_pos = pk.fix_pos;
    rb.fix_chr = pk.fix_chr;
    rb.fix_cap = cap;
    int rc = submit_locked(R, g, slot, J, [&] { return rc_submit_resident(R.ctx[g], &rb, slot); });
    if (!rc) rc = rc_wait_resident(R.ctx[g], slot);
    if (!rc) apply_fixes(J, E.bytes1, rb.fix_pos, rb.fix_chr, rb.n_fix);
    return rc;
}

// the byte arenas as the library takes them
static rc_batch byte_batch(Job &J)
{
    rc_batch rb;
    memset(&rb, 0, sizeof rb);
    rb.mode = J.mode;
    rb.n = J.a.n();
    rb.seq = J.a.seq.data();
    rb.qual = J.a.qual.data();
    rb.off = J.a.off.data();
    if (J.mode == 1) {
        rb.seq2 = J.b.seq.data();
        rb.qual2 = J.b.qual.data();
        rb.off2 = J.b.off.data();
    }
    rb.ret = J.ret.data();
    rb.l = J.l.data();
    rb.m = J.m.data();
    rb.h = J.h.data();
    return rb;
}

// -verbose: the bytes, corrected while the caller waits, with what the transcript prints
static int run_traced(Run &R, int g, Job &J)
{
    const size_t total = J.ret.size(), nbytes = extent_of(J).nbytes;
    J.tr_before.assign(nbytes, 0);
    J.tr_after.assign(nbytes, 0);
    J.tr_flags.assign(total, 0);
    J.tr_niter.assign(total, 0);
    J.tr_iter.assign(total * (size_t)g_trace_iter * RC_TRACE_ITER_WORDS, 0);
    rc_trace tr;
    tr.max_iter = g_trace_iter;
    tr.counts_before = J.tr_before.data();
    tr.counts_after = J.tr_after.data();
    tr.flags = J.tr_flags.data();
    tr.n_iter = J.tr_niter.data();
    tr.iter = J.tr_iter.data();
    rc_batch rb = byte_batch(J);
    std::lock_guard<std::mutex> lk(R.submit_mu[(size_t)g]);
    return rc_correct_batch_traced(R.ctx[g], &rb, &tr);
}

// The packed boundary: the arenas stay here; 2-bit codes, quality bits and the letters outside ACGT go down, the substitutions
// come back as a list and are applied to the arenas in front of the formatter.  RC_STATUS_NOSPACE: more substitutions than the
// list has room for (see run_resident); the arenas are untouched.
static int run_packed(Run &R, int g, int slot, Job &J)
{
    const Extent E = extent_of(J);
    const size_t cap = fix_list_room(E.nbytes);
    const Job::PkView pk = J.pk_carve(J.ret.size(), E.nbytes, cap);
    combined_offsets(J, pk.off);
    const size_t n_exc = pack_bases_of(J, E.nbytes, E.bytes1);
    if (J.fastq) {
        const QualView V = qual_view(J, E);
        for_quality_pieces(E.nbytes, [&](size_t lo, size_t hi) {
            pack_quality_bits_from_arenas(V, R.bad_q, lo, hi, pk.qbits);
            return true;
        });
    }
    rc_packed_batch pb;
    memset(&pb, 0, sizeof pb);
    pb.mode = J.mode;
    pb.n = J.a.n();
    pb.nbytes = E.nbytes;
    pb.off = pk.off;
    pb.bases = (const uint32_t *)J.pk_bases.data();
    pb.qual_bits = J.fastq ? (const uint8_t *)pk.qbits : nullptr;
    pb.exc_pos = n_exc ? (const uint32_t *)J.pk_exc_pos.data() : nullptr;
    pb.exc_chr = n_exc ? (const uint8_t *)J.pk_exc_chr.data() : nullptr;
    pb.n_exc = n_exc;
    pb.ret = J.ret.data();
    pb.l = J.l.data();
    pb.m = J.m.data();
    pb.h = J.h.data();
    pb.fix_pos = pk.fix_pos;
    pb.fix_chr = pk.fix_chr;
    pb.fix_cap = cap;
    int rc = submit_locked(R, g, slot, J, [&] { return rc_submit_packed(R.ctx[g], &pb, slot); });
    if (!rc) rc = rc_wait_packed(R.ctx[g], slot);
    if (!rc) apply_fixes(J, E.bytes1, pb.fix_pos, pb.fix_chr, pb.n_fix);
    return rc;
}

// the bytes: upload + kernels + download are queued at the submit; the wait overlaps with the other workers' packing,
// submitting and formatting
static int run_bytes(Run &R, int g, int slot, Job &J)
{
    const rc_batch rb = byte_batch(J);
    const int rc = submit_locked(R, g, slot, J, [&] { return rc_submit(R.ctx[g], &rb, slot); });
    return rc ? rc : rc_wait(R.ctx[g], slot);
}

// a batch whose byte arenas are here: traced under -verbose, packed under -packed unless a read has an empty quality line, and
// as bytes otherwise -- which is also where a packed batch that came back with RC_STATUS_NOSPACE goes
static int run_arenas(Run &R, int g, int slot, Job &J)
{
    if (g_verbose) return run_traced(R, g, J);
    int rc = RC_STATUS_NOSPACE;
    if (g_packed && !has_empty_quality_read(J)) rc = run_packed(R, g, slot, J);
    return rc == RC_STATUS_NOSPACE ? run_bytes(R, g, slot, J) : rc;
}

// the next batch for this slot of GPU g, counted as one of that GPU's active ones; null: the run is closing
static std::shared_ptr<Job> take_job(Run &R, int g, int slot)
{
    std::unique_lock<std::mutex> lk(R.mu);
    // (a resident batch belongs to the GPU that holds its bases; the others go to whichever context is free)
    auto mine = [&]() {
        for (auto it = R.q.begin(); it != R.q.end(); ++it)
            if ((*it)->gpu < 0 || (*it)->gpu == g) return it;
        return R.q.end();
    };
    auto may_work = [&]() { return slot < R.lane_limit && R.active[(size_t)g] < R.lane_limit; };
    const double tw = now_s();
    R.cv.wait(lk, [&] { return R.closing || (may_work() && mine() != R.q.end()); });
    g_w_worker += now_s() - tw;
    auto it = mine();
    if (it == R.q.end() || !may_work()) return nullptr;  // (the wait ended for `closing` alone)
    std::shared_ptr<Job> j = *it;
    R.q.erase(it);
    ++R.active[(size_t)g];
    return j;
}

static void worker_body(Run &R, int wk)
{
    const int g = wk % R.gpus, slot = wk / R.gpus;
    if (R.numa_on && R.gpus > 1 && !R.shared_gpu) {
        const int node = rc_device_numa_node(R.ctx[g]);
        if (node >= 0) bind_to_numa_node(node);
    }
    while (std::shared_ptr<Job> j = take_job(R, g, slot)) {
        Job &J = *j;
        const double tp0 = now_s();
        const size_t total = J.mode == 1 ? 2 * J.a.n() : J.a.n();
        J.ret.assign(total, 0);
        J.l.assign(total, 0);
        J.m.assign(total, 0);
        J.h.assign(total, 0);
        if (R.weak_ends) J.weak.assign(total, rc_read_weak());   // (see submit_locked)
        if (R.depth_on) J.depth.assign(total, rc_read_depth());
        // [rc timing]: pack is tp0 .. tg0, GPU tg0 .. tf0.  A resident batch's tg0 is taken behind its offsets and quality bits:
        // its host packing counts as pack.  Every other batch's is taken behind pack_arena: what run_packed packs on the host
        // counts as GPU time, and a resident batch that came back counts its whole first attempt, the wait included, as pack.
        double tg0 = tp0;
        int rc = J.resident ? run_resident(R, g, slot, J, &tg0) : RC_STATUS_NOSPACE;
        if (rc == RC_STATUS_NOSPACE) {  // never resident, or not as a resident batch after all: the byte arenas, from the text
            pack_arena(J.a, R.files[(size_t)J.file].path);
            if (J.mode == 1) pack_arena(J.b, R.mates[(size_t)J.file].path);
            tg0 = now_s();
            rc = run_arenas(R, g, slot, J);
        }
        bool fed = true;
        if (!rc && R.recount_host) {
            fed = !recount_feed(R.ctx[0], J.a) && (J.mode != 1 || !recount_feed(R.ctx[0], J.b));
            if (!fed) rc = RC_STATUS_STATE;
        }
        const double tf0 = now_s();
        if (!rc) format_job(R, J);
        const double tf1 = now_s();
        {
            std::lock_guard<std::mutex> lk(R.mu);
            g_t_pack += tg0 - tp0;
            g_t_gpu += tf0 - tg0;
            g_t_format += tf1 - tf0;
            J.rc = rc;
            if (rc) J.err = rc_last_error(fed ? R.ctx[g] : R.ctx[0]);
            J.done = true;
            --R.active[(size_t)g];
            // a batch that took the GPU longer than twice what its output takes to write (15 GB/s, 2.2 output bytes per base):
            // no need to wait for the writer to find out
            // (not the first batches: theirs is the time the kernels' code takes to load -- 10 M x 100 bp reads, ten batches: the first
            // two took 0.1 s each, the lanes they asked for 0.15 s more of a 0.28 s loop)
            const double out_bytes = 2.2 * (double)extent_of(J).nbytes;
            if (!rc && R.batches_done++ >= 2 && tf0 - tg0 > 2.0 * out_bytes / 15e9 + 0.005) raise_lane_limit(R, "a batch takes the GPU longer than the writer");
        }
        R.cv.notify_all();
    }
}

static void writer_body(Run &R)
{
    double waited = 0;
    int starved = 0;
    for (;;) {
        std::shared_ptr<Job> j;
        {
            std::unique_lock<std::mutex> lk(R.mu);
            const double tw = now_s();
            R.cv.wait(lk, [&] { return (!R.order.empty() && R.order.front()->done) || (R.reader_done && R.order.empty()); });
            waited = now_s() - tw;
            g_w_writer += waited;
            if (R.order.empty()) return;
            j = R.order.front();
        }
        if (j->rc) die("rcorrector: %s\n", j->err.c_str());
        const size_t n = j->a.n();
        ReadFile &f = R.files[(size_t)j->file], &g2 = R.mates[(size_t)j->file];
        const bool alternate = j->mode == 1 && g_stdout;  // main.cpp:487-495
        if (g_verbose) {
            // the transcript in the order of the reference's -t 1 loop (main.cpp:368-438): per
            // unit, mate 1's trace [and record, under -stdout], then mate 2's
            std::vector<char> vt;
            const size_t bytes1 = j->a.off[n];
            auto flush = [&]() {
                fwrite(vt.data(), 1, vt.size(), stdout);
                vt.clear();
            };
            for (size_t r = 0; r < n; ++r) {
                put_transcript(vt, *j, j->a, r, r, 0, R.k);
                if (g_stdout) put_record(vt, j->a, r, j->fastq, j->ret[r], j->l[r], j->m[r], j->h[r]);
                if (j->mode == 1) {
                    put_transcript(vt, *j, j->b, r, n + r, bytes1, R.k);
                    if (g_stdout) put_record(vt, j->b, r, j->fastq, j->ret[n + r], j->l[n + r], j->m[n + r], j->h[n + r]);
                }
                if (vt.size() > (1u << 20)) flush();
            }
            flush();
            fflush(stdout);
        }
        const double tw0 = now_s();
        if (j->mode == 1 && !alternate && !g_stdout) {  // two output files: written side by side
            std::thread second([&]() { emit_slices(g2, j->o2); });
            emit_slices(f, j->o1);
            second.join();
        } else {
            if (!(g_verbose && g_stdout)) emit_slices(f, j->o1);
            if (j->mode == 1 && !alternate) emit_slices(g2, j->o2);
        }
        const double wrote = now_s() - tw0;
        g_t_write += wrote;
        if (R.adaptive) {  // (see Run::lane_limit) the writer waited for this batch longer than it then took to write it: twice in a row
            starved = waited > wrote ? starved + 1 : 0;
            if (starved >= 2) {
                starved = 0;
                std::lock_guard<std::mutex> lk(R.mu);
                raise_lane_limit(R, "the writer waits for the GPU");
                R.cv.notify_all();
            }
        }
        R.total_reads += j->ret.size();  // UpdateSummary, main.cpp:73-79
        R.total_cor += j->cor_bases;
        R.weak_prefix += j->weak_prefix;
        R.weak_suffix += j->weak_suffix;
        R.weak_nosolid += j->weak_nosolid;
        for (int mate = 0; mate < 2 && R.depth_on; ++mate) {
            R.depth_reads[mate] += j->depth_reads[mate];
            R.depth_novalid[mate] += j->depth_novalid[mate];
            if (R.depth_hist[mate].size() < j->depth_hist[mate].size()) R.depth_hist[mate].resize(j->depth_hist[mate].size(), 0);
            for (size_t d = 0; d < j->depth_hist[mate].size(); ++d) R.depth_hist[mate][d] += j->depth_hist[mate][d];
        }
        bool retire = false;
        {
            std::lock_guard<std::mutex> lk(R.mu);
            R.order.pop_front();
            j->done = false;
            j->rc = 0;
            // once the reader has handed out its last batch no job is needed again: its buffers -- a GB of text, arenas
            // and output slices each -- are unmapped now, beside the batches still in flight, instead of after _exit
            // where the parent waits for it (0.25 s of a 2 s run)
            if (R.reader_done)
                retire = true;
            else
                R.pool.push_back(j);
        }
        R.cv.notify_all();
        if (retire) {  // (the last reference, as a rule: text, line index, page-locked slab, result arrays and output slices go with it)
            std::shared_ptr<Job> *last = new std::shared_ptr<Job>(std::move(j));
            std::thread([last]() { delete last; }).detach();
        }
    }
}

// (R.mu held) a job at rest, its buffers reused, or a new one
static std::shared_ptr<Job> pooled_job(Run &R)
{
    if (R.pool.empty()) return std::make_shared<Job>();
    std::shared_ptr<Job> j = R.pool.back();
    R.pool.pop_back();
    return j;
}

// (R.mu held through lk) until there is room for one more batch in flight; only the reader adds one, and the room never shrinks
static void wait_for_room(Run &R, std::unique_lock<std::mutex> &lk)
{
    const double tw = now_s();
    R.cv.wait(lk, [&R] { return R.order.size() < (size_t)(R.gpus * R.lane_limit + 2); });
    g_w_reader += now_s() - tw;
}

// the batch to the workers, and to the writer in this order, once there is room for it
static void enqueue(Run &R, const std::shared_ptr<Job> &j)
{
    {
        std::unique_lock<std::mutex> lk(R.mu);
        wait_for_room(R, lk);
        R.order.push_back(j);
        R.q.push_back(j);
    }
    R.cv.notify_all();
}

void run_pipeline(Run &R)
{
    R.pool.swap(R.warm_jobs);  // (the pool holds the only reference to a job at rest: see the writer's retirement)
    R.warm_jobs.clear();
    R.active.assign((size_t)R.gpus, 0);
    std::vector<std::thread> workers;
    for (int wk = 0; wk < R.nworkers; ++wk) workers.emplace_back([&R, wk]() { worker_body(R, wk); });
    std::thread writer([&R]() { writer_body(R); });

    // reader
    if (R.resident) {  // the batches are here already: a pooled job takes over the next one's text, line index and offsets
        for (auto &K : R.kept) {
            std::shared_ptr<Job> j;
            {   // (a job is taken when there is room for it: until then its text, written, stays with the pool)
                std::unique_lock<std::mutex> lk(R.mu);
                wait_for_room(R, lk);
                j = pooled_job(R);
            }
            j->file = K->file;
            j->mode = K->mode;
            j->fastq = K->fastq;
            j->resident = true;
            j->gpu = K->gpu;
            j->arena_a = K->arena_a;
            j->arena_b = K->arena_b;
            j->a.lpr = K->lpr_a;
            j->b.lpr = K->lpr_b;
            j->a.blk.swap(K->a);
            j->a.off.swap(K->off_a);
            j->a.seq_in_text = true;
            if (K->mode == 1) {
                j->b.blk.swap(K->b);
                j->b.off.swap(K->off_b);
                j->b.seq_in_text = true;
            }
            K.reset();  // (the text of the batch this job carried before: written, no longer needed)
            enqueue(R, j);
        }
    } else {
        int ramp = 0;
        for (size_t fi = 0; fi < R.files.size(); ++fi) {
            ReadFile &f = R.files[fi];
            ReadFile *mate = f.paired ? &R.mates[fi] : nullptr;
            const BatchShape S = batch_shape(f, mate);
            for (;;) {
                std::shared_ptr<Job> j;
                {
                    std::lock_guard<std::mutex> lk(R.mu);
                    j = pooled_job(R);
                }
                j->file = (int)fi;
                j->mode = S.mode;
                j->fastq = f.fastq;
                j->resident = false;
                j->gpu = -1;
                j->a.lpr = S.lpr_a;
                j->b.lpr = S.lpr_b;
                // the first batches of a run are small, so that the stages behind the reader start early: an eighth,
                // a quarter, a half of -batch (whole pairs; a read's result does not depend on its batch)
                size_t want_reads = R.batch_reads;
                if (ramp < 3 && R.batch_reads >= ((size_t)1 << 19)) want_reads = (R.batch_reads >> (3 - ramp)) & ~(size_t)1;
                ++ramp;
                if (!take_batch(f, f.src, mate ? &mate->src : nullptr, S, want_reads, j->a.blk, j->b.blk, true)) break;
                enqueue(R, j);
            }
        }
    }
    {
        std::lock_guard<std::mutex> lk(R.mu);
        R.reader_done = true;
        if (!R.pool.empty()) {  // jobs at rest are not needed again either
            auto *idle = new std::vector<std::shared_ptr<Job>>();
            idle->swap(R.pool);
            std::thread([idle]() { delete idle; }).detach();
        }
    }
    R.cv.notify_all();
    writer.join();
    stamp("last batch written");
    {
        std::lock_guard<std::mutex> lk(R.mu);
        R.closing = true;
    }
    R.cv.notify_all();
    for (auto &t : workers) t.join();
}
