// rc_jfdump.h -- the text of a `jellyfish dump` (">COUNT\nKMER\n" per entry), host only: whole-file read, the parser the table
// load runs on several threads, the writer's formatter.  No HIP and no rc_ctx here: rc_api_table.hip drives these, and
// tests/hostmain/jfdump_test.cpp runs them without the library.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

// parsed dump kept between rc_table_load_jfdump() and rc_estimate_error_rate()
struct rc_dump_cache {
    // forward code of every entry (file order), main.cpp:326-328, and a flag "holds a non-ACGT
    // letter before its last base" -- kept in the chunks the parser threads produced (concatenating
    // a few hundred MB on one thread cost more than parsing them on thirty-two)
    std::vector<std::vector<uint64_t>> codes;
    std::vector<std::vector<int8_t>> inv_mid;
    size_t n = 0;
    int load_state_invalid = 0;   // validity of the KmerCode object the load pass leaves behind
    bool valid = false;
};

// host threads for a job of `bytes` bytes: one below `threshold`, else as many as the host has (4 where it does not say), 32 at most
unsigned rc_host_threads(size_t bytes, size_t threshold);

// a whole file in memory, p[n] == 0
struct rc_dump_text {
    char *p = nullptr;
    size_t n = 0;
    rc_dump_text() = default;
    rc_dump_text(const rc_dump_text &) = delete;
    rc_dump_text &operator=(const rc_dump_text &) = delete;
    ~rc_dump_text() { free(p); }
};
// RC_OK, or RC_ERR_IO / RC_ERR_NOMEM with the text in err.  Several threads pread disjoint slices of a file of 8 MiB or more:
// a single reader is bound by the copy out of the page cache
int rc_dump_read_file(const char *path, rc_dump_text *out, char *err, size_t err_len);

// what one piece of the text holds, main.cpp:294-308: every entry's forward code and "non-ACGT letter before its last base";
// of the entries with a count above 1 -- `accepted` of them -- the valid ones' code and count (Store::Put ignores the others,
// Store.h:53-54), and whether the last of them left an invalid KmerCode behind (-1: the piece accepted none)
struct rc_dump_piece {
    std::vector<uint64_t> codes, put_codes;
    std::vector<int8_t> inv_mid;
    std::vector<int32_t> put_counts;
    int64_t accepted = 0;
    int last_state_invalid = -1;
};
// cut[0 .. pieces]: the text in `pieces` pieces of about the same size that begin at entry starts ('>' at offset 0 or behind white space)
std::vector<size_t> rc_dump_cut(const char *text, size_t n, unsigned pieces);
// text[lo, hi) appended to P.  Tokens are white-space separated (fscanf "%s"); the first of a pair is ">COUNT" (atoi of the text
// after the first character), the second the k-mer, pushed through KmerCode::Append character by character (only the last k
// characters survive the mask)
void rc_dump_parse_piece(const char *text, size_t lo, size_t hi, int k, rc_dump_piece *P);
// rc_dump_cut, then every piece parsed by a thread of its own
std::vector<rc_dump_piece> rc_dump_parse(const char *text, size_t n, int k, unsigned pieces);
// the pieces in file order into D (their codes / inv_mid moved, n, load_state_invalid: the last piece that accepted anything
// decides; valid = false) and what goes into the table: entries to put, entries accepted
void rc_dump_join(std::vector<rc_dump_piece> &pieces, rc_dump_cache *D, size_t *n_put, int64_t *accepted);
// the leading entries the ERROR_RATE pass looks at: an entry that leaves an invalid KmerCode behind ends the scan (the
// IsValid() test at main.cpp:323)
size_t rc_dump_scan_length(const rc_dump_cache &D);

// entries [lo, hi) as ">COUNT\nKMER\n" appended to out
void rc_dump_format(const uint64_t *codes, const int32_t *counts, size_t lo, size_t hi, int k, std::vector<char> *out);
