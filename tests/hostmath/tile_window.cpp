// rc_tile_window (rc_common.h: the k-byte window at a position of a staged tile, as k_probe, k_probe_list, k_count_scan and
// k_weak_planes cut it) against a loop over the bytes.  The planes are built here from the packer's per-byte definition
// (rc_device.h: rc_pack16 / rc_tile_pack), for a "tile" of 128 bytes + 32 bytes of halo + the two sentinel code words.
// Every k in 4 .. 32 at every position, over: letters only; a NUL at each single position; an N / a lower-case letter at each
// single position; a NUL and an N exactly k apart, in both orders.  Both variants (with and without the NUL plane).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "rc_common.h"

static const int TILE = 128, NCH = TILE / 16 + 2;  // chunks of 16 bytes: the tile and its halo
static unsigned char buf[NCH * 16];                // (the halo stays NUL: what lies behind an arena's end)
static uint32_t s_code[NCH + 2], m_inv[NCH / 2], m_nul[NCH / 2];

static int pack()
{
    uint16_t s_inv[NCH], s_nul[NCH];
    memset(s_code, 0, sizeof s_code);
    memset(s_inv, 0, sizeof s_inv);
    memset(s_nul, 0, sizeof s_nul);
    for (int p = 0; p < NCH * 16; ++p) {  // byte p = byte j of chunk c
        const int c = p / 16, j = p % 16;
        const unsigned ch = buf[p];
        unsigned v = 3, bad = 1;
        if (ch == 'A') { v = 0; bad = 0; }
        if (ch == 'C') { v = 1; bad = 0; }
        if (ch == 'G') { v = 2; bad = 0; }
        if (ch == 'T') { v = 3; bad = 0; }
        s_code[c] |= v << (30 - 2 * j);
        s_inv[c ^ 1] |= (uint16_t)(bad << (15 - j));
        s_nul[c ^ 1] |= (uint16_t)((ch == 0 ? 1u : 0u) << (15 - j));
    }
    s_code[NCH] = s_code[NCH + 1] = 0xFFFFFFFFu;
    memcpy(m_inv, s_inv, sizeof m_inv);  // (the kernels read the 16-bit planes as 32-bit words; gfx950 and this host are little-endian)
    memcpy(m_nul, s_nul, sizeof m_nul);
    for (int p = 0; p < NCH * 16; ++p)  // the layout rc_tile_window documents: byte p at bit 31 - p % 32 of word p / 32
        if (((m_nul[p / 32] >> (31 - p % 32)) & 1u) != (buf[p] == 0 ? 1u : 0u)) {
            printf("mask layout: byte %d\n", p);
            return 1;
        }
    return 0;
}

static long n_checked = 0;

// every position of the tile at this k, both variants
static int check(int k, const char *what, int at)
{
    if (pack()) return 1;
    for (int a = 0; a < TILE; ++a) {
        bool nul = false, bad = false;
        uint64_t code = 0;
        for (int i = 0; i < k; ++i) {
            const unsigned ch = buf[a + i];
            const char *q = ch ? strchr("ACGT", (int)ch) : nullptr;
            nul |= ch == 0;
            bad |= q == nullptr;
            code = (code << 2) | (uint64_t)(q ? q - "ACGT" : 0);
        }
        if (bad) code = 0;
        const rc_tile_win w = rc_tile_window<true>(s_code, m_inv, m_nul, a, k);
        const rc_tile_win v = rc_tile_window<false>(s_code, m_inv, nullptr, a, k);
        if (w.nul != nul || w.bad != bad || w.code != code || v.nul || v.bad != bad || v.code != code) {
            printf("mismatch: %s at %d, k %d, position %d: want nul %d bad %d code %016llx; got %d %d %016llx, without the NUL plane %d %d %016llx\n",
                   what, at, k, a, nul, bad, (unsigned long long)code, w.nul, w.bad, (unsigned long long)w.code, v.nul, v.bad,
                   (unsigned long long)v.code);
            return 1;
        }
        ++n_checked;
    }
    return 0;
}

int main()
{
    unsigned char letters[TILE];
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int p = 0; p < TILE; ++p) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        letters[p] = (unsigned char)"ACGT"[(s >> 33) & 3];
    }
    for (int k = 4; k <= 32; ++k) {
        memcpy(buf, letters, TILE);
        if (check(k, "letters only", 0)) return 1;
        const unsigned char single[] = {0, 'N', 'a', 't'};
        for (unsigned char c : single)
            for (int p = 0; p < TILE; ++p) {
                memcpy(buf, letters, TILE);
                buf[p] = c;
                if (check(k, c == 0 ? "a NUL" : c == 'N' ? "an N" : "a lower-case letter", p)) return 1;
            }
        for (int p = 0; p + k < TILE; ++p) {  // a window of k bytes holds one of the two, never both
            memcpy(buf, letters, TILE);
            buf[p] = 0;
            buf[p + k] = 'N';
            if (check(k, "a NUL, and an N k behind it", p)) return 1;
            buf[p] = 'N';
            buf[p + k] = 0;
            if (check(k, "an N, and a NUL k behind it", p)) return 1;
        }
    }
    printf("ok %ld windows\n", n_checked);
    return 0;
}
