// rc_stage16 + rc_pack16m (rc_common.h: how k_single brings a read into LDS, sixteen bases per lane) against a byte-at-a-time
// restatement with rc_base_code: the staged bytes, the code word, the A / T / not-ACGT masks.  The arena is a heap block of exactly nbytes bytes -- build with
// -fsanitize=address,undefined and a load past it (or in front of it) stops the program -- and the read lies at its very end,
// 0 .. 3 bytes in front of it: every o mod 16, every len 0 .. 160, every nbytes mod 4; byte content cycles through all 256
// values at several phases, plus a pass of letters.  Also checked: a group past the read's end loads nothing and is all "not a base".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "rc_common.h"

static long n_groups = 0;

static int check_read(const uint8_t *a, size_t nbytes, uint32_t o, int len)
{
    const int ng = (len + 15) / 16;
    for (int j = 0; j <= ng; ++j) {  // (j == ng: a group with no byte of the read)
        uint32_t w[4], code, am, tm, bad;
        rc_stage16(a, nbytes, o, len, j, w);
        rc_pack16m(w, code, am, tm, bad);
        uint32_t ew[4] = {0, 0, 0, 0}, ecode = 0, eam = 0, etm = 0, ebad = 0;
        for (int b = 0; b < 16; ++b) {
            const int p = 16 * j + b;
            const uint32_t c = p < len ? a[(size_t)o + p] : 0u;  // at or past len: not a base
            const int v = rc_base_code(c);
            ew[b >> 2] |= c << (8 * (b & 3));
            ecode |= (uint32_t)(v > 3 ? 3 : v) << (30 - 2 * b);
            eam |= (v == 0 ? 1u : 0u) << b;
            etm |= (v == 3 ? 1u : 0u) << b;
            ebad |= (v >= 4 ? 1u : 0u) << b;
        }
        ++n_groups;
        if (memcmp(w, ew, 16) || code != ecode || am != eam || tm != etm || bad != ebad) {
            printf("mismatch: nbytes %zu o %u len %d group %d\n got w %08x %08x %08x %08x code %08x am %04x tm %04x bad %04x\n"
                   "want w %08x %08x %08x %08x code %08x am %04x tm %04x bad %04x\n",
                   nbytes, o, len, j, w[0], w[1], w[2], w[3], code, am, tm, bad, ew[0], ew[1], ew[2], ew[3], ecode, eam, etm, ebad);
            return 1;
        }
    }
    return 0;
}

int main()
{
    static const char letters[] = "ACGTNacgtnACGTACGTRYACGTTTTTAAAA";
    for (int phase = 0; phase < 9; ++phase)
        for (uint32_t o = 0; o < 48; ++o)            // every o mod 16, three times over (o = 0: nothing in front of the read)
            for (int len = 0; len <= 160; ++len)
                for (int pad = 0; pad < 4; ++pad) {  // bytes behind the read: with every len, every nbytes mod 4
                    const size_t nbytes = (size_t)o + (size_t)len + (size_t)pad;
                    uint8_t *a = (uint8_t *)malloc(nbytes ? nbytes : 1);  // (16-byte aligned, as the arena is)
                    if (!a) return 2;
                    for (size_t i = 0; i < nbytes; ++i)
                        a[i] = phase < 8 ? (uint8_t)(i * 1u + 37u * (unsigned)phase + 3u * o) : (uint8_t)letters[(i * 7 + o + (size_t)len) & 31];
                    const int bad = check_read(a, nbytes, o, len);
                    free(a);
                    if (bad) return 1;
                }
    printf("ok %ld groups\n", n_groups);
    return 0;
}
