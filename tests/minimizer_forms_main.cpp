// Stand-alone host program of tests/test_minimizer_forms_host.py: the per-position forms of pangaea_amd/csrc/mini_forms.hpp
// (canonical M-mer without masks, window minimum as a tree, the "same value as before" mask, the plan's packed region column)
// against the definition written naively here, character by character, with its own copies of the two hash constants.
// Exit status 0 and a line "ok ..." when everything agrees; the first few differences and status 1 otherwise.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mini_forms.hpp"

namespace {

int failures = 0;
long long compared = 0;

// ---- the definition
uint32_t naive_mhash(uint32_t x) { return (uint32_t)((uint64_t)((x ^ 0x5E3779u) & 0xffffffu) * 0xC2B2AFu); }
uint32_t naive_bucket(uint32_t mv, int bits) { return bits ? (uint32_t)((uint64_t)(mv & 0xffffffu) * 0x9E3779u) >> (32 - bits) : 0u; }
int naive_char(uint64_t pw, uint64_t cw, int q) { return (int)(((q < 32 ? pw : cw) >> (2 * (q & 31))) & 3u); }      // oldest character lowest

// minimizer value of the k-mer that ends at character q (32 .. 63) of (pw, cw): the smallest hashed canonical M-mer of its
// central window -- as mini_minimizer_of has it: M-mer t (t = 0: the newest) for t = off .. off + wc - 1
uint32_t naive_minimizer(uint64_t pw, uint64_t cw, int q, int k)
{
    const int m = k >= 16 ? 13 : 11, w = k - m + 1;
    const int wc = w <= 9 ? w : 8 + (w & 1), off = (w - wc) / 2;
    uint32_t best = 0xffffffffu;
    for (int t = off; t < off + wc; ++t) {
        uint32_t fw = 0, rc = 0;
        for (int j = 0; j < m; ++j) {                               // the M-mer's characters, oldest first
            const int c = naive_char(pw, cw, q - t - (m - 1) + j);
            fw = (fw << 2) | (uint32_t)c;                           // oldest character highest
            rc |= (uint32_t)(c ^ 2) << (2 * j);                     // reversed and complemented
        }
        const uint32_t h = naive_mhash(fw < rc ? fw : rc);
        best = h < best ? h : best;
    }
    return best;
}

// ---- the forms under test, for the instantiation mini.hip's with_window picks for k
template <int W, bool DELAY, int M> void forms(uint64_t pw, uint64_t cw, int off, uint32_t *mv, uint32_t *eq, uint32_t *col)
{
    uint32_t e = 0, prev = 0, acc = 0;
    mini_minimizers_of_word<W, DELAY, M>(pw, cw, off, [&](int p, uint32_t v) {
        mv[p] = v;
        if (p > 0) eq_mask_push(e, v, prev);
        prev = v;
        acc = region_bytes_push(acc, v);
        if ((p & 3) == 3) col[p >> 2] = acc;
    });
    *eq = eq_mask_finish(e);
}
void forms_for(int k, uint64_t pw, uint64_t cw, uint32_t *mv, uint32_t *eq, uint32_t *col)
{
    int wc, off;
    mini_window(k, &wc, &off);
    if (k > 21) return wc == 8 ? forms<8, true, 13>(pw, cw, off, mv, eq, col) : forms<9, true, 13>(pw, cw, off, mv, eq, col);
    if (k < 16) return wc == 3 ? forms<3, false, 11>(pw, cw, off, mv, eq, col) : wc == 4 ? forms<4, false, 11>(pw, cw, off, mv, eq, col) : forms<5, false, 11>(pw, cw, off, mv, eq, col);
    switch (wc) {
    case 4: return forms<4, false, 13>(pw, cw, off, mv, eq, col);
    case 5: return forms<5, false, 13>(pw, cw, off, mv, eq, col);
    case 6: return forms<6, false, 13>(pw, cw, off, mv, eq, col);
    case 7: return forms<7, false, 13>(pw, cw, off, mv, eq, col);
    case 8: return forms<8, false, 13>(pw, cw, off, mv, eq, col);
    default: return forms<9, false, 13>(pw, cw, off, mv, eq, col);
    }
}

void fail(const char *what, int k, uint64_t pw, uint64_t cw, int p, uint64_t got, uint64_t want)
{
    if (++failures <= 10)
        std::printf("k=%d pw=%016llx cw=%016llx position %d: %s is %llx, the definition gives %llx\n", k, (unsigned long long)pw,
                    (unsigned long long)cw, p, what, (unsigned long long)got, (unsigned long long)want);
}

void check_pair(int k, uint64_t pw, uint64_t cw)
{
    uint32_t mv[32], eq = 0, col[8], want[32];
    forms_for(k, pw, cw, mv, &eq, col);
    for (int p = 0; p < 32; ++p) {
        want[p] = naive_minimizer(pw, cw, 32 + p, k);
        if (mv[p] != want[p]) fail("the minimizer value", k, pw, cw, p, mv[p], want[p]);
        const uint32_t same = p > 0 && want[p] == want[p - 1] ? 1u : 0u;      // (position 0 continues nothing: its bit is 0)
        if (((eq >> p) & 1u) != same) fail("the bit of the mask", k, pw, cw, p, (eq >> p) & 1u, same);
        // the region of every geometry: bits1 region bits on top of bits2 second-pass bits (bits = bits1 + bits2 <= 16)
        for (int bits1 = 0; bits1 <= 8; ++bits1)
            for (int bits2 = 0; bits2 <= 8; bits2 += 4) {
                const uint32_t region = naive_bucket(want[p], bits1 + bits2) >> bits2;
                const uint32_t got = region_of_bytes(col[p >> 2], p, bits1);
                if (got != region) fail("the region out of the packed column", k, pw, cw, p, got, region);
                if (bits1 + bits2 > 0 && mini_bucket(mv[p], bits1 + bits2) != naive_bucket(want[p], bits1 + bits2))
                    fail("mini_bucket", k, pw, cw, p, mini_bucket(mv[p], bits1 + bits2), naive_bucket(want[p], bits1 + bits2));
            }
        compared += 1;
    }
}

uint64_t rng_state = 0x243F6A8885A308D3ull;
uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

// a word whose newest M characters are the reverse complement of its oldest M (the rest random)
uint64_t ends_reverse_complementary(int m)
{
    uint64_t w = rnd();
    for (int j = 0; j < m; ++j) {
        const uint64_t c = (w >> (2 * j)) & 3u;
        w = (w & ~(3ull << (2 * (31 - j)))) | ((c ^ 2u) << (2 * (31 - j)));
    }
    return w;
}

}  // namespace

int main(int argc, char **argv)
{
    const int n_random = argc > 1 ? std::atoi(argv[1]) : 3000;
    for (int k = 13; k <= 31; ++k) {
        const int m = k >= 16 ? 13 : 11;
        // edge words: all-A, all-T, alternating AT / TA, alternating AC (hashes that recur with period two), ends that are each
        // other's reverse complement -- every ordered pair of them, and each beside random words
        std::vector<uint64_t> edge = {0ull, 0xAAAAAAAAAAAAAAAAull, 0x8888888888888888ull, 0x2222222222222222ull, 0x4444444444444444ull,
                                      ends_reverse_complementary(m), ends_reverse_complementary(m)};
        for (uint64_t a : edge)
            for (uint64_t b : edge) check_pair(k, a, b);
        for (uint64_t a : edge)
            for (int i = 0; i < 8; ++i) { check_pair(k, a, rnd()); check_pair(k, rnd(), a); }
        // the oldest M-mer of the current word against the newest of the previous one
        for (int i = 0; i < 16; ++i) {
            const uint64_t w = ends_reverse_complementary(m);
            check_pair(k, w, w);
        }
        for (int i = 0; i < n_random; ++i) check_pair(k, rnd(), rnd());
        // few distinct characters: equal hashes inside a window, long runs of one minimizer value
        for (int i = 0; i < n_random / 4; ++i) check_pair(k, rnd() & 0x5555555555555555ull, rnd() & 0x1111111111111111ull);
    }
    if (failures) {
        std::printf("%d differences in %lld positions\n", failures, compared);
        return 1;
    }
    std::printf("ok %lld positions\n", compared);
    return 0;
}
