// mini_forms.hpp -- the minimizer of every position of a word, as the plan kernel and the first scatter pass of mini.hip compute
// it, in a form that host code compiles too: no HIP header is needed, and tests/test_minimizer_forms_host.py builds a plain C++
// program from this file that compares every routine here with the definition (mini_minimizer_of in pg_device.hpp), position
// by position.  Device code reaches it through pg_device.hpp; everything lives in an anonymous namespace like the rest.
#ifndef PG_MINI_FORMS_HPP
#define PG_MINI_FORMS_HPP
#include <stdint.h>

#include "pangaea_feat.h"

#if defined(__HIPCC__)
#define PG_HD __host__ __device__ __forceinline__
#else
#define PG_HD inline
#endif
#if defined(__clang__)
#define PG_UNROLL _Pragma("unroll")
#else
#define PG_UNROLL
#endif

namespace {

// low 32 bits of the product of the low 24 bits of a and b (v_mul_u32_u24: full rate; HIP declares __umul24 as returning int)
PG_HD uint32_t umul24_lo(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__umul24(a, b);
#else
    return (a & 0xffffffu) * (b & 0xffffffu);
#endif
}
PG_HD uint32_t brev32(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(x);
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
    return (x >> 16) | (x << 16);
#endif
}

// M depends on k alone: 13 from k = 16 on, 11 for 13 <= k <= 15 (Pangaea's default k = 15 then has windows of five 11-mers;
// with 13-mers it would have three and hardly any k-mer would share its minimizer with a neighbour)
constexpr int MINI_M = PG_MINI_M, MINI_M_SMALL = PG_MINI_M_SMALL;
PG_HD int mini_m(int k) { return k >= MINI_M + 3 ? MINI_M : MINI_M_SMALL; }
static_assert(PG_MINI_MIN_K == MINI_M_SMALL + 2, "windows of at least three M-mers");

// The order in which M-mers compete for "minimizer": a multiplicative hash of the low 24 bits of the canonical M-mer (its
// oldest character does not take part: M-mers that differ only there tie, and a tie is harmless -- the bucket is a function of
// the minimum VALUE, which both strands compute from the same multiset).  The xor keeps poly-A (code 0) from being the
// smallest value of all.  Two full-rate instructions (v_xor, v_mul_u32_u24): this runs once per character of the stream in
// kernels that are bound by VALU issue; the three-xorshift mixer it replaces took seven.
PG_HD uint32_t mhash(uint32_t x)
{
    return umul24_lo(x ^ 0x5E3779u, 0xC2B2AFu);
}
// bucket of a minimizer value.  The value is a minimum -- its HIGH bits are biased towards 0 --, but its low 24 bits are a
// bijection of the minimizer M-mer's own low 24 bits (mhash: a product with an odd constant), as uniform as the M-mers are: one
// more 24-bit product mixes them upwards and the top bits of its low dword are the bucket.  (v_mul_u32_u24 takes the low 24 bits of
// its operands by itself and issues at full rate; the 32-bit product this replaces, v_mul_lo_u32, at a quarter of it -- and since
// round 4 the bucket of EVERY position of the stream is computed, not one per record.)
PG_HD uint32_t mini_bucket_product(uint32_t minv) { return umul24_lo(minv, 0x9E3779u); }
PG_HD uint32_t mini_bucket(uint32_t minv, int bits)
{
    return bits ? mini_bucket_product(minv) >> (32 - bits) : 0u;
}
PG_HD uint32_t swap_pairs32(uint32_t x) { return ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1); }
// order of the 32 two-bit characters of a word reversed
PG_HD uint64_t rev2_64(uint64_t x)
{
    const uint32_t lo = swap_pairs32(brev32((uint32_t)x)), hi = swap_pairs32(brev32((uint32_t)(x >> 32)));
    return ((uint64_t)lo << 32) | hi;
}
// The M-mers of a k-mer that compete for its minimizer: all k - M + 1 of them up to 9, beyond that (k > 21) the CENTRAL 8 or 9
// (same parity as k - M + 1, so that `off` M-mers are left out on either side).  The reverse complement maps M-mer t to
// k - M - t, i.e. the central window onto itself: both strands pick the same M-mer, as they must.  A window of at most 9
// keeps the rolling minimum of the first scatter pass in 9 registers for every k.
constexpr int MINI_MAX_WINDOW = 9;
PG_HD void mini_window(int k, int *wc, int *off)
{
    const int w = k - mini_m(k) + 1;
    *wc = w <= MINI_MAX_WINDOW ? w : MINI_MAX_WINDOW - 1 + (w & 1);
    *off = (w - *wc) / 2;
}

// ---- the minimizer value of the k-mer that ends at every character of a word
//
// per_pos(p, mv) for p = 0 .. 31 (p a compile-time constant at every call once the loop is unrolled): mv = the smallest
// mhash(canonical M-mer) over the W M-mers of the window that ends at character p of `cw` (DELAY, k > 21: that ends `off` <= 5
// characters before it -- the central window of mini_window), `pw` being the word in front of it.
//
// Canonical M-mer, six instructions: the M-mer that ends at character q of the 64 characters (pw, cw) and its reverse
// complement are cut LEFT-ALIGNED out of four dwords each -- the reverse complement out of the words complemented once (oldest
// character lowest: its characters q - 15 .. q), the M-mer itself out of the character-reversed words (newest character lowest)
// -- at offsets that are constants once the loop is unrolled: one funnel shift each and no mask.  Below the M-mer's 2 M bits
// both hold neighbouring characters, which never decide the comparison: M is odd, so an M-mer differs from its reverse
// complement inside those 2 M bits.  One minimum, one shift that drops the neighbours, then mhash (xor, 24-bit product).  For
// the newest 16 - M positions of the word the forward cut would start below bit 0: there it is a plain left shift.
//
// Window minimum, two instructions: the minima g of groups of G = ceil(W / 3) consecutive hashes (one v_min3 or v_min, nothing
// for W = 3), then one v_min3 over the three groups that end at the position, G and W - G positions before it (they overlap
// where W is not a multiple of 3).
constexpr int MINI_MAX_OFF = 5;
PG_HD uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }
// 32 bits from bit b of the four dwords w (bits outside them read as 0)
PG_HD uint32_t cut128(const uint32_t (&w)[4], int b)
{
    const int j = b >= 0 ? b >> 5 : -((-b + 31) >> 5), s = b - 32 * j;
    const uint32_t lo = j >= 0 && j < 4 ? w[j] : 0u, hi = j + 1 >= 0 && j + 1 < 4 ? w[j + 1] : 0u;
    return s == 0 ? lo : (lo >> s) | (hi << (32 - s));
}
template <int W, bool DELAY, int M, class PerPos>
PG_HD void mini_minimizers_of_word(uint64_t pw, uint64_t cw, int off, PerPos &&per_pos)
{
    constexpr int SH = 32 - 2 * M;                              // bits below a left-aligned M-mer
    constexpr int G = (W + 2) / 3;                              // hashes per group
    constexpr int PRE = W - 1 + (DELAY ? MINI_MAX_OFF : 0);     // M-mers in front of the word that are wanted in the window
    constexpr int Q0 = 32 - PRE, NQ = 32 + PRE;
    static_assert(M % 2 == 1 && SH >= 0, "an M-mer is never its own reverse complement, and fits a dword");
    static_assert(W >= 3 && W <= MINI_MAX_WINDOW, "windows of three to nine M-mers");
    static_assert(Q0 >= 15, "the 16 characters that end at the first wanted M-mer lie inside the previous word");
    const uint64_t rcw = rev2_64(cw), rpw = rev2_64(pw);
    const uint64_t ccw = cw ^ 0xAAAAAAAAAAAAAAAAull, cpw = pw ^ 0xAAAAAAAAAAAAAAAAull;
    const uint32_t fwd[4] = {(uint32_t)rcw, (uint32_t)(rcw >> 32), (uint32_t)rpw, (uint32_t)(rpw >> 32)};
    const uint32_t rcp[4] = {(uint32_t)cpw, (uint32_t)(cpw >> 32), (uint32_t)ccw, (uint32_t)(ccw >> 32)};
    uint32_t h[NQ], g[NQ], mv[NQ];                              // (index i: character Q0 + i; every index below is a constant)
    PG_UNROLL
    for (int i = 0; i < NQ; ++i) {
        const int q = Q0 + i;
        const uint32_t fl = cut128(fwd, 2 * (63 - q) - SH), rl = cut128(rcp, 2 * (q - 15));
        h[i] = mhash(min_u32(fl, rl) >> SH);
        // (the inner minimum of each is taken of a pair of positions that no other group or window holds together: of a pair that
        // a neighbour shares the compiler makes a common subexpression, and two v_min of what was one v_min3)
        if (i >= G - 1) g[i] = G == 1 ? h[i] : G == 2 ? min_u32(h[i], h[i - 1]) : min_u32(min_u32(h[i], h[i - 2]), h[i - 1]);
        if (i >= W - 1) mv[i] = W == 2 * G ? min_u32(g[i], g[i - G]) : min_u32(min_u32(g[i], g[i - (W - G)]), g[i - G]);
        if (i >= PRE) {
            uint32_t use = mv[i];
            if (DELAY) {                                        // (off is the same for the whole launch: scalar selects)
    PG_UNROLL
                for (int d = 1; d <= MINI_MAX_OFF; ++d) use = off == d ? mv[i - d] : use;
            }
            per_pos(i - PRE, use);
        }
    }
}

// ---- "same minimizer value as the position before", one bit per position, in two instructions each: a compare and an add with
// carry that shifts the bit in from below (eq' = eq + eq + bit).  Position 0 continues nothing (mini_record_ends never reads its
// bit) and is not pushed; after positions 1 .. 31 position p stands at bit 31 - p, and eq_mask_finish turns the mask round.
// The add is inline assembly on the device -- written as `eq + eq + bit` the compiler makes a select and an or of it, three
// instructions per position --, and only the add: the compare is an ordinary ballot, whose mask is the carry that goes in.
PG_HD void eq_mask_push(uint32_t &eq_rev, uint32_t mv, uint32_t prev)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long same = __builtin_amdgcn_ballot_w64(mv == prev);
    unsigned long long carry_out;
    asm("v_addc_co_u32_e64 %0, %1, %0, %0, %2" : "+v"(eq_rev), "=s"(carry_out) : "s"(same));
#else
    eq_rev = eq_rev + eq_rev + (mv == prev ? 1u : 0u);
#endif
}
PG_HD uint32_t eq_mask_finish(uint32_t eq_rev) { return brev32(eq_rev); }

// ---- the plan's column: of a position's bucket the plan reads the region only, the top `bits1` <= 8 bits of
// mini_bucket_product, so its column holds the product's top BYTE, four positions to a dword (position p in byte p & 3 of dword
// p >> 2): one v_perm_b32 per position shifts the byte in from above, one LDS write per four positions stores the dword.
PG_HD uint32_t region_bytes_push(uint32_t acc, uint32_t mv)
{
    const uint32_t prod = mini_bucket_product(mv);
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(prod, acc, 0x07030201u);       // bytes 1 .. 3 of acc, above them byte 3 of prod
#else
    return (acc >> 8) | (prod & 0xff000000u);
#endif
}
// region (bits1 = log2 of the number of regions, 0 .. 8) of position p, from the dword that holds its byte
PG_HD uint32_t region_of_bytes(uint32_t dword, int p, int bits1) { return ((dword >> (8 * (p & 3))) & 0xffu) >> (8 - bits1); }

}  // namespace
#endif
