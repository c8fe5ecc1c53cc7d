// table_ops.hip -- gfx950 kernels that work on a FINISHED k-mer table, and their C-ABI launchers: query and spectrum, the text dump
// and its reload, merge, combine and compare, depth of sequences, reads of a FASTQ text by their k-mers' counts.  None of them is on the timed path (kernels.hip: counting and
// features; mini.hip: the super-k-mer pipeline); what they share with it is pg_table.hpp.
//
// Replaces (reference file:line): jellyfish query / histo / dump / merge over the table of feature.py:76-103 and
// the dump reload of cpptools/count_kmer.cpp:139-170; each section says which.
//
// Shared inside this file: Lookup (pg_table.hpp; one probe in two halves, by table kind), dump_load + entry_of (one entry of a
// table's storage, by layout, as code, key and count), stream_slice (a bucket's slice of an aligned source), and on the host
// with_kind / with_form / probe_args in place of per-launcher switches.
#include "pg_table.hpp"

namespace {

// -------------------------------------------------------------------------------- reading a finished table
//
// What `jellyfish query` and `jellyfish histo` answer from the dump that the reference keeps (feature.py:87,103).  Both kernels
// only read the table: plain loads, no atomics on it.

// out[i] = multiplicity of the k-mer codes[i] (either strand; the stream's encoding, newest character in the low bits), 0 when
// the table does not hold it, PG_QUERY_INVALID when the code has a bit at or above 2k -- such a code reads no table memory.
// One query per lane and turn, QRY_BATCH turns at a time: the first probes of the batch are issued before any is resolved
// (every probe is a random 8-byte read, i.e. one 64-byte line, as the lookups of features_kernel).
// The lookup stays spelled out here, in three arrays, and is not Lookup<TK> (pg_table.hpp): on Lookup the kernel came out 24 instructions
// shorter and 2.3 % slower (10^8 queries of a 2^29-slot mini table: 3.16 ms against 3.09; profiles/table_ops_split_ab.txt).
constexpr int QRY_BATCH = 8;
template <int TK>
__global__ __launch_bounds__(BLOCK) void table_query_kernel(const uint64_t *__restrict__ codes, int64_t n, int k,
                                                            const uint32_t *__restrict__ dense, HashView t, uint32_t *__restrict__ out)
{
    const uint64_t kmask = low_mask<uint64_t>(k);
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t i0 = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i0 < n; i0 += stride * QRY_BATCH) {
        uint64_t key[QRY_BATCH], hh[QRY_BATCH], cur[QRY_BATCH];
        bool ask[QRY_BATCH];
#pragma unroll
        for (int u = 0; u < QRY_BATCH; ++u) {
            const int64_t i = i0 + u * stride;
            const uint64_t fw = i < n ? codes[i] : ~0ull;
            ask[u] = (fw & ~kmask) == 0;                   // (a lane past the end asks nothing and writes nothing)
            key[u] = hh[u] = cur[u] = 0;
            if (!ask[u]) continue;
            // the reverse complement as Roller builds it: complement = ^ 2 per character, order reversed
            const uint64_t rc = rev2_64(fw ^ 0xAAAAAAAAAAAAAAAAull) >> (64 - 2 * k);
            const uint64_t canon = fw < rc ? fw : rc;
            if (TK == TK_DENSE) {
                cur[u] = dense[(uint32_t)canon];
            } else {
                key[u] = TK == TK_HASH ? key42(canon) : canon;
                hh[u] = TK == TK_WIDE ? t.home_wide(canon) : (TK == TK_MINI || TK == TK_MINIW) ? t.home_mini(canon, k) : t.home_key(key[u]);
                cur[u] = t.slots[hh[u]];
            }
        }
#pragma unroll
        for (int u = 0; u < QRY_BATCH; ++u) {
            const int64_t i = i0 + u * stride;
            if (i >= n) continue;
            uint32_t cnt = PG_QUERY_INVALID;
            if (ask[u]) {
                bool found;
                if (TK == TK_DENSE) cnt = (uint32_t)cur[u];
                else if (TK == TK_WIDE || TK == TK_MINIW) cnt = wide_probe(t, hh[u], cur[u], key[u], &found);
                else cnt = hash_probe(t, hh[u], cur[u], key[u], &found);
            }
            out[i] = cnt;
        }
    }
}

// hist[c] += distinct k-mers of multiplicity c (1 <= c <= high), hist[high + 1] += those above; hist zeroed by the launcher.
// One streaming pass, 16 bytes per lane and load (FORM: four dense counters, two packed slots, or four keys of the key
// plane with their four counts), SPEC_UNROLL loads in flight per lane.  Bins are 32-bit LDS counters (dynamic LDS, high + 2 of
// them: at most 64 KiB); a workgroup sees fewer than 2^32 slots (the launcher's grid), so none overflows.  Real spectra are
// mostly c == 1 (sequencing errors): all 64 lanes would add to one LDS counter, so those lanes are counted with a ballot and
// kept in a register of the wavefront until the end (BALLOT >= 1; BALLOT == 2: c == 2 as well); every other count is an LDS add
// whose result nobody reads.  Non-zero bins leave with one 64-bit global add each: integer sums, the same whatever the order.
// the storage layout of a table: dense counters, packed slots (hash: the slot holds key42 of the code; mini: the code), or the
// planes of the wide kinds (keys = code + 1, then 32-bit counts).  The spectrum reads counts alone: its packed path is DUMP_HASH.
enum { DUMP_DENSE = 0, DUMP_HASH = 1, DUMP_MINI = 2, DUMP_PLANES = 3 };
constexpr int SPEC_UNROLL = 4;
template <int BALLOT> __device__ __forceinline__ void spectrum_bin(uint32_t *bins, uint32_t c, uint32_t cap, uint32_t &ones, uint32_t &twos)
{
    c = c < cap ? c : cap;
    if (BALLOT >= 1) ones += (uint32_t)__popcll(__ballot(c == 1));
    if (BALLOT >= 2) twos += (uint32_t)__popcll(__ballot(c == 2));
    if (c > (uint32_t)BALLOT) atomicAdd(&bins[c], 1u);
}
template <int FORM, int BALLOT>
__global__ __launch_bounds__(BIG_BLOCK) void table_spectrum_kernel(const uint4 *__restrict__ slots, const uint4 *__restrict__ counts, int64_t n_units,
                                                                   int high, unsigned long long *__restrict__ hist)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t bins[];
    const int n_bins = high + 2;
    const uint32_t cap = (uint32_t)high + 1u;
    for (int i = threadIdx.x; i < n_bins; i += BIG_BLOCK) bins[i] = 0;
    lds_sync();
    uint32_t ones = 0, twos = 0;                                     // (the same in every lane of a wavefront)
    constexpr int64_t TILE = (int64_t)BIG_BLOCK * SPEC_UNROLL;
    // (the trip count is the same for the whole workgroup: the ballots run with every lane)
    for (int64_t t0 = (int64_t)blockIdx.x * TILE; t0 < n_units; t0 += (int64_t)gridDim.x * TILE) {
        uint4 v[SPEC_UNROLL], w[SPEC_UNROLL], c[SPEC_UNROLL];
#pragma unroll
        for (int q = 0; q < SPEC_UNROLL; ++q) {
            const int64_t i = t0 + (int64_t)q * BIG_BLOCK + threadIdx.x;
            v[q] = w[q] = c[q] = make_uint4(0, 0, 0, 0);
            if (i < n_units) {
                if (FORM == DUMP_PLANES) { v[q] = slots[2 * i]; w[q] = slots[2 * i + 1]; c[q] = counts[i]; }
                else v[q] = slots[i];
            }
        }
#pragma unroll
        for (int q = 0; q < SPEC_UNROLL; ++q) {
            if (FORM == DUMP_DENSE) {
                spectrum_bin<BALLOT>(bins, v[q].x, cap, ones, twos);
                spectrum_bin<BALLOT>(bins, v[q].y, cap, ones, twos);
                spectrum_bin<BALLOT>(bins, v[q].z, cap, ones, twos);
                spectrum_bin<BALLOT>(bins, v[q].w, cap, ones, twos);
            } else if (FORM == DUMP_HASH) {
                // slot = (key << 22) | count: the count is the low 22 bits of the low dword, an empty slot is all zero
                spectrum_bin<BALLOT>(bins, (v[q].x | v[q].y) ? v[q].x & (uint32_t)HASH_CMASK : 0u, cap, ones, twos);
                spectrum_bin<BALLOT>(bins, (v[q].z | v[q].w) ? v[q].z & (uint32_t)HASH_CMASK : 0u, cap, ones, twos);
            } else {
                spectrum_bin<BALLOT>(bins, (v[q].x | v[q].y) ? c[q].x : 0u, cap, ones, twos);
                spectrum_bin<BALLOT>(bins, (v[q].z | v[q].w) ? c[q].y : 0u, cap, ones, twos);
                spectrum_bin<BALLOT>(bins, (w[q].x | w[q].y) ? c[q].z : 0u, cap, ones, twos);
                spectrum_bin<BALLOT>(bins, (w[q].z | w[q].w) ? c[q].w : 0u, cap, ones, twos);
            }
        }
    }
    if ((threadIdx.x & 63) == 0) {
        if (BALLOT >= 1 && ones) atomicAdd(&bins[1], ones);
        if (BALLOT >= 2 && twos) atomicAdd(&bins[2], twos);          // (high >= 1: bin 2 exists, as the bin above `high` if need be)
    }
    lds_sync();
    for (int i = threadIdx.x; i < n_bins; i += BIG_BLOCK) {
        const uint32_t s = bins[i];
        if (s) atomicAdd(&hist[i], (unsigned long long)s);
    }
}

// -------------------------------------------------------------------------------- the table as jellyfish's text dump, and back
//
// `jellyfish dump -c -t` of the table (feature.py:87,103: the abundance.k{k}.dump the reference leaves on disk) and the reload
// of such a file (count_kmer.cpp:139-170).  One line per kept entry, "<k-mer>\t<count>\n", the first character of the k-mer from
// the highest two bits of the canonical code, A C T G for 0 1 2 3; lines in slot order.  The table is only read, by plain loads.
//
// A UNIT is PG_DUMP_UNIT_SLOTS consecutive entries: one workgroup of BLOCK lanes, DUMP_PER consecutive entries per lane (16 bytes
// of dense counters, 32 of packed slots or of keys).  Pass 1 (table_dump_sizes_kernel) leaves the text bytes of every unit, the
// caller scans them, pass 2 (table_dump_text_kernel) writes each unit's lines where the scan puts them.
constexpr int DUMP_PER = PG_DUMP_UNIT_SLOTS / BLOCK;
static_assert(DUMP_PER == 4, "a lane's entries are one 16-byte load of dense counters");
constexpr int DUMP_MAX_LINE = PG_WIDE_MAX_K + 2 + 10;                       // 31 letters, TAB, a 32-bit count, newline
constexpr int DUMP_LDS_BYTES = PG_DUMP_UNIT_SLOTS * DUMP_MAX_LINE + 16;     // (+ the text's misalignment in global memory)

__device__ __forceinline__ uint32_t dump_digits(uint32_t c)
{
    return c < 10u ? 1u : c < 100u ? 2u : c < 1000u ? 3u : c < 10000u ? 4u : c < 100000u ? 5u : c < 1000000u ? 6u
         : c < 10000000u ? 7u : c < 100000000u ? 8u : c < 1000000000u ? 9u : 10u;
}

// entries 4 * quad .. 4 * quad + 3 of the table: present (in the table at all), code (FORM's own: the index, the key, the code),
// count.  quad < n_entries / 4 (the caller's business).
template <int FORM>
__device__ __forceinline__ void dump_load(const uint4 *__restrict__ slots, const uint4 *__restrict__ counts, int64_t quad,
                                          uint64_t raw[DUMP_PER], uint32_t cnt[DUMP_PER], bool present[DUMP_PER])
{
    if (FORM == DUMP_DENSE) {
        const uint4 v = slots[quad];
        const uint32_t c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < DUMP_PER; ++q) { raw[q] = (uint64_t)(4 * quad + q); cnt[q] = c[q]; present[q] = c[q] != 0; }
    } else {
        const uint4 a = slots[2 * quad], b = slots[2 * quad + 1];
        const uint64_t s[4] = {((uint64_t)a.y << 32) | a.x, ((uint64_t)a.w << 32) | a.z, ((uint64_t)b.y << 32) | b.x, ((uint64_t)b.w << 32) | b.z};
        uint32_t c[4] = {0, 0, 0, 0};
        if (FORM == DUMP_PLANES) { const uint4 v = counts[quad]; c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w; }
#pragma unroll
        for (int q = 0; q < DUMP_PER; ++q) {
            present[q] = s[q] != 0;
            if (FORM == DUMP_PLANES) { raw[q] = s[q] - 1; cnt[q] = c[q]; }
            else { raw[q] = s[q] >> HASH_CBITS; cnt[q] = (uint32_t)(s[q] & HASH_CMASK); }
        }
    }
}

// what dump_load gave for one entry as the canonical code and the key a table of kind TK places it by: key42 of the code for a
// packed hash table -- the stored key itself where the entry comes from one --, the code for every other kind
template <int FORM, int TK> __device__ __forceinline__ void entry_of(uint64_t raw, uint64_t *code, uint64_t *key)
{
    *code = FORM == DUMP_HASH ? key42_inverse(raw) : raw;
    *key = TK != TK_HASH ? *code : FORM == DUMP_HASH ? raw : key42(*code);
}

// sum over the workgroup (BLOCK lanes) of v, and the sum over the lanes before this one; `part` = WAVES words of LDS, free again
// after the call's second barrier
__device__ __forceinline__ uint32_t dump_block_scan(uint32_t v, uint32_t *part, uint32_t *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) part[wave] = incl;
    lds_sync();
    uint32_t before = incl - v, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t t = part[w];
        if (w < wave) before += t;
        tot += t;
    }
    lds_sync();
    *total = tot;
    return before;
}

template <int FORM>
__global__ __launch_bounds__(BLOCK) void table_dump_sizes_kernel(const uint4 *__restrict__ slots, const uint4 *__restrict__ counts, int64_t n_entries,
                                                                 int64_t n_units, int k, uint64_t lower, long long *__restrict__ unit_bytes,
                                                                 long long *__restrict__ unit_lines)
{
    __shared__ uint32_t part[WAVES];
    for (int64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const int64_t quad = u * (PG_DUMP_UNIT_SLOTS / DUMP_PER) + threadIdx.x;
        uint32_t bytes = 0, lines = 0;
        if (quad * DUMP_PER < n_entries) {
            uint64_t raw[DUMP_PER];
            uint32_t cnt[DUMP_PER];
            bool present[DUMP_PER];
            dump_load<FORM>(slots, counts, quad, raw, cnt, present);
#pragma unroll
            for (int q = 0; q < DUMP_PER; ++q)
                if (present[q] && (uint64_t)cnt[q] >= lower) { bytes += (uint32_t)k + 2u + dump_digits(cnt[q]); ++lines; }
        }
        // (both sums in one scan: a unit has at most 2^10 lines of at most 43 bytes)
        uint32_t total;
        dump_block_scan((bytes << 11) | lines, part, &total);
        if (threadIdx.x == 0) {
            unit_bytes[u] = (long long)(total >> 11);
            if (unit_lines) unit_lines[u] = (long long)(total & 2047u);
        }
    }
}

// The lines of units [unit_begin, unit_end) into `text`: unit u's at byte unit_offsets[u] - text_base.  A unit is formatted in
// LDS -- every lane writes its lines behind those of the lanes before it -- and leaves by 16-byte stores: the LDS image starts at
// the misalignment of its place in global memory, so 16-byte pieces of the one are 16-byte pieces of the other; the fewer than 16
// bytes in front of the first aligned piece and behind the last go byte-wise.  No byte outside [0, range_bytes) of `text` is
// written, whatever the offsets say.
template <int FORM>
__global__ __launch_bounds__(BLOCK) void table_dump_text_kernel(const uint4 *__restrict__ slots, const uint4 *__restrict__ counts, int64_t n_entries,
                                                                int64_t unit_begin, int64_t unit_end, int k, uint64_t lower,
                                                                const long long *__restrict__ unit_offsets, int64_t text_base, int64_t range_bytes,
                                                                uint8_t *__restrict__ text)
{
    __shared__ __attribute__((aligned(16))) uint8_t img[DUMP_LDS_BYTES];
    __shared__ uint32_t part[WAVES];
    for (int64_t u = unit_begin + blockIdx.x; u < unit_end; u += gridDim.x) {
        const int64_t quad = u * (PG_DUMP_UNIT_SLOTS / DUMP_PER) + threadIdx.x;
        uint64_t raw[DUMP_PER];
        uint32_t cnt[DUMP_PER], len[DUMP_PER] = {0, 0, 0, 0};
        if (quad * DUMP_PER < n_entries) {
            bool present[DUMP_PER];
            dump_load<FORM>(slots, counts, quad, raw, cnt, present);
#pragma unroll
            for (int q = 0; q < DUMP_PER; ++q)
                if (present[q] && (uint64_t)cnt[q] >= lower) len[q] = (uint32_t)k + 2u + dump_digits(cnt[q]);
        }
        uint32_t total;
        uint32_t at = dump_block_scan(len[0] + len[1] + len[2] + len[3], part, &total);
        const int64_t dst = (int64_t)unit_offsets[u] - text_base;            // where the unit's text starts in `text`
        const uint32_t mis = (uint32_t)(((uintptr_t)text + (uint64_t)dst) & 15u);
        at += mis;
#pragma unroll
        for (int q = 0; q < DUMP_PER; ++q) {
            if (len[q] == 0) continue;
            const uint64_t code = FORM == DUMP_HASH ? key42_inverse(raw[q]) : raw[q];
            for (int j = 0; j < k; ++j) img[at + j] = (uint8_t)(0x47544341u >> (8 * ((uint32_t)(code >> (2 * (k - 1 - j))) & 3u)));   // "ACTG"
            img[at + k] = '\t';
            uint32_t c = cnt[q];
            for (uint32_t p = at + len[q] - 2; p > at + k; --p) { img[p] = (uint8_t)('0' + c % 10u); c /= 10u; }
            img[at + len[q] - 1] = '\n';
            at += len[q];
        }
        lds_sync();
        // head: up to the first 16-byte boundary of global memory; body: whole 16-byte pieces; tail: the rest
        const uint32_t head = total < ((16u - mis) & 15u) ? total : ((16u - mis) & 15u);
        const uint32_t n16 = (total - head) >> 4;
        const uint32_t tail = total - head - (n16 << 4);
        for (uint32_t i = threadIdx.x; i < n16; i += BLOCK) {
            const int64_t p = dst + head + ((int64_t)i << 4);
            if (p >= 0 && p + 16 <= range_bytes) *(uint4 *)(text + p) = *(const uint4 *)(img + mis + head + (i << 4));
        }
        if (threadIdx.x < head + tail) {
            const uint32_t o = threadIdx.x < head ? threadIdx.x : total - tail + (threadIdx.x - head);
            const int64_t p = dst + o;
            if (p >= 0 && p < range_bytes) text[p] = img[mis + o];
        }
        lds_sync();                                                       // (the image is rewritten by the next unit)
    }
}

// ---- the reload: text -> (canonical code, count, line ordinal) of every line that holds a k-mer over ACGT
//
// Tiles of BLOCK x 16 bytes, a lane owning 16 consecutive bytes.  dump_newlines_kernel counts the newlines of every tile, one
// scan turns the counts into the ordinal of each tile's first line start, dump_parse_kernel then finds the line starts of its
// tile (the byte behind a newline, and byte 0), numbers them by a scan over the lanes' newline counts and lets the lane that owns
// a line's first byte read that line -- at most 64 bytes of it; the longest legal line has 31 + 1 + 18 + 2.  A lane with several
// line starts (lines may be as short as "A\t1\n", or blank) takes them in turns of the whole wavefront: every turn ends with a
// ballot and one add to the output counter per wavefront.  Kept entries land in no particular order -- their ordinals say where
// they stood.  Semantics: cli.load_dump (pangaea_amd/cli.py), which is count_kmer.cpp:144-169 on any file jellyfish has written.
constexpr int PARSE_TILE = BLOCK * 16;

// bit i = byte i of the lane's 16 is a newline.  p0 < n; `text` is 16-byte aligned, so a full piece is one load
__device__ __forceinline__ uint32_t dump_newline_mask(const uint8_t *__restrict__ text, int64_t p0, int64_t n)
{
    uint32_t m = 0;
    if (p0 + 16 <= n) {
        const uint4 v = *(const uint4 *)(text + p0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t x = w[q] ^ 0x0A0A0A0Au;
            const uint32_t f = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);      // 0x80 in every byte that is zero
            m |= (((f >> 7) & 1u) | ((f >> 14) & 2u) | ((f >> 21) & 4u) | ((f >> 28) & 8u)) << (4 * q);
        }
    } else {
        for (int i = 0; p0 + i < n; ++i) m |= (uint32_t)(text[p0 + i] == '\n') << i;
    }
    return m;
}

__global__ __launch_bounds__(BLOCK) void dump_newlines_kernel(const uint8_t *__restrict__ text, int64_t n, int64_t n_tiles, unsigned long long *__restrict__ hist)
{
    __shared__ uint32_t part[WAVES];
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t p0 = tile * PARSE_TILE + (int64_t)threadIdx.x * 16;
        uint32_t total;
        dump_block_scan(p0 < n ? (uint32_t)__popc(dump_newline_mask(text, p0, n)) : 0u, part, &total);
        if (threadIdx.x == 0) hist[tile] = total;
    }
}

__global__ __launch_bounds__(BLOCK) void dump_parse_kernel(const uint8_t *__restrict__ text, int64_t n, int64_t n_tiles,
                                                           const unsigned long long *__restrict__ tile_first, int k, int64_t first_ordinal,
                                                           uint64_t *__restrict__ codes, uint64_t *__restrict__ counts, long long *__restrict__ ordinals,
                                                           int64_t cap, unsigned long long *__restrict__ n_out, unsigned long long *__restrict__ status)
{
    __shared__ uint32_t part[WAVES];
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) n_out[1] = tile_first[n_tiles] + (text[n - 1] != '\n');     // lines of the text
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t p0 = tile * PARSE_TILE + (int64_t)threadIdx.x * 16;
        uint32_t nl = 0, starts = 0;
        if (p0 < n) {
            nl = dump_newline_mask(text, p0, n);
            starts = ((nl << 1) | (uint32_t)(p0 == 0 || text[p0 - 1] == '\n')) & 0xffffu;
            if (p0 + 16 > n) starts &= (1u << (int)(n - p0)) - 1u;
        }
        uint32_t total;
        const uint64_t before = tile_first[tile] + dump_block_scan((uint32_t)__popc(nl), part, &total);
        for (;;) {
            const bool have = starts != 0;
            if (!__any(have)) break;
            bool keep = false;
            uint64_t canon = 0, count = 0, line = 0;
            if (have) {
                const int b = __ffs(starts) - 1;
                starts &= starts - 1;
                line = (uint64_t)first_ordinal + before + (uint64_t)__popc(nl & ((1u << b) - 1u));
                int64_t i = p0 + b;
                uint64_t fw = 0;
                int len = 0;
                bool acgt = true;
                uint32_t c = '\n';                               // (the end of the text ends a line)
                for (; i < n; ++i) {
                    c = text[i];
                    if (c == '\n' || c == '\t' || len >= 64) break;
                    if (len < 32) {
                        fw = (fw << 2) | ((c >> 1) & 3u);
                        acgt = acgt && (c == 'A' || c == 'C' || c == 'G' || c == 'T');
                    }
                    ++len;
                }
                if (i >= n) c = '\n';
                uint32_t bad = 0;
                if (c == '\n') {
                    if (!(len == 0 || (len == 1 && text[i - 1] == '\r'))) bad = PG_DUMP_NO_TAB;      // (else: a blank line)
                } else if (c != '\t' || len != k) {
                    bad = PG_DUMP_BAD_LENGTH;
                } else {
                    int nd = 0;
                    for (++i; i < n && nd <= PG_DUMP_MAX_DIGITS; ++i, ++nd) {
                        const uint32_t d = (uint32_t)text[i] - '0';
                        if (d > 9u) break;
                        count = count * 10u + d;
                    }
                    if (i < n && text[i] == '\r') ++i;
                    if (nd < 1 || nd > PG_DUMP_MAX_DIGITS || !(i >= n || text[i] == '\n')) bad = PG_DUMP_BAD_COUNT;
                    else if (acgt) {
                        const uint64_t rc = rev2_64(fw ^ 0xAAAAAAAAAAAAAAAAull) >> (64 - 2 * k);
                        canon = fw < rc ? fw : rc;
                        keep = true;
                    }
                }
                if (bad) atomicMin(status, ((unsigned long long)(line + 1) << 8) | bad);
            }
            const uint64_t m = __ballot(keep);
            if (m) {
                const int leader = __ffsll((unsigned long long)m) - 1;
                unsigned long long base = 0;
                if (lane == leader) base = atomicAdd(n_out, (unsigned long long)__popcll(m));
                base = __shfl(base, leader);
                if (keep) {
                    const uint64_t at = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
                    if (at < (uint64_t)cap) { codes[at] = canon; counts[at] = count; ordinals[at] = (long long)line; }
                    else atomicMin(status, ((unsigned long long)(line + 1) << 8) | PG_DUMP_CAPACITY);
                }
            }
        }
    }
}

// -------------------------------------------------------------------------------- merging finished tables
//
// What `jellyfish merge` gives over the tables of feature.py:76-94: one table that holds the sum of several.  Two forms.
//
// ALIGNED (table_merge_aligned_kernel): sources and destination are all MINI tables, or all bucketed HASH tables, of one geometry.
// A k-mer's bucket is a function of the k-mer and the geometry alone (a hash of its minimizer; the top bits of its key), so the
// merge is per bucket: one workgroup zeroes an LDS table of 2^log2_bucket slots, streams that bucket's slice of every source in
// turn -- 16 bytes (two slots) per lane and load, ALIGNED_PAIRS loads in flight -- adds every occupied slot with lds_merge from
// its home slot as the builders derive it, and writes the slice once (16-byte stores).  HBM sees only streams, no global atomic
// is issued.  The destination's old slice is neither read nor assumed initialised.  A bucket whose union does not fit sets
// PG_STATUS_TABLE_FULL (its slice then holds part of the union; nothing outside the slice is ever stored).
// LDS: 8 B per slot -- 128 KiB for 2^14-slot buckets (one workgroup per CU), 64 KiB and less below (two and more).
constexpr int ALIGNED_MAX_SRCS = 16;
constexpr int ALIGNED_PAIRS = 4;
struct MergeSources {
    const ulonglong2 *p[ALIGNED_MAX_SRCS];
};

// an entry's home slot inside its bucket, from the slot's high bits (hash: the key; mini: the code itself), as the builders derive it
template <bool MINI> __device__ __forceinline__ uint32_t slice_home(uint64_t code, int hsh, uint32_t smask)
{
    return (MINI ? mini_slot_hash<true>(code) : (uint32_t)(code >> hsh)) & smask;
}

// One bucket's slice of an aligned source (n_pairs 16-byte pairs of slots at `src`) past the workgroup's LDS table: ALIGNED_PAIRS
// loads in flight per lane, then the home slot and the first LDS read of all 2 * ALIGNED_PAIRS entries, then f(entry, slot, first)
// for each (an empty slot: entry 0, first 0).
template <bool MINI, class F>
__device__ __forceinline__ void stream_slice(const ulonglong2 *__restrict__ src, uint32_t n_pairs, const unsigned long long *tab, int hsh,
                                             uint32_t smask, F &&f)
{
    for (uint32_t base = 0; base < n_pairs; base += BIG_BLOCK * ALIGNED_PAIRS) {
        uint64_t e[2 * ALIGNED_PAIRS];
#pragma unroll
        for (int j = 0; j < ALIGNED_PAIRS; ++j) {
            const uint32_t i = base + (uint32_t)j * BIG_BLOCK + threadIdx.x;
            const ulonglong2 v = i < n_pairs ? src[i] : make_ulonglong2(0ull, 0ull);
            e[2 * j] = v.x;
            e[2 * j + 1] = v.y;
        }
        uint32_t ss[2 * ALIGNED_PAIRS];
        unsigned long long first[2 * ALIGNED_PAIRS];
#pragma unroll
        for (int j = 0; j < 2 * ALIGNED_PAIRS; ++j) {
            ss[j] = slice_home<MINI>(e[j] >> HASH_CBITS, hsh, smask);
            first[j] = e[j] ? tab[ss[j]] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < 2 * ALIGNED_PAIRS; ++j) f(e[j], ss[j], first[j]);
    }
}

template <bool MINI>
__global__ __launch_bounds__(BIG_BLOCK) void table_merge_aligned_kernel(MergeSources srcs, int n_srcs, HashView t, uint32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
    const uint32_t n_slots = 1u << t.log2_bucket;
    const uint32_t smask = n_slots - 1;
    const uint32_t limit = t.limit();
    const int hsh = KEY_BITS - t.log2_slots;
    const uint32_t n_pairs = n_slots >> 1;                                       // (buckets have at least 2^4 slots)
    const uint64_t first_pair = (uint64_t)blockIdx.x << (t.log2_bucket - 1);     // the bucket's slice, in 16-byte pairs of slots
    ulonglong2 *tab2 = reinterpret_cast<ulonglong2 *>(tab);
    for (uint32_t i = threadIdx.x; i < n_pairs; i += BIG_BLOCK) tab2[i] = make_ulonglong2(0ull, 0ull);
    __syncthreads();
    bool full = false;
    for (int p = 0; p < n_srcs; ++p)
        stream_slice<MINI>(srcs.p[p] + first_pair, n_pairs, tab, hsh, smask, [&](uint64_t e, uint32_t s, unsigned long long first) {
            full |= !lds_merge_entry(tab, smask, limit, e, s, first);
        });
    if (full) atomicOr(status, PG_STATUS_TABLE_FULL);
    __syncthreads();
    ulonglong2 *out = reinterpret_cast<ulonglong2 *>(t.slots) + first_pair;
    for (uint32_t i = threadIdx.x; i < n_pairs; i += BIG_BLOCK) out[i] = tab2[i];
}

// GENERAL (table_merge_kernel): any source kind into any destination kind, whatever the geometries.  The source's storage is
// streamed with the dump kernels' 16-byte loads (dump_load: four dense counters, four packed slots, or four keys with their four
// counts), MERGE_QUADS of them in flight per lane; an entry's code is the index (dense), key42_inverse of the key (hash), the
// slot's high bits (mini), key - 1 (planes).  It is ADDED to what the destination holds: atomicAdd (dense), the saturating
// compare-and-swap of kmer_merge_kernel (hash_merge_from, pg_table.hpp) placed by key42 + home_key / home_mini (hash / mini; the first probes of a lane's batch
// are issued before any is resolved, as table_query_kernel does), wide_add (wide / miniw: 32-bit sums).  A packed source's
// saturated count travels as the value it stores; a count that enters a packed table is clamped to HASH_COUNT_SAT first.
constexpr int MERGE_QUADS = 2;

template <int FORM, int TK>
__global__ __launch_bounds__(BLOCK) void table_merge_kernel(const uint4 *__restrict__ slots, const uint4 *__restrict__ counts, int64_t n_quads, int k,
                                                            uint32_t *dense, HashView t, uint32_t *status)
{
    constexpr int N = MERGE_QUADS * DUMP_PER;
    constexpr bool PACKED = TK == TK_HASH || TK == TK_MINI;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t q0 = (int64_t)blockIdx.x * BLOCK + threadIdx.x; q0 < n_quads; q0 += stride * MERGE_QUADS) {
        uint64_t code[N], key[N], hh[N], cur[N];
        uint32_t add[N];
#pragma unroll
        for (int u = 0; u < MERGE_QUADS; ++u) {
            const int64_t q = q0 + u * stride;
            uint64_t raw[DUMP_PER] = {0, 0, 0, 0};
            uint32_t cnt[DUMP_PER] = {0, 0, 0, 0};
            bool present[DUMP_PER] = {false, false, false, false};
            if (q < n_quads) dump_load<FORM>(slots, counts, q, raw, cnt, present);
#pragma unroll
            for (int j = 0; j < DUMP_PER; ++j) {
                const int i = u * DUMP_PER + j;
                add[i] = present[j] ? cnt[j] : 0u;
                if (PACKED && add[i] > HASH_SAT) add[i] = HASH_SAT;
                entry_of<FORM, TK>(raw[j], &code[i], &key[i]);
                hh[i] = cur[i] = 0;
                if (PACKED && add[i]) {
                    hh[i] = TK == TK_HASH ? t.home_key(key[i]) : t.home_mini(code[i], k);
                    cur[i] = t.slots[hh[i]];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (add[i] == 0) continue;
            if (TK == TK_DENSE) { if ((code[i] >> (2 * k)) == 0) atomicAdd(&dense[(uint32_t)code[i]], add[i]); }   // (never indexed beyond 4^k)
            else if (TK == TK_WIDE) wide_add(t, code[i], add[i], status);
            else if (TK == TK_MINIW) wide_add(t, code[i], add[i], status, k);
            else hash_merge_from(t, hh[i], cur[i], key[i], add[i], status);
        }
    }
}

// -------------------------------------------------------------------------------- combining finished tables
//
// Two tables of feature.py:76-94 met otherwise than by their sum.  For a canonical k-mer let a, b be the counts tables A and B
// STORE for it (0: absent); the result stores r where lower <= r <= upper:
//   MIN min(a, b)   MAX max(a, b)   DIFF a > b ? a - b : 0   LEFT b ? a : 0   ONLY b ? 0 : a   KEEP a (no B)
// Two forms, as for the sum.
//
// ALIGNED (table_combine_aligned_kernel): A, B and the result are all MINI tables, or all bucketed HASH tables, of one geometry;
// one workgroup per bucket, the slice is written exactly once with 16-byte stores, its old content is never read.
//   MAX: the LDS table is zeroed, A's slice and B's slice are streamed as table_merge_aligned_kernel streams them, a key that is
//        already there keeps the larger count (lds_larger).  A union that does not fit sets PG_STATUS_TABLE_FULL.
//   the others: the result is a subset of A's bucket.  A's slice is loaded into LDS, B's slice is streamed and every B entry walks
//        A's chain (read-only but for the matched slot, at most the view's limit() steps).  Each A slot is matched by at most one B
//        entry, which rewrites the slot's count to r where r > 0 -- the key bits, all a walking lane compares, stay -- and sets the
//        slot's bit of an LDS bitmap: "matched" for MIN / LEFT (no bit: b == 0, the slot dies), "dead" for DIFF / ONLY (r == 0;
//        a slot cannot be cleared in place, an emptied slot would cut the chains the other lanes are walking).
// Removing entries breaks linear-probing chains, so a bucket that loses entries is REBUILT: every lane takes its slots (at most
// 2^14 / 1024 = 16) into registers, dropping the dead ones and those outside the window, the table is zeroed, the survivors are
// inserted again with lds_merge_entry from their home slots (they fit: a subset of what fitted), and the slice is written.
// LDS: 8 B per slot + 1 bit per slot (128 KiB + 2 KiB for 2^14-slot buckets), all of it dynamic.
enum { COMBINE_MIN = PG_COMBINE_MIN, COMBINE_MAX = PG_COMBINE_MAX, COMBINE_DIFF = PG_COMBINE_DIFF, COMBINE_LEFT = PG_COMBINE_LEFT,
       COMBINE_ONLY = PG_COMBINE_ONLY, COMBINE_KEEP = PG_COMBINE_KEEP };
constexpr int COMBINE_PER_LANE = (1 << PG_BUCKET_MAX_LOG2_SLOTS) / BIG_BLOCK;
static_assert(COMBINE_PER_LANE == 16, "a lane holds its share of the largest bucket in registers while the bucket is rebuilt");

// r of the table above for an entry of A (a > 0)
__device__ __forceinline__ uint32_t combine_result(int op, uint32_t a, uint32_t b)
{
    switch (op) {
    case COMBINE_MIN: return a < b ? a : b;
    case COMBINE_MAX: return a > b ? a : b;
    case COMBINE_DIFF: return a > b ? a - b : 0u;
    case COMBINE_LEFT: return b ? a : 0u;
    case COMBINE_ONLY: return b ? 0u : a;
    default: return a;
    }
}

// lds_merge with "the larger count" in place of the saturating sum
__device__ __forceinline__ bool lds_larger(unsigned long long *tab, uint32_t smask, uint32_t limit, uint64_t e, uint32_t s, unsigned long long cur)
{
    if (e == 0) return true;
    const uint64_t code = e >> HASH_CBITS;
    uint32_t cnt = (uint32_t)(e & HASH_CMASK);
    if (cnt > HASH_SAT) cnt = HASH_SAT;
    for (uint32_t tries = 0; tries < limit; ++tries) {
        for (;;) {
            if (cur != 0 && (cur >> HASH_CBITS) != code) break;
            const uint32_t have = (uint32_t)(cur & HASH_CMASK);
            if (cur != 0 && have >= cnt) return true;
            const unsigned long long old = atomicCAS(&tab[s], cur, (unsigned long long)((code << HASH_CBITS) | cnt));
            if (old == cur) return true;
            cur = old;
        }
        s = (s + 1) & smask;
        cur = tab[s];
    }
    return false;
}

template <bool MINI>
__global__ __launch_bounds__(BIG_BLOCK) void table_combine_aligned_kernel(const ulonglong2 *__restrict__ a, const ulonglong2 *__restrict__ b, int op,
                                                                          uint64_t lower, uint64_t upper, HashView t, uint32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
    const uint32_t n_slots = 1u << t.log2_bucket;
    const uint32_t smask = n_slots - 1;
    const uint32_t limit = t.limit();
    const int hsh = KEY_BITS - t.log2_slots;
    const uint32_t n_pairs = n_slots >> 1;                                       // (buckets have at least 2^4 slots)
    const uint64_t first_pair = (uint64_t)blockIdx.x << (t.log2_bucket - 1);     // the bucket's slice, in 16-byte pairs of slots
    const uint32_t n_flag_words = (n_slots + 31) >> 5;
    uint32_t *flags = reinterpret_cast<uint32_t *>(tab + n_slots);               // one bit per slot, behind the table
    ulonglong2 *tab2 = reinterpret_cast<ulonglong2 *>(tab);
    ulonglong2 *out = reinterpret_cast<ulonglong2 *>(t.slots) + first_pair;
    a += first_pair;
    if (b) b += first_pair;
    if (op == COMBINE_MAX) {
        for (uint32_t i = threadIdx.x; i < n_pairs; i += BIG_BLOCK) tab2[i] = make_ulonglong2(0ull, 0ull);
        __syncthreads();
        bool full = false;
        for (int p = 0; p < 2; ++p)
            stream_slice<MINI>(p ? b : a, n_pairs, tab, hsh, smask, [&](uint64_t e, uint32_t s, unsigned long long first) {
                if (e & HASH_CMASK) full |= !lds_larger(tab, smask, limit, e, s, first);
            });
        if (full) atomicOr(status, PG_STATUS_TABLE_FULL);
        __syncthreads();
        if (lower <= 1 && upper >= HASH_CMASK) {                                 // (the same for the whole grid) nothing leaves: no rebuild
            for (uint32_t i = threadIdx.x; i < n_pairs; i += BIG_BLOCK) out[i] = tab2[i];
            return;
        }
    } else {
        for (uint32_t i = threadIdx.x; i < n_pairs; i += BIG_BLOCK) tab2[i] = a[i];
        for (uint32_t i = threadIdx.x; i < n_flag_words; i += BIG_BLOCK) flags[i] = 0u;
        __syncthreads();
        if (b) {
            // (`cur`, read before the walks of this batch began, may be stale in its count alone, and only where another lane has
            // matched that slot: then the key differs from this entry's and the count is not looked at)
            stream_slice<MINI>(b, n_pairs, tab, hsh, smask, [&](uint64_t e, uint32_t s, unsigned long long cur) {
                const uint32_t cb = (uint32_t)(e & HASH_CMASK);
                if (cb == 0) return;                                             // (an empty slot; a stored count of 0 is b == 0)
                const uint64_t code = e >> HASH_CBITS;
                for (uint32_t tries = 0; tries < limit && cur != 0; ++tries) {
                    if ((cur >> HASH_CBITS) == code) {
                        const uint32_t r = combine_result(op, (uint32_t)(cur & HASH_CMASK), cb);
                        if (r) tab[s] = (unsigned long long)((code << HASH_CBITS) | r);
                        if (op == COMBINE_MIN || op == COMBINE_LEFT || r == 0) atomicOr(&flags[s >> 5], 1u << (s & 31));
                        return;
                    }
                    s = (s + 1) & smask;
                    cur = tab[s];
                }
            });
            __syncthreads();
        }
    }
    // the rebuild: survivors into registers, an empty table, every survivor in again from its home slot
    const bool marked_live = op == COMBINE_MIN || op == COMBINE_LEFT;
    const bool use_flags = op != COMBINE_MAX && op != COMBINE_KEEP;
    uint64_t v[COMBINE_PER_LANE];
#pragma unroll
    for (int j = 0; j < COMBINE_PER_LANE; ++j) {
        const uint32_t i = (uint32_t)j * BIG_BLOCK + threadIdx.x;
        uint64_t x = i < n_slots ? tab[i] : 0ull;
        if (x != 0 && use_flags && (((flags[i >> 5] >> (i & 31)) & 1u) != 0) != marked_live) x = 0ull;
        const uint64_t c = x & HASH_CMASK;
        if (c < lower || c > upper) x = 0ull;                                    // (lower >= 1: a count of 0 never stays)
        v[j] = x;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_pairs; i += BIG_BLOCK) tab2[i] = make_ulonglong2(0ull, 0ull);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < COMBINE_PER_LANE; ++j) {
        if (v[j] == 0) continue;
        const uint32_t s = slice_home<MINI>(v[j] >> HASH_CBITS, hsh, smask);
        lds_merge_entry(tab, smask, limit, v[j], s, tab[s]);                     // (always finds room: fewer entries than the bucket held)
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_pairs; i += BIG_BLOCK) out[i] = tab2[i];
}

// GENERAL (table_combine_items_kernel): any kind against any kind, whatever the geometries.  A's storage is streamed as
// table_merge_kernel streams a source (dump_load, MERGE_QUADS 16-byte loads in flight per lane); every entry of A is looked up in B
// as table_query_kernel looks a code up -- the first probes of a lane's batch issued before any is resolved, hash_probe / wide_probe,
// dense by index; TK_NONE: no B, b = 0 --, r is computed, and the entries inside the window leave as (canonical code, count) items
// through one cursor.  The cursor is aggregated further than table_compact_kernel's ballot per turn: a lane counts the survivors
// of its batch (at most 8), the workgroup scans the counts (dump_block_scan) and claims its range with ONE 64-bit atomic add per
// batch -- 2^29 slots are 2^18 adds on the one word; one add per wavefront and turn, 2^23 of them, took 90 ms of a 113 ms
// combine on the bench tables.  An item past `cap` is not stored and sets PG_STATUS_OVERFLOW_LIST; the cursor goes on counting.  The destination's kind is no
// template axis: the result table is built from the items by the inserts the library has (pg_kmer_merge, pg_kmer_merge_wide).
// MAX over both tables is two launches: A against B with MAX, B against A with ONLY.

// entries q, q + stride, .. (MERGE_QUADS quads) of A with B's count of each: code = the canonical code, ca = A's count (0: no
// entry), cb = B's count (0: not in B)
template <int FORM, int TK>
__device__ __forceinline__ void combine_load_probe(const uint4 *__restrict__ slots, const uint4 *__restrict__ counts, int64_t q0, int64_t stride,
                                                   int64_t n_quads, int k, const uint32_t *__restrict__ dense_b, const HashView &b,
                                                   uint64_t (&code)[MERGE_QUADS * DUMP_PER], uint32_t (&ca)[MERGE_QUADS * DUMP_PER],
                                                   uint32_t (&cb)[MERGE_QUADS * DUMP_PER])
{
    constexpr int N = MERGE_QUADS * DUMP_PER;
    Lookup<TK> p[N];
#pragma unroll
    for (int u = 0; u < MERGE_QUADS; ++u) {
        const int64_t q = q0 + u * stride;
        uint64_t raw[DUMP_PER] = {0, 0, 0, 0};
        uint32_t cnt[DUMP_PER] = {0, 0, 0, 0};
        bool present[DUMP_PER] = {false, false, false, false};
        if (q < n_quads) dump_load<FORM>(slots, counts, q, raw, cnt, present);
#pragma unroll
        for (int j = 0; j < DUMP_PER; ++j) {
            const int i = u * DUMP_PER + j;
            ca[i] = present[j] ? cnt[j] : 0u;
            uint64_t key;
            entry_of<FORM, TK>(raw[j], &code[i], &key);
            p[i].key = p[i].hh = p[i].cur = 0;
            if (ca[i] == 0 || (TK == TK_DENSE && (code[i] >> (2 * k)) != 0)) continue;         // (never indexed beyond 4^k: b = 0)
            p[i].issue_key(code[i], key, k, dense_b, b);
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) cb[i] = ca[i] ? p[i].resolve(b) : 0u;
}

template <int FORM, int TK>
__global__ __launch_bounds__(BLOCK) void table_combine_items_kernel(const uint4 *__restrict__ slots, const uint4 *__restrict__ counts, int64_t n_quads,
                                                                    int k, const uint32_t *__restrict__ dense_b, HashView b, int op, uint64_t lower,
                                                                    uint64_t upper, uint64_t *__restrict__ out_codes, uint32_t *__restrict__ out_counts,
                                                                    unsigned long long cap, unsigned long long *__restrict__ n_out, uint32_t *status)
{
    constexpr int N = MERGE_QUADS * DUMP_PER;
    __shared__ uint32_t part[WAVES];
    __shared__ unsigned long long cursor;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    // (the trip count is the same for the whole workgroup: the scan and its barriers run with every lane)
    for (int64_t base = (int64_t)blockIdx.x * BLOCK; base < n_quads; base += stride * MERGE_QUADS) {
        uint64_t code[N];
        uint32_t ca[N], cb[N];
        combine_load_probe<FORM, TK>(slots, counts, base + threadIdx.x, stride, n_quads, k, dense_b, b, code, ca, cb);
        uint32_t mine = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const uint32_t r = ca[i] ? combine_result(op, ca[i], cb[i]) : 0u;
            ca[i] = r != 0 && r >= lower && r <= upper ? r : 0u;                 // (from here on: the count that leaves, 0 = none)
            mine += ca[i] != 0;
        }
        uint32_t total;
        const uint32_t before = dump_block_scan(mine, part, &total);
        if (total == 0) continue;                                                // (the same for the whole workgroup)
        if (threadIdx.x == 0) cursor = atomicAdd(n_out, (unsigned long long)total);
        lds_sync();                                                              // (the next write of `cursor` lies behind the scan's barriers)
        unsigned long long pos = cursor + before;
        bool over = false;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (ca[i] == 0) continue;
            if (pos < cap) {
                out_codes[pos] = code[i];
                out_counts[pos] = ca[i];
            } else {
                over = true;
            }
            ++pos;
        }
        if (over) atomicOr(status, PG_STATUS_OVERFLOW_LIST);
    }
}

// COMPARE (table_compare_kernel): the same pass over A with B probed, no output but four 64-bit sums -- out[0] += A's entries,
// out[1] += A's total count, out[2] += entries B holds too, out[3] += the sum of min(a, b).  A lane sums in registers, a wavefront
// by shuffles, the workgroup in LDS, and each workgroup leaves with one global 64-bit add per value (integer sums: the same
// whatever the order), as table_spectrum_kernel leaves its bins.
template <int FORM, int TK>
__global__ __launch_bounds__(BLOCK) void table_compare_kernel(const uint4 *__restrict__ slots, const uint4 *__restrict__ counts, int64_t n_quads, int k,
                                                              const uint32_t *__restrict__ dense_b, HashView b, unsigned long long *__restrict__ out)
{
    constexpr int N = MERGE_QUADS * DUMP_PER;
    __shared__ unsigned long long part[4];
    if (threadIdx.x < 4) part[threadIdx.x] = 0ull;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    unsigned long long acc[4] = {0ull, 0ull, 0ull, 0ull};
    for (int64_t base = (int64_t)blockIdx.x * BLOCK; base < n_quads; base += stride * MERGE_QUADS) {
        uint64_t code[N];
        uint32_t ca[N], cb[N];
        combine_load_probe<FORM, TK>(slots, counts, base + threadIdx.x, stride, n_quads, k, dense_b, b, code, ca, cb);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (ca[i] == 0) continue;
            acc[0] += 1ull;
            acc[1] += ca[i];
            if (cb[i]) {
                acc[2] += 1ull;
                acc[3] += ca[i] < cb[i] ? ca[i] : cb[i];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t lo = (uint32_t)acc[j], hi = (uint32_t)(acc[j] >> 32);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned long long o = ((unsigned long long)(uint32_t)__shfl_down((int)hi, d) << 32) | (uint32_t)__shfl_down((int)lo, d);
            const unsigned long long s = (((unsigned long long)hi << 32) | lo) + o;
            lo = (uint32_t)s;
            hi = (uint32_t)(s >> 32);
        }
        if ((threadIdx.x & 63) == 0) atomicAdd(&part[j], ((unsigned long long)hi << 32) | lo);
    }
    __syncthreads();
    if (threadIdx.x < 4 && part[threadIdx.x]) atomicAdd(&out[threadIdx.x], part[threadIdx.x]);
}

// -------------------------------------------------------------------------------- depth of sequences in a finished table
//
// What `jellyfish query -s FILE` answers (the multiplicity of every k-mer of a sequence; feature.py:87's table) and the per-range
// numbers that stand beside the reference's contig depth (scripts/bin_assembly.sh:43, cut at scripts/low_abd_reads.sh:10).  The
// table is only read: plain loads, no atomics on it.
//
// One LANE per stream position here, not one lane per word as in the counting kernels: a lane takes the k characters that start
// at its position straight out of the one or two stream words that hold them (k <= 31), so a range of 150 characters keeps 130
// lanes busy instead of 5, nothing is pre-rolled, and the answers of a wavefront are 64 consecutive words.  The stream words are
// read 32 times over, from L1.

// the canonical k-mer that starts at character i; false where one of its characters is not set in `valid`.  The caller has made
// sure that 0 <= i and i + k <= n_chars: the second word is read only when the k-mer reaches into it.
__device__ __forceinline__ bool kmer_at(const uint64_t *__restrict__ codes, const uint32_t *__restrict__ valid, int64_t i, int k, uint64_t kmask,
                                        uint64_t *canon)
{
    const int64_t w = i >> 5;
    const int s = (int)(i & 31);
    uint64_t c = codes[w] >> (2 * s), v = valid[w] >> s;
    if (s + k > 32) {                                      // (then s >= 2: both shifts below are in range)
        c |= codes[w + 1] << (64 - 2 * s);
        v |= (uint64_t)valid[w + 1] << (32 - s);
    }
    const uint64_t vm = (1ull << k) - 1;
    if ((v & vm) != vm) return false;
    c &= kmask;
    // the stream keeps the OLDEST character lowest, a code the newest: the forward code is the window reversed, the reverse
    // complement (Roller::rc: complement = ^ 2, order reversed) is the window complemented
    const uint64_t fw = rev2_64(c) >> (64 - 2 * k), rc = (c ^ 0xAAAAAAAAAAAAAAAAull) & kmask;
    *canon = fw < rc ? fw : rc;
    return true;
}

constexpr int DEPTH_BATCH = 8;              // lookups a lane has in flight
static_assert(PG_DEPTH_SHORT_MAX == 64 * DEPTH_BATCH, "a short range is one batch of one wavefront");

// out[g] = count of the k-mer that starts at character begin + g, PG_PROFILE_NONE where none does (g < n; the launcher has
// checked 0 <= begin and begin + n <= n_chars)
template <int TK>
__device__ __forceinline__ void profile_span(const uint64_t *__restrict__ codes, const uint32_t *__restrict__ valid, int64_t n_chars,
                                             int64_t begin, int64_t n, int64_t g_first, int64_t stride, int k, const uint32_t *__restrict__ dense,
                                             const HashView &t, uint32_t *__restrict__ out)
{
    const uint64_t kmask = low_mask<uint64_t>(k);
    for (int64_t g0 = g_first; g0 < n; g0 += stride * DEPTH_BATCH) {
        Lookup<TK> p[DEPTH_BATCH];
        bool ask[DEPTH_BATCH];
#pragma unroll
        for (int u = 0; u < DEPTH_BATCH; ++u) {
            const int64_t g = g0 + u * stride, i = begin + g;
            uint64_t canon = 0;
            p[u].key = p[u].hh = p[u].cur = 0;
            ask[u] = g < n && i + k <= n_chars && kmer_at(codes, valid, i, k, kmask, &canon);
            if (ask[u]) p[u].issue(canon, k, dense, t);
        }
#pragma unroll
        for (int u = 0; u < DEPTH_BATCH; ++u) {
            const int64_t g = g0 + u * stride;
            if (g < n) out[g] = ask[u] ? p[u].resolve(t) : PG_PROFILE_NONE;
        }
    }
}

template <int TK>
__global__ __launch_bounds__(BLOCK) void table_profile_kernel(const uint64_t *__restrict__ codes, const uint32_t *__restrict__ valid, int64_t n_chars,
                                                              int64_t begin, int64_t n, int k, const uint32_t *__restrict__ dense, HashView t,
                                                              uint32_t *__restrict__ out)
{
    profile_span<TK>(codes, valid, n_chars, begin, n, (int64_t)blockIdx.x * BLOCK + threadIdx.x, (int64_t)gridDim.x * BLOCK, k, dense, t, out);
}

// A LONG range (more than PG_DEPTH_SHORT_MAX characters after clipping) as the workspace lists it: its n = length - k + 1
// positions keep their counts in words [off, off + n) of the workspace's count area.  The list grows DOWN from the end of the
// workspace, the counts grow UP from behind the head, and one 64-bit word of the head holds both cursors -- entries in its top
// DEPTH_LIST_BITS bits, count words below --, so ONE atomic add hands out both and entry e's words lie behind entry e - 1's: the
// list is sorted by `off`, whatever order the wavefronts arrive in.  (An add, not a compare-and-swap: 12 000 wavefronts that
// retry on one word took 85 ms to list 12 000 ranges.)  A range whose entry or words would not fit writes neither and sets
// PG_STATUS_DEPTH_WORKSPACE; the cursors have moved all the same, so the list then has a hole, and the two kernels of the long
// form do NOTHING once that bit is set.  (Which entry a range becomes depends on the order of arrival; its results do not.)
struct DepthLong {
    int64_t range, start, off, n;
};
constexpr int DEPTH_LIST_BITS = 24, DEPTH_OFF_BITS = 64 - DEPTH_LIST_BITS;
constexpr uint64_t DEPTH_OFF_MASK = (1ull << DEPTH_OFF_BITS) - 1;
constexpr int64_t DEPTH_HEAD_BYTES = 256;
__device__ __forceinline__ const DepthLong *depth_entry(const void *ws, int64_t ws_bytes, uint64_t e)
{
    return reinterpret_cast<const DepthLong *>((const char *)ws + ws_bytes) - 1 - e;
}

// SHORT form: one wavefront per range, grid-stride.  The lane's up to DEPTH_BATCH values stay in registers; the five results
// come from ballots and wavefront reductions, the lower median from a search over the bits of the value (how many values lie
// below the candidate: one ballot per register and bit).  40 bytes leave per range, nothing else.  A long range is only entered
// in the workspace's list here.
template <int TK>
__global__ __launch_bounds__(BLOCK) void depth_short_kernel(const uint64_t *__restrict__ codes, const uint32_t *__restrict__ valid, int64_t n_chars,
                                                            const int64_t *__restrict__ range_start, const int64_t *__restrict__ range_end,
                                                            int64_t n_ranges, int k, uint64_t lower, const uint32_t *__restrict__ dense, HashView t,
                                                            long long *__restrict__ out, void *ws, int64_t ws_bytes, uint32_t *status)
{
    const int lane = threadIdx.x & 63;
    const uint64_t kmask = low_mask<uint64_t>(k);
    const int64_t n_waves = (int64_t)gridDim.x * WAVES;
    for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < n_ranges; r += n_waves) {
        int64_t a = range_start[r], b = range_end[r];
        a = a < 0 ? 0 : a > n_chars ? n_chars : a;          // (outside the contract: clipped, so that nothing outside the stream is read)
        b = b < 0 ? 0 : b > n_chars ? n_chars : b;
        const int64_t n_pos = b - a >= k ? b - a - k + 1 : 0;
        long long *o = out + 5 * r;
        if (b - a > PG_DEPTH_SHORT_MAX) {
            if (lane == 0) {
                const unsigned long long old = atomicAdd((unsigned long long *)ws, (1ull << DEPTH_OFF_BITS) | (unsigned long long)n_pos);
                const uint64_t e = old >> DEPTH_OFF_BITS, off = old & DEPTH_OFF_MASK;
                // (n_pos <= n_chars < 2^37: the sum below cannot wrap.  Cursors that have run over their fields -- more than
                // 2^24 entries or 2^40 words asked for -- have failed this test on the way there, and the bit stays set.)
                if (e + 1 < (1ull << DEPTH_LIST_BITS) && off + (uint64_t)n_pos <= DEPTH_OFF_MASK &&
                    (uint64_t)DEPTH_HEAD_BYTES + 4 * (off + (uint64_t)n_pos) + sizeof(DepthLong) * (e + 1) <= (uint64_t)ws_bytes) {
                    DepthLong *d = const_cast<DepthLong *>(depth_entry(ws, ws_bytes, e));
                    d->range = r; d->start = a; d->off = (int64_t)off; d->n = n_pos;
                } else {
                    atomicOr(status, PG_STATUS_DEPTH_WORKSPACE);
                    o[0] = o[1] = o[2] = o[3] = o[4] = 0;
                }
            }
            continue;
        }
        uint32_t val[DEPTH_BATCH];
        Lookup<TK> p[DEPTH_BATCH];
        bool have[DEPTH_BATCH];
#pragma unroll
        for (int u = 0; u < DEPTH_BATCH; ++u) {
            const int64_t g = lane + 64 * u;
            uint64_t canon = 0;
            p[u].key = p[u].hh = p[u].cur = 0;
            have[u] = g < n_pos && kmer_at(codes, valid, a + g, k, kmask, &canon);
            if (have[u]) p[u].issue(canon, k, dense, t);
        }
        uint32_t n = 0, present = 0, vmax = 0;
        unsigned long long sum = 0;
#pragma unroll
        for (int u = 0; u < DEPTH_BATCH; ++u) {
            uint32_t c = have[u] ? p[u].resolve(t) : 0u;
            if (c < lower) c = 0;
            val[u] = c;
            n += (uint32_t)__popcll(__ballot(have[u]));
            present += (uint32_t)__popcll(__ballot(c > 0));
            sum += c;
            vmax = c > vmax ? c : vmax;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            sum += __shfl_xor(sum, d);
            const uint32_t m = __shfl_xor(vmax, d);
            vmax = m > vmax ? m : vmax;
        }
        // the value at sorted index (n - 1) / 2: the largest x with fewer than (n - 1) / 2 + 1 values below it
        uint32_t median = 0;
        if (vmax) {
            const uint32_t mid = (n - 1) / 2;
            for (int bit = 31 - __clz((int)vmax); bit >= 0; --bit) {
                const uint32_t cand = median | (1u << bit);
                uint32_t below = 0;
#pragma unroll
                for (int u = 0; u < DEPTH_BATCH; ++u) below += (uint32_t)__popcll(__ballot(have[u] && val[u] < cand));
                if (below <= mid) median = cand;
            }
        }
        if (lane == 0) {
            o[0] = n; o[1] = present; o[2] = (long long)sum; o[3] = vmax; o[4] = median;
        }
    }
}

// LONG form, first half: the counts of every listed range go to the workspace once, 4 bytes per position (PG_PROFILE_NONE where
// no k-mer starts).  The count words of all ranges are one flat array; a workgroup takes tiles of it, finds the entry its tile
// begins in (a search over the sorted list, the same for every lane) and walks on from there -- a long range has hundreds of
// positions, so a tile meets a handful.
constexpr int64_t DEPTH_TILE = (int64_t)BLOCK * DEPTH_BATCH;
template <int TK>
__global__ __launch_bounds__(BLOCK) void depth_fill_kernel(const uint64_t *__restrict__ codes, const uint32_t *__restrict__ valid, int64_t n_chars,
                                                           const void *ws, int64_t ws_bytes, int k, const uint32_t *__restrict__ dense, HashView t,
                                                           const uint32_t *status)
{
    if (*status & PG_STATUS_DEPTH_WORKSPACE) return;        // (the list has a hole: depth_short_kernel)
    const unsigned long long head = *(const unsigned long long *)ws;
    const int64_t n_long = (int64_t)(head >> DEPTH_OFF_BITS), total = (int64_t)(head & DEPTH_OFF_MASK);
    uint32_t *counts = (uint32_t *)((char *)const_cast<void *>(ws) + DEPTH_HEAD_BYTES);
    const uint64_t kmask = low_mask<uint64_t>(k);
    for (int64_t t0 = (int64_t)blockIdx.x * DEPTH_TILE; t0 < total; t0 += (int64_t)gridDim.x * DEPTH_TILE) {
        int64_t lo = 0, hi = n_long - 1;                    // the last entry whose off <= t0
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (depth_entry(ws, ws_bytes, (uint64_t)mid)->off <= t0) lo = mid;
            else hi = mid - 1;
        }
        Lookup<TK> p[DEPTH_BATCH];
        bool ask[DEPTH_BATCH];
        int64_t e = lo;
        DepthLong d = *depth_entry(ws, ws_bytes, (uint64_t)e);
#pragma unroll
        for (int u = 0; u < DEPTH_BATCH; ++u) {
            const int64_t g = t0 + u * BLOCK + threadIdx.x;
            uint64_t canon = 0;
            p[u].key = p[u].hh = p[u].cur = 0;
            ask[u] = false;
            if (g >= total) continue;
            while (g >= d.off + d.n) d = *depth_entry(ws, ws_bytes, (uint64_t)++e);
            const int64_t i = d.start + (g - d.off);
            ask[u] = i >= 0 && i + k <= n_chars && kmer_at(codes, valid, i, k, kmask, &canon);
            if (ask[u]) p[u].issue(canon, k, dense, t);
        }
#pragma unroll
        for (int u = 0; u < DEPTH_BATCH; ++u) {
            const int64_t g = t0 + u * BLOCK + threadIdx.x;
            if (g < total) counts[g] = ask[u] ? p[u].resolve(t) : PG_PROFILE_NONE;
        }
    }
}

// LONG form, second half: one workgroup per listed range reads the range's words -- once for n_kmers, n_present, sum and max,
// then once per digit of the value for the lower median: a radix select from the top, DEPTH_DIGIT_BITS bits at a time with a
// histogram in LDS, keeping only the values that agree with the digits already chosen.  Digits above the maximum are all zero
// and take no pass: packed tables (counts <= PG_HASH_COUNT_SAT = 2^21) need two at most, spectra of real reads one.  64-bit
// bins (16 KiB of LDS): a range may have more than 2^32 positions.  A lane gathers equal digits that follow each other before
// it adds to LDS -- most values of a real range are 0 or one small number, and 64 lanes adding to one bin take turns.
constexpr int DEPTH_DIGIT_BITS = 11, DEPTH_BINS = 1 << DEPTH_DIGIT_BITS;
static_assert(DEPTH_BINS % 64 == 0, "wavefront 0 scans the bins, a whole number per lane");

__device__ __forceinline__ unsigned long long depth_block_sum(unsigned long long v, unsigned long long *part)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < BIG_BLOCK / 64; ++w) s += part[w];
    __syncthreads();
    return s;
}
__device__ __forceinline__ unsigned long long depth_block_max(unsigned long long v, unsigned long long *part)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < BIG_BLOCK / 64; ++w) s = part[w] > s ? part[w] : s;
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(BIG_BLOCK) void depth_select_kernel(const void *ws, int64_t ws_bytes, uint64_t lower, long long *__restrict__ out,
                                                                 const uint32_t *status)
{
    __shared__ unsigned long long hist[DEPTH_BINS];
    __shared__ unsigned long long part[BIG_BLOCK / 64];
    __shared__ unsigned long long chosen[2];                // the digit wavefront 0 chose, and the rank left inside its bin
    if (*status & PG_STATUS_DEPTH_WORKSPACE) return;        // (the list has a hole: depth_short_kernel)
    const unsigned long long head = *(const unsigned long long *)ws;
    const int64_t n_long = (int64_t)(head >> DEPTH_OFF_BITS);
    const uint32_t *counts = (const uint32_t *)((const char *)ws + DEPTH_HEAD_BYTES);
    const int lane = threadIdx.x & 63;
    for (int64_t e = blockIdx.x; e < n_long; e += gridDim.x) {
        const DepthLong d = *depth_entry(ws, ws_bytes, (uint64_t)e);
        const uint32_t *v = counts + d.off;
        unsigned long long n = 0, present = 0, sum = 0, vmax = 0;
        for (int64_t i0 = threadIdx.x; i0 < d.n; i0 += (int64_t)BIG_BLOCK * DEPTH_BATCH) {
            uint32_t c[DEPTH_BATCH];                         // (all loads of the batch first: one in flight per lane read 8 GB/s)
#pragma unroll
            for (int u = 0; u < DEPTH_BATCH; ++u) c[u] = i0 + u * BIG_BLOCK < d.n ? v[i0 + u * BIG_BLOCK] : PG_PROFILE_NONE;
#pragma unroll
            for (int u = 0; u < DEPTH_BATCH; ++u) {
                if (c[u] == PG_PROFILE_NONE) continue;
                if (c[u] < lower) c[u] = 0;
                ++n;
                present += c[u] > 0;
                sum += c[u];
                vmax = c[u] > vmax ? c[u] : vmax;
            }
        }
        n = depth_block_sum(n, part);
        present = depth_block_sum(present, part);
        sum = depth_block_sum(sum, part);
        vmax = depth_block_max(vmax, part);
        uint32_t prefix = 0, known = 0;                      // the median's digits chosen so far, and the mask of their bits
        unsigned long long rank = n ? (n - 1) / 2 : 0;
#pragma unroll 1
        for (int shift = 2 * DEPTH_DIGIT_BITS; shift >= 0 && vmax; shift -= DEPTH_DIGIT_BITS) {
            if ((vmax >> shift) == 0) continue;              // (every value has 0 in this digit and above)
            for (int i = threadIdx.x; i < DEPTH_BINS; i += BIG_BLOCK) hist[i] = 0;
            __syncthreads();
            uint32_t run_digit = 0;
            unsigned long long run = 0;
            for (int64_t i0 = threadIdx.x; i0 < d.n; i0 += (int64_t)BIG_BLOCK * DEPTH_BATCH) {
                uint32_t c[DEPTH_BATCH];
#pragma unroll
                for (int u = 0; u < DEPTH_BATCH; ++u) c[u] = i0 + u * BIG_BLOCK < d.n ? v[i0 + u * BIG_BLOCK] : PG_PROFILE_NONE;
#pragma unroll
                for (int u = 0; u < DEPTH_BATCH; ++u) {
                    if (c[u] == PG_PROFILE_NONE) continue;
                    if (c[u] < lower) c[u] = 0;
                    if ((c[u] & known) != prefix) continue;
                    const uint32_t digit = (c[u] >> shift) & (DEPTH_BINS - 1);
                    if (digit != run_digit) {
                        if (run) atomicAdd(&hist[run_digit], run);
                        run_digit = digit;
                        run = 0;
                    }
                    ++run;
                }
            }
            if (run) atomicAdd(&hist[run_digit], run);
            __syncthreads();
            if (threadIdx.x < 64) {
                constexpr int PER = DEPTH_BINS / 64;
                unsigned long long mine = 0;
#pragma unroll 1
                for (int j = 0; j < PER; ++j) mine += hist[lane * PER + j];
                unsigned long long incl = mine;
#pragma unroll
                for (int s = 1; s < 64; s <<= 1) {
                    const unsigned long long o = __shfl_up(incl, s);
                    if (lane >= s) incl += o;
                }
                unsigned long long before = incl - mine;
                if (before <= rank && rank < incl) {         // exactly one lane: rank < the values that take part
                    int j = 0;
#pragma unroll 1
                    for (; j < PER - 1 && before + hist[lane * PER + j] <= rank; ++j) before += hist[lane * PER + j];
                    chosen[0] = (unsigned long long)(lane * PER + j);
                    chosen[1] = rank - before;
                }
            }
            __syncthreads();
            prefix |= (uint32_t)chosen[0] << shift;
            known |= (uint32_t)(DEPTH_BINS - 1) << shift;
            rank = chosen[1];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            long long *o = out + 5 * d.range;
            o[0] = (long long)n; o[1] = (long long)present; o[2] = (long long)sum; o[3] = (long long)vmax; o[4] = (long long)prefix;
        }
    }
}

// -------------------------------------------------------------------------------- reads of a FASTQ text by their k-mers' counts
//
// What `kmc_tools filter` / khmer's filter-abund answer from a table and a FASTQ file, and the k-mer counterpart of the read set
// that scripts/low_abd_reads.sh:10 (extract_unmapped.cpp) pulls out by alignment: per record how many k-mers its sequence line
// holds and how many of them the table counts inside [lower, upper], and the kept records copied byte for byte.  The kernels
// work on the TEXT (the packed stream keeps barcode runs, no read boundaries, names or qualities); semantics: the header's
// section of the same name.  The table is only read: plain loads, no atomics on it.

// ---- 1. the line index: line_start[j] = byte offset of line j's first character, line_start[lines] = n.  The tiles and the
// newline mask are the dump reload's (dump_newlines_kernel counts, scan_kernel numbers the tiles); a lane that owns newlines
// writes the start of the line behind each.  Nothing is stored at or beyond `cap`.
__global__ __launch_bounds__(BLOCK) void fastq_lines_kernel(const uint8_t *__restrict__ text, int64_t n, int64_t n_tiles,
                                                            const unsigned long long *__restrict__ tile_first, long long *__restrict__ line_start,
                                                            int64_t cap, long long *__restrict__ n_lines)
{
    __shared__ uint32_t part[WAVES];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t nl = (int64_t)tile_first[n_tiles], lines = nl + (text[n - 1] != '\n');     // (a last line without newline is a line)
        *n_lines = lines;
        if (cap > 0) line_start[0] = 0;
        if (lines > nl && lines < cap) line_start[lines] = n;
    }
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t p0 = tile * PARSE_TILE + (int64_t)threadIdx.x * 16;
        uint32_t nl = p0 < n ? dump_newline_mask(text, p0, n) : 0u;
        uint32_t total;
        int64_t at = (int64_t)tile_first[tile] + dump_block_scan((uint32_t)__popc(nl), part, &total) + 1;
        while (nl) {
            const int b = __ffs(nl) - 1;
            nl &= nl - 1;
            if (at < cap) line_start[at] = p0 + b + 1;
            ++at;
        }
    }
}

// ---- 2. (k-mers, hits) of every record.  One wavefront per record, grid-stride, as depth_short_kernel takes a range.  A batch is
// 64 x DEPTH_BATCH positions of the sequence line: the wavefront reads the HITS_CHARS characters those positions reach (the
// batch's own and the k - 1 <= 30 behind them, in whole words; the next batch reads its overlap again, from L1), one byte per
// lane and turn, and composes them into the stream's word form in its own corner of LDS -- 2-bit codes (ch >> 1) & 3, oldest
// character lowest, 32 to a word, and the validity bits beside them -- from three ballots per turn.  From there the k-mers come
// out exactly as kmer_at takes them from a stream, and the lookups are depth_short_kernel's: all first probes of the batch
// issued before any is resolved.  No packed copy of the text goes through HBM; 8 bytes leave per record.
constexpr int HITS_TURNS = DEPTH_BATCH + 1;
constexpr int HITS_CHARS = 64 * HITS_TURNS, HITS_WORDS = HITS_CHARS / 32;
static_assert(64 * DEPTH_BATCH + PG_WIDE_MAX_K - 1 <= HITS_CHARS, "a batch's last k-mer ends inside the staged characters");

// the bits of x at the even positions of a 64-bit word
__device__ __forceinline__ uint64_t spread_bits(uint32_t x)
{
    uint64_t v = x;
    v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
    v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
    v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}

// (what one lane of a wavefront wrote to LDS, the others may read behind this, and the other way round)
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the record's malformation, or 0, from its five line starts (an index that is none -- outside the contract -- is a bad record
// too: nothing outside the text is read).  *len = the sequence line's bytes.  read_spans_kernel asks the same questions, and
// more, in one round trip of its own
__device__ __forceinline__ uint32_t fastq_record_check(const uint8_t *__restrict__ text, int64_t n_bytes, int64_t s0, int64_t s1, int64_t s2, int64_t s3,
                                                       int64_t s4, uint32_t min_qual, int64_t *len)
{
    *len = 0;
    if (!(s0 >= 0 && s0 < s1 && s1 < s2 && s2 < s3 && s3 <= s4 && s4 <= n_bytes)) return PG_FASTQ_BAD_INDEX;
    if (text[s0] != '@') return PG_FASTQ_NO_AT;
    if (text[s2] != '+') return PG_FASTQ_NO_PLUS;
    *len = s2 - 1 - s1;                                      // (the sequence line ends with the newline in front of the '+' line)
    if (min_qual) {
        const int64_t qlen = s4 - s3 - (s4 > s3 && text[s4 - 1] == '\n');
        if (qlen < *len) return PG_FASTQ_SHORT_QUALITY;
    }
    return 0;
}

// a malformed record to the two status words (one lane calls this)
__device__ __forceinline__ void fastq_record_bad(unsigned long long *status, int64_t ordinal, uint32_t bad)
{
    atomicMin(&status[1], ((unsigned long long)ordinal << 8) | bad);
    atomicOr(&status[0], (unsigned long long)PG_STATUS_FASTQ_FORMAT);
}

// the batch that begins at position `base` of a sequence line of `len` bytes, staged into the wavefront's stream words
__device__ __forceinline__ void hits_stage(const uint8_t *__restrict__ text, int64_t s1, int64_t s3, int64_t len, int64_t base, int lane, int lenient,
                                           uint32_t min_qual, uint64_t *wc, uint32_t *wv)
{
#pragma unroll
    for (int u = 0; u < HITS_TURNS; ++u) {
        if (base + 64 * u >= len) break;                     // (the same for the whole wavefront; no k-mer of the line reaches these words)
        const int64_t j = base + 64 * u + lane;
        uint32_t ch = 0;
        bool ok = false;
        if (j < len) {
            ch = text[s1 + j];
            const uint32_t up = lenient ? ch & 0xDFu : ch;
            ok = up == 'A' || up == 'C' || up == 'G' || up == 'T';
            if (ok && min_qual) ok = text[s3 + j] >= min_qual;               // (a base: j is below the quality line's length)
        }
        const uint64_t v = __ballot(ok), b0 = __ballot((ch >> 1) & 1u), b1 = __ballot((ch >> 2) & 1u);
        if (lane < 2) {
            wc[2 * u + lane] = spread_bits((uint32_t)(b0 >> (32 * lane))) | (spread_bits((uint32_t)(b1 >> (32 * lane))) << 1);
            wv[2 * u + lane] = (uint32_t)(v >> (32 * lane));
        }
    }
    wave_lds_sync();
}

// the staged batch looked up: have[u] = position base + 64 u + lane holds a k-mer, c[u] = its stored count (0 without one).  All
// first probes are issued before any is resolved
template <int TK>
__device__ __forceinline__ void hits_lookup(const uint64_t *wc, const uint32_t *wv, int64_t base, int64_t n_pos, int lane, int k, uint64_t kmask,
                                            const uint32_t *__restrict__ dense, const HashView &t, bool (&have)[DEPTH_BATCH], uint32_t (&c)[DEPTH_BATCH])
{
    Lookup<TK> p[DEPTH_BATCH];
#pragma unroll
    for (int u = 0; u < DEPTH_BATCH; ++u) {
        const int g = lane + 64 * u;
        uint64_t canon = 0;
        p[u].key = p[u].hh = p[u].cur = 0;
        have[u] = base + g < n_pos && kmer_at(wc, wv, g, k, kmask, &canon);
        if (have[u]) p[u].issue(canon, k, dense, t);
    }
#pragma unroll
    for (int u = 0; u < DEPTH_BATCH; ++u) c[u] = have[u] ? p[u].resolve(t) : 0u;
}

template <int TK>
__global__ __launch_bounds__(BLOCK) void read_hits_kernel(const uint8_t *__restrict__ text, int64_t n_bytes, const long long *__restrict__ line_start,
                                                          int64_t n_records, int64_t first_record, int k, uint64_t lower, uint64_t upper, int lenient,
                                                          uint32_t min_qual, const uint32_t *__restrict__ dense, HashView t, uint32_t *__restrict__ out,
                                                          unsigned long long *status)
{
    __shared__ uint64_t s_codes[WAVES][HITS_WORDS];
    __shared__ uint32_t s_valid[WAVES][HITS_WORDS];
    const int lane = threadIdx.x & 63;
    uint64_t *wc = s_codes[threadIdx.x >> 6];
    uint32_t *wv = s_valid[threadIdx.x >> 6];
    const uint64_t kmask = low_mask<uint64_t>(k);
    const int64_t n_waves = (int64_t)gridDim.x * WAVES;
    for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < n_records; r += n_waves) {
        const int64_t s0 = line_start[4 * r], s1 = line_start[4 * r + 1], s2 = line_start[4 * r + 2], s3 = line_start[4 * r + 3], s4 = line_start[4 * r + 4];
        int64_t len;
        const uint32_t bad = fastq_record_check(text, n_bytes, s0, s1, s2, s3, s4, min_qual, &len);
        if (bad) {                                           // (the same for the whole wavefront)
            if (lane == 0) {
                fastq_record_bad(status, first_record + r, bad);
                out[2 * r] = out[2 * r + 1] = 0;
            }
            continue;
        }
        const int64_t n_pos = len >= k ? len - k + 1 : 0;
        uint32_t n = 0, h = 0;
        for (int64_t base = 0; base < n_pos; base += 64 * DEPTH_BATCH) {
            hits_stage(text, s1, s3, len, base, lane, lenient, min_qual, wc, wv);
            bool have[DEPTH_BATCH];
            uint32_t c[DEPTH_BATCH];
            hits_lookup<TK>(wc, wv, base, n_pos, lane, k, kmask, dense, t, have, c);
#pragma unroll
            for (int u = 0; u < DEPTH_BATCH; ++u) {
                n += (uint32_t)__popcll(__ballot(have[u]));
                h += (uint32_t)__popcll(__ballot(have[u] && c[u] >= lower && c[u] <= upper));
            }
            wave_lds_sync();                                 // (the next batch stages over these words)
        }
        if (lane == 0) { out[2 * r] = n; out[2 * r + 1] = h; }
    }
}

// ---- 3. the kept records to their places: record kept[i]'s bytes [line_start[4 r], line_start[4 r + 4]) to out + dst_off[i].  One
// wavefront per kept record.  Source and destination are unaligned with respect to each other: the destination side goes in
// whole 16-byte pieces (each read from wherever it lies in the source), the fewer than 16 bytes in front of the first aligned
// piece and behind the last byte-wise, as table_dump_text_kernel places its units.  No byte outside [0, n_bytes) of the text is
// read and none outside [0, out_bytes) of `out` written, whatever the device arrays say.

// len bytes from src to dst by one wavefront (the caller has checked both ranges)
__device__ __forceinline__ void wave_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, int64_t len, int lane)
{
    int64_t head = (int64_t)((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
    if (head > len) head = len;
    const int64_t n16 = (len - head) >> 4, tail = len - head - (n16 << 4);
    for (int64_t q = lane; q < n16; q += 64) {
        uint4 v;
        __builtin_memcpy(&v, src + head + (q << 4), 16);                      // (no alignment is promised for the source)
        *(uint4 *)(dst + head + (q << 4)) = v;
    }
    if (lane < head + tail) {
        const int64_t o = lane < head ? lane : len - tail + (lane - head);
        dst[o] = src[o];
    }
}

__global__ __launch_bounds__(BLOCK) void fastq_gather_kernel(const uint8_t *__restrict__ text, int64_t n_bytes, const long long *__restrict__ line_start,
                                                             int64_t n_records, const long long *__restrict__ kept, const long long *__restrict__ dst_off,
                                                             int64_t n_kept, uint8_t *__restrict__ out, int64_t out_bytes)
{
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * WAVES;
    for (int64_t i = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); i < n_kept; i += n_waves) {
        const int64_t r = kept[i];
        if (r < 0 || r >= n_records) continue;
        const int64_t a = line_start[4 * r], b = line_start[4 * r + 4], d = dst_off[i];
        if (a < 0 || b < a || b > n_bytes || d < 0 || d > out_bytes - (b - a)) continue;
        wave_copy(out + d, text + a, b - a, lane);
    }
}

// ---- 4. the solid span of every record: read_hits_kernel's staging and lookups, and per turn of a batch the ballot of
// have && in-window -- 64 solid flags in position order, the same in every lane -- walked for its runs.  The walk keeps (start,
// length) of the run that is open at the word's first position and of the best run closed so far in wave-uniform registers, so
// a run may begin in one word and end any number of words or batches later; ctz of the word and of its complement jump from
// one run boundary to the next.  The flags never touch LDS and no lane loops over positions.  A closed run replaces the best
// only when it is LONGER (ties keep the earlier one) and, in PG_SPAN_FIRST mode, only when it began at position 0.  There is no
// early exit in FIRST mode: n and h are those of read_hits_kernel over the whole line.  Semantics: the header's section "Reads
// of a FASTQ text trimmed to their solid span".
struct SpanRuns {
    uint32_t cur_start, cur_len, best_start, best_len;       // (32 bits, as n and h: a line of 2^32 positions is outside the contract)

    __device__ __forceinline__ void close(int mode)
    {
        if (cur_len > best_len && (mode == PG_SPAN_LONGEST || cur_start == 0)) { best_start = cur_start; best_len = cur_len; }
        cur_len = 0;
    }
    // the flags of positions at .. at + 63, lowest bit first (positions without a flag: 0)
    __device__ __forceinline__ void take(uint64_t w, uint32_t at, int mode)
    {
        int pos = 0;
        while (pos < 64) {
            const uint64_t gaps = ~(w >> pos);               // (the shift fills with 0: there is a gap at or before bit 64 - pos)
            const int ones = pos ? __builtin_ctzll(gaps) : gaps ? __builtin_ctzll(gaps) : 64;
            if (ones) {
                if (!cur_len) cur_start = at + pos;
                cur_len += ones;
                pos += ones;
                if (pos == 64) break;                        // (the run is open at the word's end)
            }
            close(mode);
            const uint64_t rest = w >> pos;
            if (!rest) break;
            pos += __builtin_ctzll(rest);
        }
    }
};

template <int TK>
__global__ __launch_bounds__(BLOCK) void read_spans_kernel(const uint8_t *__restrict__ text, int64_t n_bytes, const long long *__restrict__ line_start,
                                                           int64_t n_records, int64_t first_record, int k, uint64_t lower, uint64_t upper, int lenient,
                                                           uint32_t min_qual, int mode, const uint32_t *__restrict__ dense, HashView t,
                                                           uint32_t *__restrict__ out, long long *__restrict__ trimmed_bytes, unsigned long long *status)
{
    __shared__ uint64_t s_codes[WAVES][HITS_WORDS];
    __shared__ uint32_t s_valid[WAVES][HITS_WORDS];
    const int lane = threadIdx.x & 63;
    // (the wavefront's number, in a form the compiler knows to be the same in every lane: the record's index words and everything
    // derived from them then go through scalar loads and registers, not through 64 lanes that all ask for the same address)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *wc = s_codes[wave];
    uint32_t *wv = s_valid[wave];
    const uint64_t kmask = low_mask<uint64_t>(k);
    const int64_t n_waves = (int64_t)gridDim.x * WAVES;
    for (int64_t r = (int64_t)blockIdx.x * WAVES + wave; r < n_records; r += n_waves) {
        const int64_t s0 = line_start[4 * r], s1 = line_start[4 * r + 1], s2 = line_start[4 * r + 2], s3 = line_start[4 * r + 3], s4 = line_start[4 * r + 4];
        // the record's check, as fastq_record_check makes it, and its line ends.  Every byte looked at -- '@', '+', the last of the
        // sequence line, the last two of the record -- has its address from the index alone, so all five loads leave together:
        // one round trip in front of the characters, not one per question
        uint32_t bad = 0;
        int64_t len = 0;
        int cr_s = 0, cr_q = 0, nl = 0;
        if (!(s0 >= 0 && s0 < s1 && s1 < s2 && s2 < s3 && s3 <= s4 && s4 <= n_bytes)) bad = PG_FASTQ_BAD_INDEX;
        else {
            len = s2 - 1 - s1;
            // (s0 <= s1 - 1 <= s2 - 2 and s1 <= s2 - 1 <= s4 - 2: all five lie inside the text, whether or not a line is empty)
            const uint32_t c0 = text[s0], c2 = text[s2], e_s = text[s2 - 2], e1 = text[s4 - 1], e2 = text[s4 - 2];
            nl = (s4 > s3) & (e1 == '\n');                    // (& and not &&: no load waits behind a branch on another)
            const int64_t qlen = s4 - s3 - nl;
            cr_s = (len > 0) & (e_s == '\r');
            cr_q = (qlen > 0) & ((nl ? e2 : e1) == '\r');
            if (c0 != '@') bad = PG_FASTQ_NO_AT;
            else if (c2 != '+') bad = PG_FASTQ_NO_PLUS;
            else if ((min_qual && qlen < len) || qlen - cr_q < len - cr_s) bad = PG_FASTQ_SHORT_QUALITY;      // (the quality line is cut too)
            if (bad) len = 0;
        }
        if (bad) {                                           // (the same for the whole wavefront)
            if (lane == 0) {
                fastq_record_bad(status, first_record + r, bad);
                trimmed_bytes[r] = 0;
            }
            if (lane < 4) out[4 * r + lane] = 0;
            continue;
        }
        const int64_t n_pos = len >= k ? len - k + 1 : 0;
        uint32_t n = 0, h = 0;
        SpanRuns runs = {0, 0, 0, 0};
        for (int64_t base = 0; base < n_pos; base += 64 * DEPTH_BATCH) {
            hits_stage(text, s1, s3, len, base, lane, lenient, min_qual, wc, wv);
            bool have[DEPTH_BATCH];
            uint32_t c[DEPTH_BATCH];
            hits_lookup<TK>(wc, wv, base, n_pos, lane, k, kmask, dense, t, have, c);
#pragma unroll
            for (int u = 0; u < DEPTH_BATCH; ++u) {
                const uint64_t solid = __ballot(have[u] && c[u] >= lower && c[u] <= upper);
                n += (uint32_t)__popcll(__ballot(have[u]));
                h += (uint32_t)__popcll(solid);
                if (solid | runs.cur_len) runs.take(solid, (uint32_t)(base + 64 * u), mode);
            }
            wave_lds_sync();                                 // (the next batch stages over these words)
        }
        runs.close(mode);
        const int64_t length = runs.best_len ? (int64_t)runs.best_len + k - 1 : 0;
        if (lane < 4) out[4 * r + lane] = lane == 0 ? n : lane == 1 ? h : lane == 2 ? runs.best_start : (uint32_t)length;
        if (lane == 0) trimmed_bytes[r] = (s1 - s0) + length + cr_s + 1 + (s3 - s2) + length + cr_q + nl;
    }
}

// ---- 5. the kept records to their places, each cut to its span (start, length) = spans[r][2], spans[r][3]: line 0 as it is,
// seq[start : start + length] and its line end, line 2 as it is, qual[start : start + length] and its line end ('\r' where the
// line had one, the last '\n' iff the record ended in one).  One wavefront per kept record, four wave_copy calls; the line ends
// are single bytes of their own.  cr_s, cr_q and the final newline are read from the text again, and everything handed in is
// checked: a record whose r, index, span or destination is not what read_spans_kernel would have given is skipped.  No byte
// outside [0, n_bytes) of the text is read and none outside [0, out_bytes) of `out` written.
__global__ __launch_bounds__(BLOCK) void fastq_gather_trimmed_kernel(const uint8_t *__restrict__ text, int64_t n_bytes,
                                                                     const long long *__restrict__ line_start, int64_t n_records,
                                                                     const long long *__restrict__ kept, const uint32_t *__restrict__ spans,
                                                                     const long long *__restrict__ dst_off, int64_t n_kept, uint8_t *__restrict__ out,
                                                                     int64_t out_bytes)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));    // (as in read_spans_kernel: scalar loads of what is per record)
    const int64_t n_waves = (int64_t)gridDim.x * WAVES;
    for (int64_t i = (int64_t)blockIdx.x * WAVES + wave; i < n_kept; i += n_waves) {
        const int64_t r = kept[i];
        if (r < 0 || r >= n_records) continue;
        const int64_t s0 = line_start[4 * r], s1 = line_start[4 * r + 1], s2 = line_start[4 * r + 2], s3 = line_start[4 * r + 3], s4 = line_start[4 * r + 4];
        if (!(s0 >= 0 && s0 < s1 && s1 < s2 && s2 < s3 && s3 <= s4 && s4 <= n_bytes)) continue;
        const int64_t start = spans[4 * r + 2], length = spans[4 * r + 3], d = dst_off[i];
        const int64_t len = s2 - 1 - s1;
        // (the three bytes that say how the lines end have their addresses from the index and lie inside the text whether or not a
        // line is empty -- s0 <= s2 - 2, s1 <= s4 - 2 --: they are loaded together)
        const uint32_t e_s = text[s2 - 2], e1 = text[s4 - 1], e2 = text[s4 - 2];
        const int nl = (s4 > s3) & (e1 == '\n');            // (& and not &&: no load waits behind a branch on another)
        const int64_t qlen = s4 - s3 - nl;
        const int cr_s = (len > 0) & (e_s == '\r'), cr_q = (qlen > 0) & ((nl ? e2 : e1) == '\r');
        if (start + length > len - cr_s || start + length > qlen - cr_q) continue;
        const int64_t size = (s1 - s0) + length + cr_s + 1 + (s3 - s2) + length + cr_q + nl;
        if (d < 0 || d > out_bytes - size) continue;
        uint8_t *const seq = out + d + (s1 - s0), *const plus = seq + length + cr_s + 1, *const qual = plus + (s3 - s2);
        wave_copy(out + d, text + s0, s1 - s0, lane);
        wave_copy(seq, text + s1 + start, length, lane);
        wave_copy(plus, text + s2, s3 - s2, lane);
        wave_copy(qual, text + s3 + start, length, lane);
        if (lane < cr_s + 1) seq[length + lane] = lane < cr_s ? '\r' : '\n';
        if (lane < cr_q + nl) qual[length + lane] = lane < cr_q ? '\r' : '\n';
    }
}

// ---- 6. single substitutions put right: read_spans_kernel's staging, lookups and record header, and per turn of a batch TWO
// ballots, have and solid.  have & ~solid are the WEAK positions (a k-mer outside the window), solid the S positions, ~have the
// V positions (no k-mer); -1 and n_pos are E.  The walker below keeps the open run of weak positions and the class of the
// position in front of it in wave-uniform registers across ballot words and batches, and jumps from run boundary to run
// boundary with ctz, as SpanRuns does.  A run that closes is judged at once by the same wavefront -- no list of candidates,
// so no cap per record -- against the header's table of shapes, and a candidate is verified (correct_candidate).  Semantics: the
// header's section "Single substitutions in the reads of a FASTQ text put right".
enum { CLS_V = 0, CLS_S = 1, CLS_E = 2 };

struct WeakRuns {
    uint32_t start, len, left;                               // the open run [start, start + len) and the class of position start - 1
    uint32_t carry;                                          // the last position of the word before was solid

    // the next run that closes inside the word of positions at .. at + cnt - 1 (weak has no bit at or above cnt), from bit *pos
    // on: true with (a, n, lf, rt) = its start, its length and the classes of its two neighbours, *pos where to go on
    __device__ __forceinline__ bool next(uint64_t weak, uint64_t solid, uint32_t at, int cnt, int *pos, uint32_t *a, uint32_t *n, uint32_t *lf,
                                         uint32_t *rt)
    {
        int at_bit = *pos;
        while (at_bit < cnt) {
            const uint64_t gaps = ~(weak >> at_bit);         // (the shift fills with 0: there is a gap at or before bit 64 - at_bit)
            const int ones = at_bit ? __builtin_ctzll(gaps) : gaps ? __builtin_ctzll(gaps) : 64;
            if (ones) {
                if (!len) {
                    start = at + at_bit;
                    left = start == 0 ? (uint32_t)CLS_E : at_bit ? (uint32_t)((solid >> (at_bit - 1)) & 1u) : carry;
                }
                len += ones;
                at_bit += ones;
                if (at_bit >= cnt) break;                    // (the run is open at the word's end, or at the line's)
            }
            const bool closed = len != 0;
            if (closed) {
                *a = start;
                *n = len;
                *lf = left;
                *rt = (uint32_t)((solid >> at_bit) & 1u);
                len = 0;
            }
            const uint64_t rest = weak >> at_bit;
            at_bit = rest ? at_bit + __builtin_ctzll(rest) : cnt;
            if (closed) {
                *pos = at_bit;
                return true;
            }
        }
        *pos = at_bit;
        return false;
    }
};

// what a closed run needs beside its own numbers (the same for the whole kernel, or for the record)
struct CorrectArgs {
    const uint8_t *text;
    uint8_t *out;
    int64_t s1, len;
    int k;
    uint64_t kmask, lower, upper;
    const uint32_t *dense;
    HashView t;
};

// the closed run [a, a + n) between neighbours of classes lf and rt: 0 = no candidate, 1 = a candidate that stays, 2 = corrected.
// The shapes: S .. S with n == k, E .. S and S .. E with n <= k; the base in question is p = a + n - 1 where the right neighbour
// is solid, a + k - 1 at the line's end.  Every k-mer of the run holds base p and no other k-mer does, so the 2k - 1 characters
// seq[a .. a + 2k - 2], clipped to the line, are all the verification needs: one per lane, straight from the text (a may lie in
// the batch before the staged one), their 2-bit codes as two ballots.  All of them are bases, since every position of the run
// holds a k-mer.  Lane j < n shifts the ballots by j, which is the window of the k-mer at a + j in the stream's form, puts each of
// the three other codes at base p, and issues all three lookups before it resolves any; three ballots say which alternatives
// every k-mer of the run accepts.  Exactly one: lane 0 stores that base, in the letter case of the byte it replaces -- the only
// store of the kernel beside its row.  The ballots stay in registers: a window of at most 61 characters needs no LDS.
// Inlined into every turn of the unrolled batch: as one function that the kernel calls it measured 2 % slower.
template <int TK>
__device__ __forceinline__ uint32_t correct_candidate(const CorrectArgs &g, uint32_t a, uint32_t n, uint32_t lf, uint32_t rt, int lane)
{
    const int k = g.k;
    if (lf == CLS_V || rt == CLS_V || (lf == CLS_E && rt == CLS_E)) return 0;
    if (lf == CLS_S && rt == CLS_S ? n != (uint32_t)k : n > (uint32_t)k) return 0;
    const uint32_t p = rt == CLS_S ? a + n - 1 : a + (uint32_t)k - 1;
    const int64_t j = (int64_t)a + lane;
    uint32_t ch = 0;
    if (lane < 2 * k - 1 && j < g.len) ch = g.text[g.s1 + j];
    const uint64_t b0 = __ballot((ch >> 1) & 1u), b1 = __ballot((ch >> 2) & 1u);
    const uint32_t was = (uint32_t)__shfl((int)ch, (int)(p - a));        // (p - a < 2k - 1 <= 61, and p < len: that lane has read)
    const uint32_t code = (was >> 1) & 3u;
    const bool mine = (uint32_t)lane < n;
    const int at = 2 * ((int)(p - a) - lane);                // (where base p lies in the window of the k-mer at a + lane: 0 <= at < 2k for mine)
    const uint64_t w = (spread_bits((uint32_t)(b0 >> lane)) | (spread_bits((uint32_t)(b1 >> lane)) << 1)) & g.kmask;
    Lookup<TK> q[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        q[x].key = q[x].hh = q[x].cur = 0;
        if (mine) {
            const uint64_t c = (w & ~(3ull << at)) | ((uint64_t)((code + 1 + x) & 3u) << at);
            // (as kmer_at: the forward code is the window reversed, the reverse complement the window complemented)
            const uint64_t fw = rev2_64(c) >> (64 - 2 * k), rc = (c ^ 0xAAAAAAAAAAAAAAAAull) & g.kmask;
            q[x].issue(fw < rc ? fw : rc, k, g.dense, g.t);
        }
    }
    uint32_t valid = 0;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const uint32_t c = mine ? q[x].resolve(g.t) : 0u;
        if (__ballot(mine && !(c >= g.lower && c <= g.upper)) == 0) valid |= 1u << x;
    }
    if (__popc(valid) != 1) return 1;
    const uint32_t put = (code + (uint32_t)__ffs(valid)) & 3u;          // (the codes: A 0, C 1, T 2, G 3)
    if (g.out && lane == 0) g.out[g.s1 + p] = (uint8_t)(((0x47544341u >> (8 * put)) & 0xFFu) | (was & 0x20u));
    return 2;
}

// text and out carry no __restrict__: out may be the text itself.  That is sound because a record belongs to one wavefront, and
// inside a record every store follows every load of its byte: base p of a run lies in front of the first character of any later
// run of the record (the later run begins behind this one's solid right neighbour, b > p), so no later verification reads it,
// and in front of the first character of the batch staged after the run has closed (that batch begins behind b).  The record's
// header bytes are read before its first store.
template <int TK>
__global__ __launch_bounds__(BLOCK) void read_correct_kernel(const uint8_t *text, int64_t n_bytes, const long long *__restrict__ line_start,
                                                             int64_t n_records, int64_t first_record, int k, uint64_t lower, uint64_t upper, int lenient,
                                                             uint32_t min_qual, const uint32_t *__restrict__ dense, HashView t, uint8_t *out,
                                                             uint32_t *__restrict__ rows, unsigned long long *status)
{
    __shared__ uint64_t s_codes[WAVES][HITS_WORDS];
    __shared__ uint32_t s_valid[WAVES][HITS_WORDS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));    // (as in read_spans_kernel: what is per record stays scalar)
    uint64_t *wc = s_codes[wave];
    uint32_t *wv = s_valid[wave];
    CorrectArgs g;
    g.text = text;
    g.out = out;
    g.k = k;
    g.kmask = low_mask<uint64_t>(k);
    g.lower = lower;
    g.upper = upper;
    g.dense = dense;
    g.t = t;
    const int64_t n_waves = (int64_t)gridDim.x * WAVES;
    for (int64_t r = (int64_t)blockIdx.x * WAVES + wave; r < n_records; r += n_waves) {
        const int64_t s0 = line_start[4 * r], s1 = line_start[4 * r + 1], s2 = line_start[4 * r + 2], s3 = line_start[4 * r + 3], s4 = line_start[4 * r + 4];
        // (the record's check and its line ends exactly as read_spans_kernel makes them: five loads that leave together)
        uint32_t bad = 0;
        int64_t len = 0;
        if (!(s0 >= 0 && s0 < s1 && s1 < s2 && s2 < s3 && s3 <= s4 && s4 <= n_bytes)) bad = PG_FASTQ_BAD_INDEX;
        else {
            len = s2 - 1 - s1;
            const uint32_t c0 = text[s0], c2 = text[s2], e_s = text[s2 - 2], e1 = text[s4 - 1], e2 = text[s4 - 2];
            const int nl = (s4 > s3) & (e1 == '\n');
            const int64_t qlen = s4 - s3 - nl;
            const int cr_s = (len > 0) & (e_s == '\r'), cr_q = (qlen > 0) & ((nl ? e2 : e1) == '\r');
            if (c0 != '@') bad = PG_FASTQ_NO_AT;
            else if (c2 != '+') bad = PG_FASTQ_NO_PLUS;
            else if ((min_qual && qlen < len) || qlen - cr_q < len - cr_s) bad = PG_FASTQ_SHORT_QUALITY;
            len -= cr_s;                                     // (the bases of the line: a final '\r' is beyond its end, not a position without a k-mer)
        }
        if (bad) {                                           // (the same for the whole wavefront)
            if (lane == 0) fastq_record_bad(status, first_record + r, bad);
            if (lane < 4) rows[4 * r + lane] = 0;
            continue;
        }
        g.s1 = s1;
        g.len = len;
        const int64_t n_pos = len >= k ? len - k + 1 : 0;
        uint32_t n = 0, h = 0, candidates = 0, corrected = 0;
        WeakRuns runs = {0, 0, CLS_E, 0};
        for (int64_t base = 0; base < n_pos; base += 64 * DEPTH_BATCH) {
            hits_stage(text, s1, s3, len, base, lane, lenient, min_qual, wc, wv);
            bool have[DEPTH_BATCH];
            uint32_t c[DEPTH_BATCH];
            hits_lookup<TK>(wc, wv, base, n_pos, lane, k, g.kmask, dense, t, have, c);
#pragma unroll
            for (int u = 0; u < DEPTH_BATCH; ++u) {
                const uint64_t held = __ballot(have[u]), solid = __ballot(have[u] && c[u] >= lower && c[u] <= upper);
                const uint64_t weak = held & ~solid;
                const int64_t rest = n_pos - (base + 64 * u);
                const int cnt = rest >= 64 ? 64 : rest > 0 ? (int)rest : 0;
                n += (uint32_t)__popcll(held);
                h += (uint32_t)__popcll(solid);
                if (cnt && (weak | runs.len)) {
                    int pos = 0;
                    uint32_t a, m, lf, rt;
                    while (runs.next(weak, solid, (uint32_t)(base + 64 * u), cnt, &pos, &a, &m, &lf, &rt)) {
                        const uint32_t did = correct_candidate<TK>(g, a, m, lf, rt, lane);
                        candidates += did != 0;
                        corrected += did == 2;
                    }
                }
                if (cnt) runs.carry = (uint32_t)(solid >> 63);
            }
            wave_lds_sync();                                 // (the next batch stages over these words)
        }
        if (runs.len) {                                      // (open at the line's end: its right neighbour is E)
            const uint32_t did = correct_candidate<TK>(g, runs.start, runs.len, runs.left, CLS_E, lane);
            candidates += did != 0;
            corrected += did == 2;
        }
        if (lane < 4) rows[4 * r + lane] = lane == 0 ? n : lane == 1 ? h : lane == 2 ? candidates : corrected;
    }
}

// ---- 7. the depth of every record: an order statistic of its k-mers' counts, and the draw of its unit.  read_hits_kernel's
// staging and lookups again; what is new is that the answer is not additive over the batches of a record.  Every k-mer has the
// value c = its stored count, 0 when absent or below `lower`; d is the value at index ((n - 1) * percentile) / 100 of the n
// values in ascending order.  Two forms in one kernel, chosen per record and the same for the whole wavefront:
//   SHORT  n_pos <= 64 * DEPTH_BATCH (every linked short read): one batch, its values stay in the lanes' DEPTH_BATCH registers
//          and d comes from depth_short_kernel's search over the bits of the value -- one ballot per register and bit, from the
//          maximum's top bit down.
//   LONG   a radix select that keeps nothing per position: a first sweep over the batches gives n, present and the maximum,
//          then one sweep per 8-bit digit from the maximum's top non-zero byte down stages and looks the batches up again and
//          bins the digit of every value whose higher digits equal the prefix found so far into the wavefront's 256 bins in
//          LDS; the bin the rank falls in is the next digit.  At most 1 + 4 sweeps, no workspace, no length limit.
// The draw is splitmix64 of seed + (unit + 1) * the golden-ratio increment, its top 24 bits; semantics: the header's section
// "Depth of the reads of a FASTQ text".
constexpr int DRAW_BITS = 24;
__device__ __forceinline__ uint32_t unit_draw(uint64_t seed, uint64_t unit)
{
    uint64_t z = seed + (unit + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(z >> (64 - DRAW_BITS));
}

// hits_lookup with the values as the depth takes them: a count below `lower` is 0 (and so is a position without a k-mer)
template <int TK>
__device__ __forceinline__ void depth_values(const uint64_t *wc, const uint32_t *wv, int64_t base, int64_t n_pos, int lane, int k, uint64_t kmask,
                                             uint64_t lower, const uint32_t *__restrict__ dense, const HashView &t, bool (&have)[DEPTH_BATCH],
                                             uint32_t (&val)[DEPTH_BATCH])
{
    hits_lookup<TK>(wc, wv, base, n_pos, lane, k, kmask, dense, t, have, val);
#pragma unroll
    for (int u = 0; u < DEPTH_BATCH; ++u)
        if (val[u] < lower) val[u] = 0;
}

constexpr int SELECT_DIGIT_BITS = 8, SELECT_BINS = 1 << SELECT_DIGIT_BITS, SELECT_PER_LANE = SELECT_BINS / 64;

template <int TK>
__global__ __launch_bounds__(BLOCK) void read_depths_kernel(const uint8_t *__restrict__ text, int64_t n_bytes, const long long *__restrict__ line_start,
                                                            int64_t n_records, int64_t first_record, int k, uint64_t lower, uint32_t percentile,
                                                            int lenient, uint32_t min_qual, uint64_t seed, int unit_log2,
                                                            const uint32_t *__restrict__ dense, HashView t, uint4 *__restrict__ out,
                                                            unsigned long long *status)
{
    __shared__ uint64_t s_codes[WAVES][HITS_WORDS];
    __shared__ uint32_t s_valid[WAVES][HITS_WORDS];
    __shared__ uint32_t s_bins[WAVES][SELECT_BINS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));    // (as in read_spans_kernel: scalar loads of what is per record)
    uint64_t *wc = s_codes[wave];
    uint32_t *wv = s_valid[wave];
    uint32_t *bins = s_bins[wave];
    const uint64_t kmask = low_mask<uint64_t>(k);
    const int64_t n_waves = (int64_t)gridDim.x * WAVES;
    for (int64_t r = (int64_t)blockIdx.x * WAVES + wave; r < n_records; r += n_waves) {
        const int64_t s0 = line_start[4 * r], s1 = line_start[4 * r + 1], s2 = line_start[4 * r + 2], s3 = line_start[4 * r + 3], s4 = line_start[4 * r + 4];
        int64_t len;
        const uint32_t bad = fastq_record_check(text, n_bytes, s0, s1, s2, s3, s4, min_qual, &len);
        if (bad) {                                           // (the same for the whole wavefront)
            if (lane == 0) {
                fastq_record_bad(status, first_record + r, bad);
                out[r] = make_uint4(0, 0, 0, 0);
            }
            continue;
        }
        const int64_t n_pos = len >= k ? len - k + 1 : 0;
        uint32_t n = 0, present = 0, vmax = 0, d = 0, rank = 0;
        // sweep 0 gives n, present and the maximum, and is the only one of a SHORT record; sweep i > 0 of a LONG one bins the
        // digit at `shift`.  One loop for both, so that the staging and the lookups exist once in the kernel's code
        int shift = -1;
        while (true) {
            const uint64_t prefix = (uint64_t)d >> (shift + SELECT_DIGIT_BITS);
            if (shift >= 0) {
#pragma unroll
                for (int j = 0; j < SELECT_PER_LANE; ++j) bins[lane + 64 * j] = 0;
            }
            bool have[DEPTH_BATCH];
            uint32_t val[DEPTH_BATCH];
#pragma unroll
            for (int u = 0; u < DEPTH_BATCH; ++u) { have[u] = false; val[u] = 0; }
            for (int64_t base = 0; base < n_pos; base += 64 * DEPTH_BATCH) {
                hits_stage(text, s1, s3, len, base, lane, lenient, min_qual, wc, wv);     // (its sync orders the cleared bins too)
                depth_values<TK>(wc, wv, base, n_pos, lane, k, kmask, lower, dense, t, have, val);
                if (shift < 0) {
#pragma unroll
                    for (int u = 0; u < DEPTH_BATCH; ++u) {
                        n += (uint32_t)__popcll(__ballot(have[u]));
                        present += (uint32_t)__popcll(__ballot(val[u] > 0));
                        vmax = val[u] > vmax ? val[u] : vmax;
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < DEPTH_BATCH; ++u)
                        if (have[u] && ((uint64_t)val[u] >> (shift + SELECT_DIGIT_BITS)) == prefix)
                            atomicAdd(&bins[(val[u] >> shift) & (SELECT_BINS - 1)], 1u);
                }
                wave_lds_sync();                             // (the next batch, sweep or record stages over these words; the bins are complete)
            }
            if (shift < 0) {
#pragma unroll
                for (int s = 32; s >= 1; s >>= 1) {
                    const uint32_t m = __shfl_xor(vmax, s);
                    vmax = m > vmax ? m : vmax;
                }
                if (!vmax) break;                            // (no k-mer, or none with a value: d = 0)
                // the value at sorted index `rank`.  (n - 1 < 2^32 and percentile <= 100: 64 bits hold the product)
                rank = (uint32_t)(((uint64_t)(n - 1) * percentile) / 100);
                const int top = 31 - __clz((int)vmax);
                if (n_pos <= 64 * DEPTH_BATCH) {
                    // SHORT: the values of the one batch are still in the registers.  The largest x with at most `rank` values below it
                    for (int bit = top; bit >= 0; --bit) {
                        const uint32_t cand = d | (1u << bit);
                        uint32_t below = 0;
#pragma unroll
                        for (int u = 0; u < DEPTH_BATCH; ++u) below += (uint32_t)__popcll(__ballot(have[u] && val[u] < cand));
                        if (below <= rank) d = cand;
                    }
                    break;
                }
                shift = top & ~(SELECT_DIGIT_BITS - 1);
                continue;
            }
            // lane l holds bins 4 l .. 4 l + 3: the lane, then the bin, in which the running sum passes the rank.  (rank is below the
            // number of values that share the prefix, at every digit: the search ends inside the bins)
            uint32_t b[SELECT_PER_LANE], mine = 0;
#pragma unroll
            for (int j = 0; j < SELECT_PER_LANE; ++j) { b[j] = bins[SELECT_PER_LANE * lane + j]; mine += b[j]; }
            uint32_t upto = mine;                            // (inclusive sum over the lanes up to this one)
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const uint32_t o = __shfl_up(upto, s);
                if (lane >= s) upto += o;
            }
            const uint64_t past = __ballot(upto > rank);
            const int owner = past ? __builtin_ctzll(past) : 63;
            uint32_t before = upto - mine, digit = SELECT_PER_LANE * lane + SELECT_PER_LANE - 1;
            bool found = false;
#pragma unroll
            for (int j = 0; j < SELECT_PER_LANE; ++j) {
                if (!found && before + b[j] > rank) { digit = SELECT_PER_LANE * lane + j; found = true; }
                if (!found) before += b[j];
            }
            digit = __shfl(digit, owner);
            rank -= __shfl(before, owner);
            d |= digit << shift;
            wave_lds_sync();                                 // (the next digit clears the bins)
            if (shift == 0) break;
            shift -= SELECT_DIGIT_BITS;
        }
        if (lane == 0) out[r] = make_uint4(n, present, d, unit_draw(seed, (uint64_t)(first_record + r) >> unit_log2));
    }
}

}  // namespace

// the table as the streaming kernels see it (spectrum, dump, merge, combine): layout, entries, the counts plane of the planes form
struct DumpView {
    int form;
    int64_t n_entries;
    const uint4 *counts;
};
static int dump_view(const pg_table *t, const char *who, DumpView *v)
{
    int rc = check_table(t);
    if (rc) return rc;
    if ((uintptr_t)t->data & 15) return pg_fail(PG_EINVAL, "%s: t->data is not 16-byte aligned", who);
    v->counts = nullptr;
    if (t->kind == PG_TABLE_DENSE) {
        v->form = DUMP_DENSE;
        v->n_entries = (int64_t)1 << (2 * t->k);
    } else {
        v->form = t->kind == PG_TABLE_HASH ? DUMP_HASH : t->kind == PG_TABLE_MINI ? DUMP_MINI : DUMP_PLANES;
        v->n_entries = (int64_t)1 << t->log2_slots;
        if (v->form == DUMP_PLANES) v->counts = (const uint4 *)((const uint64_t *)t->data + v->n_entries);
    }
    return PG_OK;
}

extern "C" int pg_table_query(const pg_table *t, const uint64_t *codes, int64_t n, uint32_t *counts, void *stream)
{
    if (!t) return pg_fail(PG_EINVAL, "pg_table_query: t is null");
    if (!codes) return pg_fail(PG_EINVAL, "pg_table_query: codes is null");
    if (!counts) return pg_fail(PG_EINVAL, "pg_table_query: counts is null");
    if (n < 0) return pg_fail(PG_EINVAL, "pg_table_query: n is negative (%lld)", (long long)n);
    int rc = check_table(t);
    if (rc) return rc;
    if (n == 0) return PG_OK;
    const int grid = grid_for((n + QRY_BATCH - 1) / QRY_BATCH);
    const ProbeArgs pa = probe_args(t);
    rc = with_kind(t->kind, [&](auto tk) {
        return launch(table_query_kernel<decltype(tk)::value>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, "pg_table_query", codes, n, t->k, pa.dense,
                      pa.view, counts);
    });
    return rc ? rc : check_launch("pg_table_query");
}

extern "C" int pg_table_spectrum(const pg_table *t, int high, uint64_t *hist, void *stream)
{
    if (!t) return pg_fail(PG_EINVAL, "pg_table_spectrum: t is null");
    if (!hist) return pg_fail(PG_EINVAL, "pg_table_spectrum: hist is null");
    if (high < 1 || high > PG_SPECTRUM_MAX_HIGH) return pg_fail(PG_EINVAL, "pg_table_spectrum: high %d outside [1, %d]", high, PG_SPECTRUM_MAX_HIGH);
    DumpView v;
    int rc = dump_view(t, "pg_table_spectrum", &v);
    if (rc) return rc;
    // units of 16 bytes of the slots (planes form: 32 bytes of keys + 16 of counts); every form's table is a whole number of them
    const bool packed = v.form == DUMP_HASH || v.form == DUMP_MINI;
    const int64_t n_units = v.n_entries / (packed ? 2 : 4);
    // two workgroups of 1024 per CU: tables of up to 2^40 slots leave a workgroup at most 2^31 of them, so its 32-bit bins hold
    constexpr int64_t tile = (int64_t)BIG_BLOCK * SPEC_UNROLL;
    int64_t grid = (n_units + tile - 1) / tile;
    if (grid > 512) grid = 512;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)(high + 2) * sizeof(uint32_t);
    if (hipMemsetAsync(hist, 0, (size_t)(high + 2) * sizeof(uint64_t), s) != hipSuccess) return pg_fail(PG_EHIP, "pg_table_spectrum: cannot clear hist");
    // PG_SPECTRUM_BALLOT (timing experiments): 0 = every count through an LDS add, 1 = c == 1 by ballot (the default), 2 = c == 2 as well
    const char *env = getenv("PG_SPECTRUM_BALLOT");
    const int ballot = env && *env ? atoi(env) : 1;
    auto go = [&](auto form, auto bal) {
        return launch(table_spectrum_kernel<decltype(form)::value, decltype(bal)::value>, dim3((unsigned)grid), dim3(BIG_BLOCK), lds, s, "pg_table_spectrum",
                      (const uint4 *)t->data, v.counts, n_units, high, (unsigned long long *)hist);
    };
    auto by_ballot = [&](auto form) { return ballot <= 0 ? go(form, int_tag<0>{}) : ballot == 1 ? go(form, int_tag<1>{}) : go(form, int_tag<2>{}); };
    rc = v.form == DUMP_DENSE ? by_ballot(int_tag<DUMP_DENSE>{}) : packed ? by_ballot(int_tag<DUMP_HASH>{}) : by_ballot(int_tag<DUMP_PLANES>{});
    return rc ? rc : check_launch("pg_table_spectrum");
}

// ---- depth of sequences in a finished table (kernels: "depth of sequences" above)
extern "C" int pg_table_profile(const pg_table *t, const uint64_t *codes, const uint32_t *valid, int64_t n_chars, int64_t char_begin,
                                int64_t char_end, uint32_t *counts, void *stream)
{
    if (!t) return pg_fail(PG_EINVAL, "pg_table_profile: t is null");
    if (!codes || !valid) return pg_fail(PG_EINVAL, "pg_table_profile: the stream is null");
    if (!counts) return pg_fail(PG_EINVAL, "pg_table_profile: counts is null");
    if (n_chars < 0) return pg_fail(PG_EINVAL, "pg_table_profile: n_chars is negative (%lld)", (long long)n_chars);
    if (char_begin < 0 || char_end < char_begin || char_end > n_chars)
        return pg_fail(PG_EINVAL, "pg_table_profile: range [%lld, %lld) outside the stream's %lld characters", (long long)char_begin,
                       (long long)char_end, (long long)n_chars);
    int rc = check_table(t);
    if (rc) return rc;
    const int64_t n = char_end - char_begin;
    if (n == 0) return PG_OK;
    const int grid = grid_for((n + DEPTH_BATCH - 1) / DEPTH_BATCH);
    const ProbeArgs pa = probe_args(t);
    rc = with_kind(t->kind, [&](auto tk) {
        return launch(table_profile_kernel<decltype(tk)::value>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, "pg_table_profile", codes, valid, n_chars,
                      char_begin, n, t->k, pa.dense, pa.view, counts);
    });
    return rc ? rc : check_launch("pg_table_profile");
}

extern "C" int64_t pg_table_depth_workspace_bytes(int64_t n_long, int64_t long_positions)
{
    if (n_long < 0 || long_positions < 0) return pg_fail(PG_EINVAL, "pg_table_depth_workspace_bytes: negative size");
    if (n_long > PG_DEPTH_MAX_LONG) return pg_fail(PG_EINVAL, "pg_table_depth_workspace_bytes: more than %d long ranges in one call", PG_DEPTH_MAX_LONG);
    if (long_positions > (int64_t)(DEPTH_OFF_MASK >> 3)) return pg_fail(PG_EINVAL, "pg_table_depth_workspace_bytes: too many positions");
    const int64_t body = 4 * long_positions + (int64_t)sizeof(DepthLong) * n_long;
    return DEPTH_HEAD_BYTES + (body + 255) / 256 * 256;
}

extern "C" int pg_table_depth(const pg_table *t, const uint64_t *codes, const uint32_t *valid, int64_t n_chars, const int64_t *range_start,
                              const int64_t *range_end, int64_t n_ranges, int64_t lower, int64_t *out, void *workspace,
                              int64_t workspace_bytes, uint32_t *status, void *stream)
{
    if (!t) return pg_fail(PG_EINVAL, "pg_table_depth: t is null");
    if (!codes || !valid) return pg_fail(PG_EINVAL, "pg_table_depth: the stream is null");
    if (n_chars < 0) return pg_fail(PG_EINVAL, "pg_table_depth: n_chars is negative (%lld)", (long long)n_chars);
    if (n_chars > (int64_t)(DEPTH_OFF_MASK >> 3)) return pg_fail(PG_EINVAL, "pg_table_depth: a stream of %lld characters is too long", (long long)n_chars);
    if (n_ranges < 0) return pg_fail(PG_EINVAL, "pg_table_depth: n_ranges is negative (%lld)", (long long)n_ranges);
    if (n_ranges > 0 && (!range_start || !range_end)) return pg_fail(PG_EINVAL, "pg_table_depth: the range arrays are null");
    if (n_ranges > 0 && !out) return pg_fail(PG_EINVAL, "pg_table_depth: out is null");
    if (lower < 1) return pg_fail(PG_EINVAL, "pg_table_depth: lower must be at least 1 (got %lld)", (long long)lower);
    if (!workspace) return pg_fail(PG_EINVAL, "pg_table_depth: workspace is null");
    if ((uintptr_t)workspace & 255) return pg_fail(PG_EINVAL, "pg_table_depth: workspace is not 256-byte aligned");
    if (workspace_bytes < DEPTH_HEAD_BYTES)
        return pg_fail(PG_EINVAL, "pg_table_depth: workspace of %lld bytes is smaller than the %lld every call needs", (long long)workspace_bytes,
                       (long long)DEPTH_HEAD_BYTES);
    if (!status) return pg_fail(PG_EINVAL, "pg_table_depth: status is null");
    int rc = check_table(t);
    if (rc) return rc;
    if (n_ranges == 0) return PG_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t ws_bytes = workspace_bytes & ~(int64_t)255;      // (the list of long ranges hangs from the end: keep it aligned)
    if (hipMemsetAsync(workspace, 0, (size_t)DEPTH_HEAD_BYTES, s) != hipSuccess) return pg_fail(PG_EHIP, "pg_table_depth: cannot clear the workspace's head");
    const ProbeArgs pa = probe_args(t);
    const int grid = grid_for(n_ranges, WAVES);
    // room for one long range at least?  (a caller whose ranges are all short gives the head alone: two launches less)
    const int64_t room = (ws_bytes - DEPTH_HEAD_BYTES) / 4;
    const bool any_long = ws_bytes - DEPTH_HEAD_BYTES >= (int64_t)sizeof(DepthLong) + 4 * (PG_DEPTH_SHORT_MAX + 2 - PG_WIDE_MAX_K);
    const int fill_grid = grid_for((room + DEPTH_BATCH - 1) / DEPTH_BATCH);
    int64_t select_grid = (ws_bytes - DEPTH_HEAD_BYTES) / ((int64_t)sizeof(DepthLong) + 4 * (PG_DEPTH_SHORT_MAX + 2 - PG_WIDE_MAX_K));
    if (select_grid > 2048) select_grid = 2048;
    rc = with_kind(t->kind, [&](auto tk) {
        constexpr int TK = decltype(tk)::value;
        int r = launch(depth_short_kernel<TK>, dim3(grid), dim3(BLOCK), 0, s, "pg_table_depth", codes, valid, n_chars, range_start, range_end, n_ranges,
                       t->k, (uint64_t)lower, pa.dense, pa.view, (long long *)out, workspace, ws_bytes, status);
        if (!r && any_long)
            r = launch(depth_fill_kernel<TK>, dim3(fill_grid), dim3(BLOCK), 0, s, "pg_table_depth", codes, valid, n_chars, workspace, ws_bytes, t->k,
                       pa.dense, pa.view, status);
        return r;
    });
    if (rc) return rc;
    if (any_long)
        hipLaunchKernelGGL(depth_select_kernel, dim3((unsigned)select_grid), dim3(BIG_BLOCK), 0, s, (const void *)workspace, ws_bytes,
                           (uint64_t)lower, (long long *)out, (const uint32_t *)status);
    return check_launch("pg_table_depth");
}

extern "C" int64_t pg_table_dump_units(const pg_table *t)
{
    if (!t) return pg_fail(PG_EINVAL, "pg_table_dump_units: t is null");
    DumpView v;
    int rc = dump_view(t, "pg_table_dump_units", &v);
    if (rc) return rc;
    return (v.n_entries + PG_DUMP_UNIT_SLOTS - 1) / PG_DUMP_UNIT_SLOTS;
}

// kernel by the storage layout of a table (DumpView::form): f(int_tag<DUMP_DENSE | DUMP_HASH | DUMP_MINI | DUMP_PLANES>)
template <class F> int with_form(int form, F &&f)
{
    return form == DUMP_DENSE ? f(int_tag<DUMP_DENSE>{}) : form == DUMP_HASH ? f(int_tag<DUMP_HASH>{}) : form == DUMP_MINI ? f(int_tag<DUMP_MINI>{})
                                                                                                        : f(int_tag<DUMP_PLANES>{});
}

extern "C" int pg_table_dump_sizes(const pg_table *t, int64_t lower, int64_t *unit_bytes, int64_t *unit_lines, void *stream)
{
    if (!t) return pg_fail(PG_EINVAL, "pg_table_dump_sizes: t is null");
    if (!unit_bytes) return pg_fail(PG_EINVAL, "pg_table_dump_sizes: unit_bytes is null");
    if (lower < 1) return pg_fail(PG_EINVAL, "pg_table_dump_sizes: lower is below 1 (%lld)", (long long)lower);
    DumpView v;
    int rc = dump_view(t, "pg_table_dump_sizes", &v);
    if (rc) return rc;
    const int64_t n_units = (v.n_entries + PG_DUMP_UNIT_SLOTS - 1) / PG_DUMP_UNIT_SLOTS;
    const int grid = grid_for(n_units, 1);
    rc = with_form(v.form, [&](auto form) {
        return launch(table_dump_sizes_kernel<decltype(form)::value>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, "pg_table_dump_sizes",
                      (const uint4 *)t->data, v.counts, v.n_entries, n_units, t->k, (uint64_t)lower, (long long *)unit_bytes, (long long *)unit_lines);
    });
    return rc ? rc : check_launch("pg_table_dump_sizes");
}

extern "C" int pg_table_dump_text(const pg_table *t, int64_t lower, int64_t unit_begin, int64_t unit_end, const int64_t *unit_offsets,
                                  int64_t text_base, int64_t range_bytes, uint8_t *text, int64_t text_bytes, void *stream)
{
    if (!t) return pg_fail(PG_EINVAL, "pg_table_dump_text: t is null");
    if (!unit_offsets) return pg_fail(PG_EINVAL, "pg_table_dump_text: unit_offsets is null");
    if (!text) return pg_fail(PG_EINVAL, "pg_table_dump_text: text is null");
    if (lower < 1) return pg_fail(PG_EINVAL, "pg_table_dump_text: lower is below 1 (%lld)", (long long)lower);
    if (text_base < 0) return pg_fail(PG_EINVAL, "pg_table_dump_text: text_base is negative (%lld)", (long long)text_base);
    if (range_bytes < 0) return pg_fail(PG_EINVAL, "pg_table_dump_text: range_bytes is negative (%lld)", (long long)range_bytes);
    if (text_bytes < 0) return pg_fail(PG_EINVAL, "pg_table_dump_text: text_bytes is negative (%lld)", (long long)text_bytes);
    DumpView v;
    int rc = dump_view(t, "pg_table_dump_text", &v);
    if (rc) return rc;
    const int64_t n_units = (v.n_entries + PG_DUMP_UNIT_SLOTS - 1) / PG_DUMP_UNIT_SLOTS;
    if (unit_begin < 0 || unit_begin > unit_end)
        return pg_fail(PG_EINVAL, "pg_table_dump_text: units [%lld, %lld) are no range", (long long)unit_begin, (long long)unit_end);
    if (unit_end > n_units)
        return pg_fail(PG_EINVAL, "pg_table_dump_text: units [%lld, %lld) reach past the table's %lld", (long long)unit_begin, (long long)unit_end, (long long)n_units);
    if (text_bytes < range_bytes)
        return pg_fail(PG_EINVAL, "pg_table_dump_text: text of %lld bytes is shorter than the range's %lld", (long long)text_bytes, (long long)range_bytes);
    if (unit_end == unit_begin || range_bytes == 0) return PG_OK;
    const int grid = grid_for(unit_end - unit_begin, 1);
    rc = with_form(v.form, [&](auto form) {
        return launch(table_dump_text_kernel<decltype(form)::value>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, "pg_table_dump_text",
                      (const uint4 *)t->data, v.counts, v.n_entries, unit_begin, unit_end, t->k, (uint64_t)lower, (const long long *)unit_offsets, text_base,
                      range_bytes, text);
    });
    return rc ? rc : check_launch("pg_table_dump_text");
}

// ---- merging finished tables: what `jellyfish merge` gives over the tables of feature.py:76-94

// bytes of a table's storage
static int64_t table_bytes(const pg_table *t)
{
    if (t->kind == PG_TABLE_DENSE) return (int64_t)4 << (2 * t->k);
    return (int64_t)(t->kind == PG_TABLE_HASH || t->kind == PG_TABLE_MINI ? 8 : 12) << t->log2_slots;
}

static bool tables_overlap(const pg_table *a, const pg_table *b)
{
    const uintptr_t a0 = (uintptr_t)a->data, b0 = (uintptr_t)b->data;
    return a0 < b0 + (uint64_t)table_bytes(b) && b0 < a0 + (uint64_t)table_bytes(a);
}

// a geometry the aligned form takes: MINI, or HASH in LDS-sized buckets (at most 2^30 of them: one launch)
static bool aligned_kind(const pg_table *t)
{
    if (!t) return false;
    if (t->kind == PG_TABLE_MINI)
        return t->k >= PG_MINI_MIN_K && t->k <= PG_HASH_MAX_K && t->log2_bucket_slots >= 4 && t->log2_bucket_slots <= PG_BUCKET_MAX_LOG2_SLOTS &&
               t->log2_slots >= t->log2_bucket_slots && t->log2_slots - t->log2_bucket_slots <= PG_MINI_MAX_LOG2_BUCKETS;
    if (t->kind == PG_TABLE_HASH)
        return t->k >= 1 && t->k <= PG_HASH_MAX_K && t->log2_slots >= 10 && t->log2_slots <= 40 && t->log2_bucket_slots >= 4 &&
               t->log2_bucket_slots <= PG_BUCKET_MAX_LOG2_SLOTS && t->log2_bucket_slots <= t->log2_slots && t->log2_slots - t->log2_bucket_slots <= 30;
    return false;
}

extern "C" int pg_table_merge_aligned_applies(const pg_table *a, const pg_table *b)
{
    return aligned_kind(a) && aligned_kind(b) && a->kind == b->kind && a->k == b->k && a->log2_slots == b->log2_slots &&
                   a->log2_bucket_slots == b->log2_bucket_slots
               ? 1 : 0;
}

extern "C" int pg_table_merge_aligned(const pg_table *dst, const pg_table *const *srcs, int n_srcs, uint32_t *status, void *stream)
{
    if (!dst) return pg_fail(PG_EINVAL, "pg_table_merge_aligned: dst is null");
    if (!srcs) return pg_fail(PG_EINVAL, "pg_table_merge_aligned: srcs is null");
    if (!status) return pg_fail(PG_EINVAL, "pg_table_merge_aligned: status is null");
    if (n_srcs < 1 || n_srcs > ALIGNED_MAX_SRCS) return pg_fail(PG_EINVAL, "pg_table_merge_aligned: n_srcs %d outside [1, %d]", n_srcs, ALIGNED_MAX_SRCS);
    int rc = check_table(dst);
    if (rc) return rc;
    if ((uintptr_t)dst->data & 15) return pg_fail(PG_EINVAL, "pg_table_merge_aligned: dst->data is not 16-byte aligned");
    MergeSources ms;
    for (int i = 0; i < ALIGNED_MAX_SRCS; ++i) ms.p[i] = nullptr;
    for (int i = 0; i < n_srcs; ++i) {
        if (!srcs[i]) return pg_fail(PG_EINVAL, "pg_table_merge_aligned: srcs[%d] is null", i);
        if ((rc = check_table(srcs[i]))) return rc;
        if (srcs[i]->k != dst->k) return pg_fail(PG_EINVAL, "pg_table_merge_aligned: k differs (dst %d, srcs[%d] %d)", dst->k, i, srcs[i]->k);
        if (!pg_table_merge_aligned_applies(dst, srcs[i]))
            return pg_fail(PG_EINVAL, "pg_table_merge_aligned: dst and srcs[%d] are not mini tables, or bucketed hash tables, of one geometry "
                                      "(kind %d / %d, 2^%d / 2^%d slots, buckets of 2^%d / 2^%d)", i, dst->kind, srcs[i]->kind, dst->log2_slots,
                           srcs[i]->log2_slots, dst->log2_bucket_slots, srcs[i]->log2_bucket_slots);
        if ((uintptr_t)srcs[i]->data & 15) return pg_fail(PG_EINVAL, "pg_table_merge_aligned: srcs[%d]->data is not 16-byte aligned", i);
        if (tables_overlap(dst, srcs[i])) return pg_fail(PG_EINVAL, "pg_table_merge_aligned: dst aliases srcs[%d]", i);
        ms.p[i] = (const ulonglong2 *)srcs[i]->data;
    }
    if (!aligned_kind(dst)) return pg_fail(PG_EINVAL, "pg_table_merge_aligned: needs mini tables or bucketed hash tables with LDS-sized buckets");
    const int bits = dst->log2_slots - dst->log2_bucket_slots;
    const size_t lds = (size_t)8 << dst->log2_bucket_slots;
    const bool mini = dst->kind == PG_TABLE_MINI;
    rc = with_flag(mini, [&](auto m) {
        return launch(table_merge_aligned_kernel<decltype(m)::value>, dim3(1u << bits), dim3(BIG_BLOCK), lds, (hipStream_t)stream, "pg_table_merge_aligned",
                      ms, n_srcs, view_of(dst), status);
    });
    return rc ? rc : check_launch("pg_table_merge_aligned");
}

extern "C" int pg_table_merge(const pg_table *dst, const pg_table *src, uint32_t *status, void *stream)
{
    if (!dst) return pg_fail(PG_EINVAL, "pg_table_merge: dst is null");
    if (!src) return pg_fail(PG_EINVAL, "pg_table_merge: src is null");
    int rc = check_table(dst);
    if (rc) return rc;
    DumpView v;
    if ((rc = dump_view(src, "pg_table_merge", &v))) return rc;
    if (dst->k != src->k) return pg_fail(PG_EINVAL, "pg_table_merge: k differs (dst %d, src %d)", dst->k, src->k);
    if (!status && dst->kind != PG_TABLE_DENSE) return pg_fail(PG_EINVAL, "pg_table_merge: status is null");
    if (tables_overlap(dst, src)) return pg_fail(PG_EINVAL, "pg_table_merge: dst aliases src");
    const int64_t n_quads = v.n_entries / DUMP_PER;                       // (4^k and 2^log2_slots are whole numbers of quads)
    const int grid = grid_for((n_quads + MERGE_QUADS - 1) / MERGE_QUADS);
    const ProbeArgs pa = probe_args(dst);
    rc = with_form(v.form, [&](auto form) {
        return with_kind(dst->kind, [&](auto tk) {
            return launch(table_merge_kernel<decltype(form)::value, decltype(tk)::value>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, "pg_table_merge",
                          (const uint4 *)src->data, v.counts, n_quads, dst->k, pa.dense, pa.view, status);
        });
    });
    return rc ? rc : check_launch("pg_table_merge");
}

// ---- combining finished tables (min, max, diff, left, only, keep): beside the tables of feature.py:76-94, replacing nothing

// what the three entries refuse alike; `b` may be null where the op says so
static int combine_args(const char *who, const pg_table *a, const pg_table *b, int op, int64_t lower, int64_t upper)
{
    if (!a) return pg_fail(PG_EINVAL, "%s: a is null", who);
    if (op < PG_COMBINE_MIN || op > PG_COMBINE_KEEP) return pg_fail(PG_EINVAL, "%s: unknown op %d", who, op);
    if (op == PG_COMBINE_KEEP && b) return pg_fail(PG_EINVAL, "%s: PG_COMBINE_KEEP takes no b", who);
    if (op != PG_COMBINE_KEEP && !b) return pg_fail(PG_EINVAL, "%s: b is null (only PG_COMBINE_KEEP takes none)", who);
    if (lower < 1) return pg_fail(PG_EINVAL, "%s: lower is below 1 (%lld)", who, (long long)lower);
    if (upper >= 0 && upper < lower) return pg_fail(PG_EINVAL, "%s: upper %lld is below lower %lld", who, (long long)upper, (long long)lower);
    int rc = check_table(a);
    if (rc) return rc;
    if (b && (rc = check_table(b))) return rc;
    if (b && a->k != b->k) return pg_fail(PG_EINVAL, "%s: k differs (a %d, b %d)", who, a->k, b->k);
    if ((uintptr_t)a->data & 15) return pg_fail(PG_EINVAL, "%s: a->data is not 16-byte aligned", who);
    if (b && ((uintptr_t)b->data & 15)) return pg_fail(PG_EINVAL, "%s: b->data is not 16-byte aligned", who);
    return PG_OK;
}

extern "C" int pg_table_combine_aligned(const pg_table *dst, const pg_table *a, const pg_table *b, int op, int64_t lower, int64_t upper,
                                        uint32_t *status, void *stream)
{
    const char *who = "pg_table_combine_aligned";
    if (!dst) return pg_fail(PG_EINVAL, "%s: dst is null", who);
    if (!status) return pg_fail(PG_EINVAL, "%s: status is null", who);
    int rc = combine_args(who, a, b, op, lower, upper);
    if (rc) return rc;
    if ((rc = check_table(dst))) return rc;
    if (dst->k != a->k) return pg_fail(PG_EINVAL, "%s: k differs (dst %d, a %d)", who, dst->k, a->k);
    if ((uintptr_t)dst->data & 15) return pg_fail(PG_EINVAL, "%s: dst->data is not 16-byte aligned", who);
    if (!pg_table_merge_aligned_applies(dst, a) || (b && !pg_table_merge_aligned_applies(dst, b)))
        return pg_fail(PG_EINVAL, "%s: dst, a and b are not mini tables, or bucketed hash tables, of one geometry (kind %d / %d / %d, 2^%d / 2^%d / 2^%d "
                                  "slots, buckets of 2^%d / 2^%d / 2^%d)", who, dst->kind, a->kind, b ? b->kind : a->kind, dst->log2_slots, a->log2_slots,
                       b ? b->log2_slots : a->log2_slots, dst->log2_bucket_slots, a->log2_bucket_slots, b ? b->log2_bucket_slots : a->log2_bucket_slots);
    if (tables_overlap(dst, a)) return pg_fail(PG_EINVAL, "%s: dst aliases a", who);
    if (b && tables_overlap(dst, b)) return pg_fail(PG_EINVAL, "%s: dst aliases b", who);
    const int bits = dst->log2_slots - dst->log2_bucket_slots;
    // the bucket's slots and one bit for each, the bitmap rounded up to 16 bytes
    const size_t lds = ((size_t)8 << dst->log2_bucket_slots) + ((((size_t)1 << dst->log2_bucket_slots) / 8 + 15) & ~(size_t)15);
    const bool mini = dst->kind == PG_TABLE_MINI;
    const uint64_t up = upper < 0 ? ~0ull : (uint64_t)upper;
    const ulonglong2 *pa = (const ulonglong2 *)a->data, *pb = b ? (const ulonglong2 *)b->data : nullptr;
    rc = with_flag(mini, [&](auto m) {
        return launch(table_combine_aligned_kernel<decltype(m)::value>, dim3(1u << bits), dim3(BIG_BLOCK), lds, (hipStream_t)stream, who, pa, pb, op,
                      (uint64_t)lower, up, view_of(dst), status);
    });
    return rc ? rc : check_launch(who);
}

extern "C" int pg_table_combine_items(const pg_table *a, const pg_table *b, int op, int64_t lower, int64_t upper, uint64_t *codes, uint32_t *counts,
                                      int64_t cap, int64_t *n_out, uint32_t *status, void *stream)
{
    const char *who = "pg_table_combine_items";
    if (!status) return pg_fail(PG_EINVAL, "%s: status is null", who);
    int rc = combine_args(who, a, b, op, lower, upper);
    if (rc) return rc;
    if (cap < 0) return pg_fail(PG_EINVAL, "%s: cap is negative (%lld)", who, (long long)cap);
    if (!n_out) return pg_fail(PG_EINVAL, "%s: n_out is null", who);
    if (cap > 0 && (!codes || !counts)) return pg_fail(PG_EINVAL, "%s: codes or counts is null", who);
    DumpView v;
    if ((rc = dump_view(a, who, &v))) return rc;
    const int64_t n_quads = v.n_entries / DUMP_PER;                       // (4^k and 2^log2_slots are whole numbers of quads)
    const int grid = grid_for((n_quads + MERGE_QUADS - 1) / MERGE_QUADS);
    const ProbeArgs pb = probe_args(b);
    const uint64_t up = upper < 0 ? ~0ull : (uint64_t)upper;
    // kernel by (layout of a, kind of b; TK_NONE: no b)
    rc = with_form(v.form, [&](auto form) {
        return with_kind_or_none(b, [&](auto tk) {
            return launch(table_combine_items_kernel<decltype(form)::value, decltype(tk)::value>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, who,
                          (const uint4 *)a->data, v.counts, n_quads, a->k, pb.dense, pb.view, op, (uint64_t)lower, up, codes, counts,
                          (unsigned long long)cap, (unsigned long long *)n_out, status);
        });
    });
    return rc ? rc : check_launch(who);
}

extern "C" int pg_table_compare(const pg_table *a, const pg_table *b, uint64_t *out, void *stream)
{
    const char *who = "pg_table_compare";
    if (!a) return pg_fail(PG_EINVAL, "%s: a is null", who);
    if (!out) return pg_fail(PG_EINVAL, "%s: out is null", who);
    int rc = combine_args(who, a, b, b ? PG_COMBINE_MIN : PG_COMBINE_KEEP, 1, -1);
    if (rc) return rc;
    DumpView v;
    if ((rc = dump_view(a, who, &v))) return rc;
    const int64_t n_quads = v.n_entries / DUMP_PER;
    const int grid = grid_for((n_quads + MERGE_QUADS - 1) / MERGE_QUADS);
    const ProbeArgs pb = probe_args(b);
    if (hipMemsetAsync(out, 0, 4 * sizeof(uint64_t), (hipStream_t)stream) != hipSuccess) return pg_fail(PG_EHIP, "%s: cannot clear out", who);
    rc = with_form(v.form, [&](auto form) {
        return with_kind_or_none(b, [&](auto tk) {
            return launch(table_compare_kernel<decltype(form)::value, decltype(tk)::value>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, who,
                          (const uint4 *)a->data, v.counts, n_quads, a->k, pb.dense, pb.view, (unsigned long long *)out);
        });
    });
    return rc ? rc : check_launch(who);
}

extern "C" int64_t pg_dump_parse_workspace_bytes(int64_t n_bytes)
{
    if (n_bytes < 0) return pg_fail(PG_EINVAL, "pg_dump_parse_workspace_bytes: n_bytes is negative (%lld)", (long long)n_bytes);
    const int64_t n_tiles = (n_bytes + PARSE_TILE - 1) / PARSE_TILE;
    return (2 * n_tiles + 2) * (int64_t)sizeof(uint64_t);                  // newlines per tile; their exclusive scan, n_tiles + 1
}

extern "C" int pg_dump_parse(const uint8_t *text, int64_t n_bytes, int k, int64_t first_ordinal, uint64_t *codes, uint64_t *counts,
                             int64_t *ordinals, int64_t cap, int64_t *n_out, uint64_t *status, void *workspace, int64_t workspace_bytes,
                             void *stream)
{
    if (!text) return pg_fail(PG_EINVAL, "pg_dump_parse: text is null");
    if (n_bytes < 0) return pg_fail(PG_EINVAL, "pg_dump_parse: n_bytes is negative (%lld)", (long long)n_bytes);
    if (k < 1 || k > PG_WIDE_MAX_K) return pg_fail(PG_EINVAL, "pg_dump_parse: k %d outside [1, %d]", k, PG_WIDE_MAX_K);
    if (first_ordinal < 0) return pg_fail(PG_EINVAL, "pg_dump_parse: first_ordinal is negative (%lld)", (long long)first_ordinal);
    if (!codes) return pg_fail(PG_EINVAL, "pg_dump_parse: codes is null");
    if (!counts) return pg_fail(PG_EINVAL, "pg_dump_parse: counts is null");
    if (!ordinals) return pg_fail(PG_EINVAL, "pg_dump_parse: ordinals is null");
    if (cap < 0) return pg_fail(PG_EINVAL, "pg_dump_parse: cap is negative (%lld)", (long long)cap);
    if (!n_out) return pg_fail(PG_EINVAL, "pg_dump_parse: n_out is null");
    if (!status) return pg_fail(PG_EINVAL, "pg_dump_parse: status is null");
    if ((uintptr_t)text & 15) return pg_fail(PG_EINVAL, "pg_dump_parse: text is not 16-byte aligned");
    if (n_bytes == 0) return PG_OK;
    const int64_t need = pg_dump_parse_workspace_bytes(n_bytes);
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < need)
        return pg_fail(PG_EINVAL, "pg_dump_parse: workspace of %lld bytes, %lld needed (8-byte aligned)", (long long)workspace_bytes, (long long)need);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_tiles = (n_bytes + PARSE_TILE - 1) / PARSE_TILE;
    unsigned long long *hist = (unsigned long long *)workspace, *first = hist + n_tiles + 1;
    if (hipMemsetAsync(n_out, 0, 2 * sizeof(int64_t), s) != hipSuccess || hipMemsetAsync(status, 0xff, sizeof(uint64_t), s) != hipSuccess)
        return pg_fail(PG_EHIP, "pg_dump_parse: cannot clear the counters");
    const int grid = grid_for(n_tiles, 1);
    hipLaunchKernelGGL(dump_newlines_kernel, dim3(grid), dim3(BLOCK), 0, s, text, n_bytes, n_tiles, hist);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(BIG_BLOCK), 0, s, (const unsigned long long *)hist, n_tiles, first);
    hipLaunchKernelGGL(dump_parse_kernel, dim3(grid), dim3(BLOCK), 0, s, text, n_bytes, n_tiles, (const unsigned long long *)first, k, first_ordinal,
                       codes, counts, (long long *)ordinals, cap, (unsigned long long *)n_out, (unsigned long long *)status);
    return check_launch("pg_dump_parse");
}

// ---- reads of a FASTQ text by their k-mers' counts (kernels: the section of the same name above); beside the read set of
// scripts/low_abd_reads.sh:10 / extract_unmapped.cpp, replacing nothing
extern "C" int64_t pg_fastq_index_workspace_bytes(int64_t n_bytes)
{
    if (n_bytes < 0) return pg_fail(PG_EINVAL, "pg_fastq_index_workspace_bytes: n_bytes is negative (%lld)", (long long)n_bytes);
    return pg_dump_parse_workspace_bytes(n_bytes);                         // (the same tiles: newlines per tile and their scan)
}

extern "C" int pg_fastq_index(const uint8_t *text, int64_t n_bytes, int64_t *line_start, int64_t cap, int64_t *n_lines, void *workspace,
                              int64_t workspace_bytes, void *stream)
{
    if (!text) return pg_fail(PG_EINVAL, "pg_fastq_index: text is null");
    if (n_bytes < 0) return pg_fail(PG_EINVAL, "pg_fastq_index: n_bytes is negative (%lld)", (long long)n_bytes);
    if (!line_start) return pg_fail(PG_EINVAL, "pg_fastq_index: line_start is null");
    if (cap < 1) return pg_fail(PG_EINVAL, "pg_fastq_index: cap is below 1 (%lld)", (long long)cap);
    if (!n_lines) return pg_fail(PG_EINVAL, "pg_fastq_index: n_lines is null");
    if ((uintptr_t)text & 15) return pg_fail(PG_EINVAL, "pg_fastq_index: text is not 16-byte aligned");
    if (n_bytes == 0) return PG_OK;
    const int64_t need = pg_fastq_index_workspace_bytes(n_bytes);
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < need)
        return pg_fail(PG_EINVAL, "pg_fastq_index: workspace of %lld bytes, %lld needed (8-byte aligned)", (long long)workspace_bytes, (long long)need);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_tiles = (n_bytes + PARSE_TILE - 1) / PARSE_TILE;
    unsigned long long *hist = (unsigned long long *)workspace, *first = hist + n_tiles + 1;
    const int grid = grid_for(n_tiles, 1);
    hipLaunchKernelGGL(dump_newlines_kernel, dim3(grid), dim3(BLOCK), 0, s, text, n_bytes, n_tiles, hist);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(BIG_BLOCK), 0, s, (const unsigned long long *)hist, n_tiles, first);
    hipLaunchKernelGGL(fastq_lines_kernel, dim3(grid), dim3(BLOCK), 0, s, text, n_bytes, n_tiles, (const unsigned long long *)first,
                       (long long *)line_start, cap, (long long *)n_lines);
    return check_launch("pg_fastq_index");
}

extern "C" int pg_table_read_hits(const pg_table *t, int k, const uint8_t *text, int64_t n_bytes, const int64_t *line_start, int64_t n_records,
                                  int64_t first_record, int64_t lower, int64_t upper, int lowercase_is_base, int min_qual_char, uint32_t *hits,
                                  uint64_t *status, void *stream)
{
    const char *who = "pg_table_read_hits";
    if (!t) return pg_fail(PG_EINVAL, "%s: t is null", who);
    if (!text) return pg_fail(PG_EINVAL, "%s: text is null", who);
    if (!line_start) return pg_fail(PG_EINVAL, "%s: line_start is null", who);
    if (!hits) return pg_fail(PG_EINVAL, "%s: hits is null", who);
    if (!status) return pg_fail(PG_EINVAL, "%s: status is null", who);
    if (n_bytes < 0) return pg_fail(PG_EINVAL, "%s: n_bytes is negative (%lld)", who, (long long)n_bytes);
    if (n_records < 0) return pg_fail(PG_EINVAL, "%s: n_records is negative (%lld)", who, (long long)n_records);
    if (first_record < 0) return pg_fail(PG_EINVAL, "%s: first_record is negative (%lld)", who, (long long)first_record);
    if (lower < 0) return pg_fail(PG_EINVAL, "%s: lower is negative (%lld)", who, (long long)lower);
    if (upper >= 0 && upper < lower) return pg_fail(PG_EINVAL, "%s: upper %lld is below lower %lld", who, (long long)upper, (long long)lower);
    if (min_qual_char < 0 || min_qual_char > 255) return pg_fail(PG_EINVAL, "%s: min_qual_char %d is no byte (0: none)", who, min_qual_char);
    if ((uintptr_t)text & 15) return pg_fail(PG_EINVAL, "%s: text is not 16-byte aligned", who);
    int rc = check_table(t);
    if (rc) return rc;
    if (t->k != k) return pg_fail(PG_EINVAL, "%s: k differs (table %d, asked %d)", who, t->k, k);
    if (n_records == 0) return PG_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(uint64_t), s) != hipSuccess || hipMemsetAsync(status + 1, 0xff, sizeof(uint64_t), s) != hipSuccess)
        return pg_fail(PG_EHIP, "%s: cannot clear the status", who);
    const ProbeArgs pa = probe_args(t);
    const int grid = grid_for(n_records, WAVES);
    const uint64_t up = upper < 0 ? ~0ull : (uint64_t)upper;
    rc = with_kind(t->kind, [&](auto tk) {
        return launch(read_hits_kernel<decltype(tk)::value>, dim3(grid), dim3(BLOCK), 0, s, who, text, n_bytes, (const long long *)line_start, n_records,
                      first_record, k, (uint64_t)lower, up, lowercase_is_base ? 1 : 0, (uint32_t)min_qual_char, pa.dense, pa.view, hits,
                      (unsigned long long *)status);
    });
    return rc ? rc : check_launch(who);
}

extern "C" int pg_fastq_gather(const uint8_t *text, int64_t n_bytes, const int64_t *line_start, int64_t n_records, const int64_t *kept,
                               const int64_t *dst_off, int64_t n_kept, uint8_t *out, int64_t out_bytes, void *stream)
{
    const char *who = "pg_fastq_gather";
    if (!text) return pg_fail(PG_EINVAL, "%s: text is null", who);
    if (!line_start) return pg_fail(PG_EINVAL, "%s: line_start is null", who);
    if (n_bytes < 0) return pg_fail(PG_EINVAL, "%s: n_bytes is negative (%lld)", who, (long long)n_bytes);
    if (n_records < 0) return pg_fail(PG_EINVAL, "%s: n_records is negative (%lld)", who, (long long)n_records);
    if (n_kept < 0 || n_kept > n_records) return pg_fail(PG_EINVAL, "%s: n_kept %lld outside [0, %lld]", who, (long long)n_kept, (long long)n_records);
    if (out_bytes < 0) return pg_fail(PG_EINVAL, "%s: out_bytes is negative (%lld)", who, (long long)out_bytes);
    if (n_kept > 0 && (!kept || !dst_off)) return pg_fail(PG_EINVAL, "%s: kept or dst_off is null", who);
    if (n_kept > 0 && !out) return pg_fail(PG_EINVAL, "%s: out is null", who);
    if (n_kept == 0) return PG_OK;
    hipLaunchKernelGGL(fastq_gather_kernel, dim3(grid_for(n_kept, WAVES)), dim3(BLOCK), 0, (hipStream_t)stream, text, n_bytes, (const long long *)line_start,
                       n_records, (const long long *)kept, (const long long *)dst_off, n_kept, out, out_bytes);
    return check_launch(who);
}

// ---- reads of a FASTQ text trimmed to their solid span (kernels: 4. and 5. of the section above); beside the read set of
// scripts/low_abd_reads.sh:10 / extract_unmapped.cpp, replacing nothing
extern "C" int pg_table_read_spans(const pg_table *t, int k, const uint8_t *text, int64_t n_bytes, const int64_t *line_start, int64_t n_records,
                                   int64_t first_record, int64_t lower, int64_t upper, int lowercase_is_base, int min_qual_char, int mode,
                                   uint32_t *spans, int64_t *trimmed_bytes, uint64_t *status, void *stream)
{
    const char *who = "pg_table_read_spans";
    if (!t) return pg_fail(PG_EINVAL, "%s: t is null", who);
    if (!text) return pg_fail(PG_EINVAL, "%s: text is null", who);
    if (!line_start) return pg_fail(PG_EINVAL, "%s: line_start is null", who);
    if (!spans) return pg_fail(PG_EINVAL, "%s: spans is null", who);
    if (!trimmed_bytes) return pg_fail(PG_EINVAL, "%s: trimmed_bytes is null", who);
    if (!status) return pg_fail(PG_EINVAL, "%s: status is null", who);
    if (n_bytes < 0) return pg_fail(PG_EINVAL, "%s: n_bytes is negative (%lld)", who, (long long)n_bytes);
    if (n_records < 0) return pg_fail(PG_EINVAL, "%s: n_records is negative (%lld)", who, (long long)n_records);
    if (first_record < 0) return pg_fail(PG_EINVAL, "%s: first_record is negative (%lld)", who, (long long)first_record);
    if (lower < 0) return pg_fail(PG_EINVAL, "%s: lower is negative (%lld)", who, (long long)lower);
    if (upper >= 0 && upper < lower) return pg_fail(PG_EINVAL, "%s: upper %lld is below lower %lld", who, (long long)upper, (long long)lower);
    if (min_qual_char < 0 || min_qual_char > 255) return pg_fail(PG_EINVAL, "%s: min_qual_char %d is no byte (0: none)", who, min_qual_char);
    if (mode != PG_SPAN_FIRST && mode != PG_SPAN_LONGEST)
        return pg_fail(PG_EINVAL, "%s: mode %d is neither PG_SPAN_FIRST nor PG_SPAN_LONGEST", who, mode);
    if ((uintptr_t)text & 15) return pg_fail(PG_EINVAL, "%s: text is not 16-byte aligned", who);
    int rc = check_table(t);
    if (rc) return rc;
    if (t->k != k) return pg_fail(PG_EINVAL, "%s: k differs (table %d, asked %d)", who, t->k, k);
    if (n_records == 0) return PG_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(uint64_t), s) != hipSuccess || hipMemsetAsync(status + 1, 0xff, sizeof(uint64_t), s) != hipSuccess)
        return pg_fail(PG_EHIP, "%s: cannot clear the status", who);
    const ProbeArgs pa = probe_args(t);
    const int grid = grid_for(n_records, WAVES);
    const uint64_t up = upper < 0 ? ~0ull : (uint64_t)upper;
    rc = with_kind(t->kind, [&](auto tk) {
        return launch(read_spans_kernel<decltype(tk)::value>, dim3(grid), dim3(BLOCK), 0, s, who, text, n_bytes, (const long long *)line_start, n_records,
                      first_record, k, (uint64_t)lower, up, lowercase_is_base ? 1 : 0, (uint32_t)min_qual_char, mode, pa.dense, pa.view, spans,
                      (long long *)trimmed_bytes, (unsigned long long *)status);
    });
    return rc ? rc : check_launch(who);
}

extern "C" int pg_fastq_gather_trimmed(const uint8_t *text, int64_t n_bytes, const int64_t *line_start, int64_t n_records, const int64_t *kept,
                                       const uint32_t *spans, const int64_t *dst_off, int64_t n_kept, uint8_t *out, int64_t out_bytes, void *stream)
{
    const char *who = "pg_fastq_gather_trimmed";
    if (!text) return pg_fail(PG_EINVAL, "%s: text is null", who);
    if (!line_start) return pg_fail(PG_EINVAL, "%s: line_start is null", who);
    if (n_bytes < 0) return pg_fail(PG_EINVAL, "%s: n_bytes is negative (%lld)", who, (long long)n_bytes);
    if (n_records < 0) return pg_fail(PG_EINVAL, "%s: n_records is negative (%lld)", who, (long long)n_records);
    if (n_kept < 0 || n_kept > n_records) return pg_fail(PG_EINVAL, "%s: n_kept %lld outside [0, %lld]", who, (long long)n_kept, (long long)n_records);
    if (out_bytes < 0) return pg_fail(PG_EINVAL, "%s: out_bytes is negative (%lld)", who, (long long)out_bytes);
    if (n_kept > 0 && !kept) return pg_fail(PG_EINVAL, "%s: kept is null", who);
    if (n_kept > 0 && !spans) return pg_fail(PG_EINVAL, "%s: spans is null", who);
    if (n_kept > 0 && !dst_off) return pg_fail(PG_EINVAL, "%s: dst_off is null", who);
    if (n_kept > 0 && !out) return pg_fail(PG_EINVAL, "%s: out is null", who);
    if (n_kept == 0) return PG_OK;
    hipLaunchKernelGGL(fastq_gather_trimmed_kernel, dim3(grid_for(n_kept, WAVES)), dim3(BLOCK), 0, (hipStream_t)stream, text, n_bytes,
                       (const long long *)line_start, n_records, (const long long *)kept, spans, (const long long *)dst_off, n_kept, out, out_bytes);
    return check_launch(who);
}

// ---- single substitutions in the reads of a FASTQ text put right (kernel: 6. of the section above); beside the read set of
// scripts/low_abd_reads.sh:10 / extract_unmapped.cpp, replacing nothing
extern "C" int pg_table_correct_reads(const pg_table *t, int k, const uint8_t *text, int64_t n_bytes, const int64_t *line_start, int64_t n_records,
                                      int64_t first_record, int64_t lower, int64_t upper, int lowercase_is_base, int min_qual_char, uint8_t *out,
                                      uint32_t *rows, uint64_t *status, void *stream)
{
    const char *who = "pg_table_correct_reads";
    if (!t) return pg_fail(PG_EINVAL, "%s: t is null", who);
    if (!text) return pg_fail(PG_EINVAL, "%s: text is null", who);
    if (!line_start) return pg_fail(PG_EINVAL, "%s: line_start is null", who);
    if (!rows) return pg_fail(PG_EINVAL, "%s: rows is null", who);
    if (!status) return pg_fail(PG_EINVAL, "%s: status is null", who);
    if (n_bytes < 0) return pg_fail(PG_EINVAL, "%s: n_bytes is negative (%lld)", who, (long long)n_bytes);
    if (n_records < 0) return pg_fail(PG_EINVAL, "%s: n_records is negative (%lld)", who, (long long)n_records);
    if (first_record < 0) return pg_fail(PG_EINVAL, "%s: first_record is negative (%lld)", who, (long long)first_record);
    if (lower < 0) return pg_fail(PG_EINVAL, "%s: lower is negative (%lld)", who, (long long)lower);
    if (upper >= 0 && upper < lower) return pg_fail(PG_EINVAL, "%s: upper %lld is below lower %lld", who, (long long)upper, (long long)lower);
    if (min_qual_char < 0 || min_qual_char > 255) return pg_fail(PG_EINVAL, "%s: min_qual_char %d is no byte (0: none)", who, min_qual_char);
    if ((uintptr_t)text & 15) return pg_fail(PG_EINVAL, "%s: text is not 16-byte aligned", who);
    int rc = check_table(t);
    if (rc) return rc;
    if (t->k != k) return pg_fail(PG_EINVAL, "%s: k differs (table %d, asked %d)", who, t->k, k);
    if (n_records == 0) return PG_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(uint64_t), s) != hipSuccess || hipMemsetAsync(status + 1, 0xff, sizeof(uint64_t), s) != hipSuccess)
        return pg_fail(PG_EHIP, "%s: cannot clear the status", who);
    const ProbeArgs pa = probe_args(t);
    const int grid = grid_for(n_records, WAVES);
    const uint64_t up = upper < 0 ? ~0ull : (uint64_t)upper;
    rc = with_kind(t->kind, [&](auto tk) {
        return launch(read_correct_kernel<decltype(tk)::value>, dim3(grid), dim3(BLOCK), 0, s, who, text, n_bytes, (const long long *)line_start, n_records,
                      first_record, k, (uint64_t)lower, up, lowercase_is_base ? 1 : 0, (uint32_t)min_qual_char, pa.dense, pa.view, out, rows,
                      (unsigned long long *)status);
    });
    return rc ? rc : check_launch(who);
}

// ---- depth of the reads of a FASTQ text (kernel: 7. of the section above); beside the read set of
// scripts/low_abd_reads.sh:10 / extract_unmapped.cpp, replacing nothing
extern "C" int pg_table_read_depths(const pg_table *t, int k, const uint8_t *text, int64_t n_bytes, const int64_t *line_start, int64_t n_records,
                                    int64_t first_record, int64_t lower, int percentile, int lowercase_is_base, int min_qual_char, uint64_t seed,
                                    int unit_log2, uint32_t *rows, uint64_t *status, void *stream)
{
    const char *who = "pg_table_read_depths";
    if (!t) return pg_fail(PG_EINVAL, "%s: t is null", who);
    if (!text) return pg_fail(PG_EINVAL, "%s: text is null", who);
    if (!line_start) return pg_fail(PG_EINVAL, "%s: line_start is null", who);
    if (!rows) return pg_fail(PG_EINVAL, "%s: rows is null", who);
    if (!status) return pg_fail(PG_EINVAL, "%s: status is null", who);
    if (n_bytes < 0) return pg_fail(PG_EINVAL, "%s: n_bytes is negative (%lld)", who, (long long)n_bytes);
    if (n_records < 0) return pg_fail(PG_EINVAL, "%s: n_records is negative (%lld)", who, (long long)n_records);
    if (first_record < 0) return pg_fail(PG_EINVAL, "%s: first_record is negative (%lld)", who, (long long)first_record);
    if (lower < 1) return pg_fail(PG_EINVAL, "%s: lower is below 1 (%lld)", who, (long long)lower);
    if (percentile < 0 || percentile > 100) return pg_fail(PG_EINVAL, "%s: percentile %d outside [0, 100]", who, percentile);
    if (min_qual_char < 0 || min_qual_char > 255) return pg_fail(PG_EINVAL, "%s: min_qual_char %d is no byte (0: none)", who, min_qual_char);
    if (unit_log2 != 0 && unit_log2 != 1) return pg_fail(PG_EINVAL, "%s: unit_log2 %d is neither 0 nor 1", who, unit_log2);
    if ((uintptr_t)text & 15) return pg_fail(PG_EINVAL, "%s: text is not 16-byte aligned", who);
    if ((uintptr_t)rows & 15) return pg_fail(PG_EINVAL, "%s: rows is not 16-byte aligned", who);
    int rc = check_table(t);
    if (rc) return rc;
    if (t->k != k) return pg_fail(PG_EINVAL, "%s: k differs (table %d, asked %d)", who, t->k, k);
    if (n_records == 0) return PG_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(uint64_t), s) != hipSuccess || hipMemsetAsync(status + 1, 0xff, sizeof(uint64_t), s) != hipSuccess)
        return pg_fail(PG_EHIP, "%s: cannot clear the status", who);
    const ProbeArgs pa = probe_args(t);
    const int grid = grid_for(n_records, WAVES);
    rc = with_kind(t->kind, [&](auto tk) {
        return launch(read_depths_kernel<decltype(tk)::value>, dim3(grid), dim3(BLOCK), 0, s, who, text, n_bytes, (const long long *)line_start,
                      n_records, first_record, k, (uint64_t)lower, (uint32_t)percentile, lowercase_is_base ? 1 : 0, (uint32_t)min_qual_char, seed,
                      unit_log2, pa.dense, pa.view, (uint4 *)rows, (unsigned long long *)status);
    });
    return rc ? rc : check_launch(who);
}
